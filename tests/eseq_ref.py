"""A float64 restatement of the CNN layer on edge sequences in rows layout, written from the formula (DESIGN.md "SI count models:
CNN", formula 1), with its gradients by hand -- plain loops over windows, no autograd and none of the package's code:

    x0 = x * gate                       conv[b, s] = sum_j x0[b, s - p + j] @ W[:, :, j]^T + bias       s in [0, L1)
    pooled[b, t] = max_j act(conv)[b, t - p + j]   over the s inside [0, L1), ties to the first         t in [0, L2)
    gate1 = window max of gate (k, p), gate2 = window max of gate1 (k, p)
    y = pooled * gate2 (+ x0 when residual and L2 == L)

and the loaders of tests/golden/si_cnn.npz / si_cnn_layers.npz shared by the host and the GPU tests."""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SLOPE = 1 / 5.5


def _act(v, act):
    if act == "relu":
        return np.maximum(v, 0.0), (v > 0).astype(np.float64)
    if act == "leaky_relu":
        return np.where(v > 0, v, v * SLOPE), np.where(v > 0, 1.0, SLOPE)
    if act == "none":
        return v, np.ones_like(v)
    raise ValueError(act)


def _gate_window(g, k, p):
    B, L = g.shape
    Lo = L + 2 * p - k + 1
    out = np.zeros((B, Lo))
    for s in range(Lo):
        lo, hi = max(s - p, 0), min(s - p + k - 1, L - 1)
        out[:, s] = g[:, lo:hi + 1].max(axis=1)
    return out


def layer_forward(x, gate, W, bias, p, act, residual):
    """(y [B, L2, C], gate2 [B, L2], the saved pieces) in float64."""
    x, gate, W, bias = (np.asarray(a, dtype=np.float64) for a in (x, gate, W, bias))
    B, L, C = x.shape
    k = W.shape[2]
    L1 = L + 2 * p - k + 1
    L2 = L1 + 2 * p - k + 1
    x0 = x * gate[:, :, None]
    conv = np.tile(bias, (B, L1, 1))
    for s in range(L1):
        for j in range(k):
            r = s - p + j
            if 0 <= r < L:
                conv[:, s] += x0[:, r] @ W[:, :, j].T
    a, da = _act(conv, act)
    pooled = np.full((B, L2, C), -np.inf)
    win = np.zeros((B, L2, C), dtype=np.int64)                   # the conv position that won
    for t in range(L2):
        for j in range(k):
            s = t - p + j
            if 0 <= s < L1:
                better = a[:, s] > pooled[:, t]
                pooled[:, t] = np.where(better, a[:, s], pooled[:, t])
                win[:, t] = np.where(better, s, win[:, t])
    g2 = _gate_window(_gate_window(gate, k, p), k, p)
    y = pooled * g2[:, :, None]
    res = bool(residual) and L2 == L
    if res:
        y = y + x0
    return y, g2, dict(x0=x0, da=da, win=win, g2=g2, gate=gate, W=W, p=p, res=res, L1=L1)


def layer_backward(saved, dy):
    """(dx, dW, dbias) of sum(y * coef) given dy = coef, float64."""
    dy = np.asarray(dy, dtype=np.float64)
    x0, da, win, g2, gate, W, p, res, L1 = (saved[k] for k in ("x0", "da", "win", "g2", "gate", "W", "p", "res", "L1"))
    B, L, C = x0.shape
    k = W.shape[2]
    dpool = dy * g2[:, :, None]
    dconv = np.zeros((B, L1, C))
    bi, ci = np.meshgrid(np.arange(B), np.arange(C), indexing="ij")
    for t in range(dy.shape[1]):
        np.add.at(dconv, (bi, win[:, t], ci), dpool[:, t])
    dconv = dconv * da
    dW = np.zeros_like(W)
    dx0 = np.zeros_like(x0)
    for s in range(L1):
        for j in range(k):
            r = s - p + j
            if 0 <= r < L:
                dW[:, :, j] += dconv[:, s].T @ x0[:, r]
                dx0[:, r] += dconv[:, s] @ W[:, :, j]
    if res:
        dx0 = dx0 + dy
    return dx0 * gate[:, :, None], dW, dconv.sum(axis=(0, 1))


# ---- the golden files ----
def load_cases():
    """Every case of si_cnn.npz and si_cnn_layers.npz: [(meta dict, {key: array})]."""
    cases = []
    for fname in ("si_cnn.npz", "si_cnn_layers.npz"):
        z = np.load(os.path.join(GOLDEN, fname))
        for m in json.loads(bytes(z["meta"]).decode()):
            arrs = {}
            for key, kind, off, shape in m["index"]:
                n = int(np.prod(shape)) if shape else 1
                a = z["%s/%s" % (m["tag"], kind)][off:off + n].reshape(shape)
                arrs[key] = a.astype(bool) if kind == "u8" else a
            cases.append((m, arrs))
    return cases


def close(got, want, what, rel=1e-4):
    """The project's bound for fp32 against fp32 goldens: 1e-4 of the tensor's largest magnitude; bool / integer tensors exact."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, "%s: shape %s vs %s" % (what, got.shape, want.shape)
    if want.dtype == bool or want.dtype.kind in "iu":
        assert np.array_equal(got, want), "%s differs" % what
        return
    scale = max(float(np.abs(want).max()), 1e-30) if want.size else 1.0
    err = float(np.abs(got.astype(np.float64) - want.astype(np.float64)).max()) if want.size else 0.0
    assert err <= rel * scale, "%s: max error %.3e over the bound %.3e (scale %.3e)" % (what, err, rel * scale, scale)
