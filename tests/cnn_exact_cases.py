"""The operands of the exact CNN-layer parity tests (tests/test_si_cnn_exact_premise.py on the CPU, tests/test_gpu_si_cnn_exact.py on
the GPU): small integers, so that every product, every partial sum in any order and every result of the layer and of its gradients is
an integer below 2^24 -- fp32 then computes them without rounding, and a kernel is held to the float64 restatement
(tests/eseq_ref.py) bit for bit.

    x in [-3, 3], W in [-2, 2] with half of its entries 0, bias in [-4, 4], loss coefficients in [-3, 3], gate 0 / 1.

With so few distinct values two slots of a max window often tie at a value that carries a gradient (about 3 % of the live outputs), so
the "ties go to the first slot" rule of the forward kernel and of the dconv gather decides bits here.

B = 8 right-aligned sequences in L = 70 positions: two output tiles of 64 - (k - 1), two input-gradient tiles of 64, three
weight-gradient tiles of 32 conv rows; lengths 70, 0 (every gate zero, lens[b] = 0), 1, 2, max(k - 1, 1), k, 63 and 40.  Sequence 0
has gate zeros at its first, two interior and its last live position; the length-40 sequence keeps about 60 % of its positions.  At
k = 5, padding 0 the first output tile of the short sequences lies left of their support (a dead tile)."""
import numpy as np

import eseq_ref as R

B, L = 8, 70
WIDTHS = [16, 32, 48, 64, 80, 96, 112, 128]
KP = [(2, 0), (2, 1), (3, 0), (3, 1), (4, 0), (4, 1), (4, 2), (5, 0), (5, 1), (5, 2)]
ACTS = ["relu", "none"]
KEEPS_LENGTH = [(3, 1), (5, 2)]                                       # L2 == L: the residual applies
NAMES = ("y", "gate_out", "dx", "dW", "dbias")


def kp_id(kp):
    return "k%d_p%d" % kp


def out_len(k, p):
    return L + 4 * p - 2 * k + 2


def lengths(k):
    return [70, 0, 1, 2, max(k - 1, 1), k, 63, 40]


_INPUTS = {}


def inputs(C, k, p):
    """dict(x, gate, lens, W, bias, coef) of the case; built once per (C, k, p) and never changed."""
    key = (C, k, p)
    if key not in _INPUTS:
        rng = np.random.default_rng(7000 + 100 * C + 10 * k + p)
        lens = lengths(k)
        gate = np.zeros((B, L), np.float32)
        for b, n in enumerate(lens):
            gate[b, L - n:] = 1.0
        gate[0, [0, 23, 51, L - 1]] = 0.0                             # first, two interior, last live position
        gate[7, L - 40:] = rng.random(40) < 0.6                       # filter zeros inside a sequence
        x = rng.integers(-3, 4, size=(B, L, C)).astype(np.float32)
        W = (rng.integers(-2, 3, size=(C, C, k)) * (rng.random((C, C, k)) < 0.5)).astype(np.float32)
        bias = rng.integers(-4, 5, size=C).astype(np.float32)
        coef = rng.integers(-3, 4, size=(B, out_len(k, p), C)).astype(np.float32)
        d = dict(x=x, gate=gate, lens=lens, W=W, bias=bias, coef=coef)
        for a in d.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _INPUTS[key] = d
    return _INPUTS[key]


def reference(C, k, p, act, residual):
    """(y, gate_out, dx, dW, dbias) of the float64 restatement (each case is asked for by one test, so nothing is kept)."""
    d = inputs(C, k, p)
    y, g2, saved = R.layer_forward(d["x"], d["gate"], d["W"], d["bias"], p, act, residual)
    return (y, g2) + tuple(R.layer_backward(saved, d["coef"]))


def conv_rows(x0, W, bias, p):
    """conv [B, L1, C] in float64: bias + sum_j x0[:, s - p + j] @ W[:, :, j]^T."""
    x0, W = np.asarray(x0, np.float64), np.asarray(W, np.float64)
    k = W.shape[2]
    L1 = x0.shape[1] + 2 * p - k + 1
    conv = np.tile(np.asarray(bias, np.float64), (x0.shape[0], L1, 1))
    for s in range(L1):
        for j in range(k):
            r = s - p + j
            if 0 <= r < x0.shape[1]:
                conv[:, s] += x0[:, r] @ W[:, :, j].T
    return conv


def magnitude_bound(C, k, p, act, residual):
    """An upper bound of the magnitude of every value and of every partial sum, in any summation order, of the layer and of its
    gradients: the same formulas on the magnitudes of the operands (every product enters with its absolute value)."""
    d = inputs(C, k, p)
    x0 = np.abs(d["x"].astype(np.float64)) * d["gate"][:, :, None]
    worst = float(conv_rows(x0, np.abs(d["W"]), np.abs(d["bias"]), p).max())              # the conv rows (act and max do not grow them)
    _, _, saved = R.layer_forward(d["x"], d["gate"], d["W"], d["bias"], p, act, residual)
    saved = dict(saved, x0=x0, W=np.abs(saved["W"]), da=np.abs(saved["da"]))
    for a in R.layer_backward(saved, np.abs(d["coef"])):                                   # dconv, dx (+ dy), dW, dbias on magnitudes
        worst = max(worst, float(np.abs(a).max()))
    return worst + (float(x0.max()) if residual else 0.0)                                  # y = pooled + x0


def tie_count(C, k, p, act):
    """(live outputs whose window maximum is attained by two or more slots, live outputs): live = gate_out != 0, counted per channel."""
    d = inputs(C, k, p)
    a = R._act(conv_rows(d["x"] * d["gate"][:, :, None], d["W"], d["bias"], p), act)[0]
    g2 = R._gate_window(R._gate_window(d["gate"].astype(np.float64), k, p), k, p)
    L1, L2 = a.shape[1], g2.shape[1]
    best = np.full((B, L2, C), -np.inf)
    hits = np.zeros((B, L2, C), np.int64)
    for j in range(k):
        t = np.arange(L2)
        s = t - p + j
        ok = (s >= 0) & (s < L1)
        v = np.full((B, L2, C), -np.inf)
        v[:, ok] = a[:, s[ok]]
        hits = np.where(v > best, 1, hits + (v == best))
        best = np.maximum(best, v)
    live = np.broadcast_to(g2[:, :, None] != 0, hits.shape)
    return int(((hits >= 2) & live).sum()), int(live.sum())
