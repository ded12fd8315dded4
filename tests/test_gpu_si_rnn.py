"""The RNN count model on edge sequences on the GPU: dn_eseq_rnn.hip behind ops.eseq_rnn and the model on both paths.

* the reference's goldens (tests/golden/si_rnn*.npz) on the fused and on the composed path: every OutputDict tensor, every gradient;
  no case skipped on either path (a case outside the kernels' predicate -- Hd = 8 -- runs composed by itself); the KernelTimer tags
  show which path ran;
* op level against torch's own nn.LSTM / nn.GRU / nn.RNN in float64 on the CPU with the same weights, x, gate and loss coefficients,
  forward and every gradient: cell x direction x Hd in {16, 32, 64} x residual, B = 33 (tiles of 16, 16 and 1), L = 70 with lengths
  70, 0 (an all-ones mask, as len_mask gives it), 1 (69 bias-driven pad steps before the only live one), 2, 3, 15, 16, 17, 40, 69 and
  random others, gate zeros at the first, the last and two interior live positions of one sequence, one sequence whose every gate is
  zero, biases of both signs; B = 1, L = 1 and L = 2 as batches of their own;
* forward and gradients bit-identical across two runs; fused against composed on the GPU; a bf16 input, Hd = 8, Hd = 128 and
  training-mode dropout take the composed path (seen through the tags) and match; requires_grad off on x, or on the weights, leaves
  the remaining gradients unchanged bit for bit.

The bound: 1e-4 of each tensor's largest magnitude, masks exact.  Inputs: weights uniform in +-1 / sqrt(Hd), biases uniform in +-0.5,
standard-normal x and coefficients; at these scales torch's own fp32 run of this grid on the CPU lies at most 1.8e-6 from its fp64
run, so the bound leaves fifty-fold room for another summation order and the device's expf / tanhf."""
import numpy as np
import pytest
import torch

import eseq_ref as R
from test_si_rnn_host import LAYERS, MODELS, check_layer, check_model, run_layer, run_model

pytestmark = pytest.mark.gpu
DEV = "cuda"
CELLS = ["LSTM", "GRU", "RNN"]
GATES = {"LSTM": 4, "GRU": 3, "RNN": 1}
FUSED_TAGS = {"eseq_rnn_proj", "eseq_rnn_fwd", "eseq_rnn_bwd", "eseq_rnn_wgrad"}
NAMES = ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")
FIXED_LENS = [70, 0, 1, 2, 3, 15, 16, 17, 40, 69]


def _ops():
    from dummynode4graphlearning_amd import ops
    return ops


def _tags(fn):
    ops = _ops()
    with ops.KernelTimer() as t:
        out = fn()
    torch.cuda.synchronize()
    return out, {r[0] for r in t.records}


def _names(bi):
    return [n + s for s in (("", "_reverse") if bi else ("",)) for n in NAMES]


# ---------------------------------------------------------------------------------------------- goldens
@pytest.mark.parametrize("path", ["fused", "composed"])
@pytest.mark.parametrize("case", MODELS, ids=[m["name"] for m, _ in MODELS])
def test_model_goldens(case, path):
    ops = _ops()
    m, arrs = case
    with ops.eseq_fused(path == "fused"):
        (model, res), tags = _tags(lambda: run_model(m, arrs, DEV))
    check_model(m, arrs, model, res)
    cfg = m["cfg"]
    kernels_apply = cfg["hid_dim"] // (2 if cfg["rep_rnn_bidirectional"] else 1) in ops.ESEQ_RNN_WIDTHS
    assert (FUSED_TAGS <= tags) == (path == "fused" and kernels_apply), tags
    assert ("eseq_rnn_composed" in tags) == (path == "composed" or not kernels_apply), tags
    assert ("eseq_filter_gate" in tags) == (path == "fused"), tags


@pytest.mark.parametrize("path", ["fused", "composed"])
@pytest.mark.parametrize("case", LAYERS, ids=[m["name"] for m, _ in LAYERS])
def test_layer_goldens(case, path):
    m, arrs = case
    if path == "fused":
        (layer, _, y, dx), tags = _tags(lambda: run_layer(m, arrs, DEV, fused=True))
        assert FUSED_TAGS <= tags and "eseq_rnn_composed" not in tags, tags
    else:
        layer, _, y, dx = run_layer(m, arrs, DEV)
    check_layer(m, arrs, layer, y, dx)


# ---------------------------------------------------------------------------------------------- op level
def _op_inputs(cell, bi, Hd, seed, B=33, L=70, lens=None, H=None):
    rng = np.random.default_rng(seed)
    D, G = (2 if bi else 1), GATES[cell]
    H = D * Hd if H is None else H
    if lens is None:
        lens = (FIXED_LENS + [40] + [int(v) for v in rng.integers(1, L + 1, size=B)])[:B] if L == 70 else [int(v) for v in rng.integers(0, L + 1, size=B)]
    gate = np.zeros((B, L), np.float32)
    for b, n in enumerate(lens):
        gate[b, L - (n if n > 0 else L):] = 1.0                     # length 0: an all-ones mask
    if L == 70 and B > 10:
        gate[0, [0, 23, 51, L - 1]] = 0.0                           # first, two interior, last live position
        gate[10] = 0.0                                              # every gate zero (its length stays 40)
        gate[11, L - lens[11]:] = (rng.random(lens[11]) < 0.6)      # filter zeros inside a sequence
    a = 1.0 / np.sqrt(Hd)
    params = {}
    for n in _names(bi):
        shape = (G * Hd, H) if "weight_ih" in n else ((G * Hd, Hd) if "weight_hh" in n else (G * Hd,))
        params[n] = rng.uniform(-a, a, size=shape).astype(np.float32) if "weight" in n else rng.uniform(-0.5, 0.5, size=shape).astype(np.float32)
    x = rng.standard_normal((B, L, H)).astype(np.float32)
    coef = rng.standard_normal((B, L, D * Hd)).astype(np.float32)
    return dict(x=x, gate=gate, lens=lens, params=params, coef=coef, cell=cell, bi=bi, Hd=Hd, H=H)


def _run_op(d, residual, fused=True, x_grad=True, w_grad=True, dtype=torch.float32):
    ops = _ops()
    xt = torch.from_numpy(d["x"]).to(DEV, dtype).requires_grad_(x_grad)
    pt = {n: torch.from_numpy(a).to(DEV, dtype).requires_grad_(w_grad) for n, a in d["params"].items()}
    gt = torch.from_numpy(d["gate"]).to(DEV)
    lens = [n if n > 0 else d["x"].shape[1] for n in d["lens"]]
    if fused:
        with ops.eseq_fused(True):
            y = ops.eseq_rnn(xt, lens, pt, gt, d["cell"], d["bi"], residual)
    else:
        y = ops.launch_tagged("eseq_rnn_composed", lambda: ops.eseq_rnn_composed(xt, pt, gt, d["cell"], d["bi"], residual))
    (y.float() * torch.from_numpy(d["coef"]).to(DEV)).sum().backward()
    out = {"y": y.detach().float().cpu().numpy()}
    if x_grad:
        out["dx"] = xt.grad.float().cpu().numpy()
    if w_grad:
        for n, t in pt.items():
            out["d" + n] = t.grad.float().cpu().numpy()
    return out


_REF = {}


def _reference(d, residual, key):
    """torch's own module in float64 on the CPU; computed once per (inputs, residual)."""
    k = (key, residual)
    if k not in _REF:
        mod = {"LSTM": torch.nn.LSTM, "GRU": torch.nn.GRU, "RNN": torch.nn.RNN}[d["cell"]](
            d["H"], d["Hd"], bidirectional=d["bi"], batch_first=True).double()
        with torch.no_grad():
            for n, a in d["params"].items():
                getattr(mod, n).copy_(torch.from_numpy(a).double())
        x = torch.from_numpy(d["x"]).double().requires_grad_(True)
        g = torch.from_numpy(d["gate"]).double().unsqueeze(-1)
        x0 = x * g
        y = mod(x0)[0] * g
        if residual and y.shape == x0.shape:
            y = y + x0
        (y * torch.from_numpy(d["coef"]).double()).sum().backward()
        out = {"y": y.detach().numpy(), "dx": x.grad.numpy()}
        for n in d["params"]:
            out["d" + n] = getattr(mod, n).grad.numpy()
        _REF[k] = out
    return _REF[k]


def _close_all(got, want, what):
    assert set(got) <= set(want)
    for k in got:
        R.close(got[k], want[k], "%s %s" % (what, k))


@pytest.mark.parametrize("Hd", [16, 32, 64])
@pytest.mark.parametrize("bi", [False, True], ids=["uni", "bi"])
@pytest.mark.parametrize("cell", CELLS)
def test_op_against_torch_float64(cell, bi, Hd):
    ops = _ops()
    key = (cell, bi, Hd, "grid")
    d = _op_inputs(cell, bi, Hd, 1000 + 7 * Hd + 2 * CELLS.index(cell) + bi)
    assert d["lens"][:10] == FIXED_LENS and len(d["lens"]) == 33
    for n in _names(bi):
        if "bias" in n:
            assert (d["params"][n] > 0).any() and (d["params"][n] < 0).any()
    assert ops.eseq_rnn_supported(torch.from_numpy(d["x"]).to(DEV), {n: torch.from_numpy(a).to(DEV) for n, a in d["params"].items()}, cell, bi)
    for residual in (True, False):
        got, tags = _tags(lambda: _run_op(d, residual))
        assert FUSED_TAGS <= tags and "eseq_rnn_composed" not in tags, tags
        want = _reference(d, residual, key)
        _close_all(got, want, "%s bi=%s Hd=%d res=%s" % (cell, bi, Hd, residual))
        assert not got["y"][10].any()                                # the all-zero-gate sequence: exact zeros
        assert not got["y"][2, :69].any() and got["y"][2, 69].any()  # length 1: the pad steps are gated out, the live step is not
        assert got["y"][1].all()                                     # length 0: every position is live
        assert not got["dx"][10].any() and not got["dx"][2, :69].any()


@pytest.mark.parametrize("shape", [(1, 70), (5, 1), (19, 2)], ids=["B1", "L1", "L2"])
@pytest.mark.parametrize("cell", CELLS)
def test_op_with_one_sequence_and_with_one_and_two_steps(cell, shape):
    B, L = shape
    for bi in (False, True):
        lens = [L] if B == 1 else None
        d = _op_inputs(cell, bi, 32, 50 + B + L + bi, B=B, L=L, lens=lens)
        want = _reference(d, True, (cell, bi, B, L))
        _close_all(_run_op(d, True), want, "%s bi=%s B=%d L=%d" % (cell, bi, B, L))


def test_input_width_other_than_the_output_width_drops_the_residual():
    d = _op_inputs("GRU", True, 48, 77, H=64)                         # D Hd = 96 != H = 64; Hd = 48: three waves
    want = _reference(d, True, ("GRU", True, 48, "H64"))
    _close_all(_run_op(d, True), want, "GRU bi Hd=48 H=64")
    assert want["y"].shape == (33, 70, 96)


@pytest.mark.parametrize("cell", CELLS)
def test_forward_and_gradients_are_bitwise_reproducible(cell):
    d = _op_inputs(cell, True, 64, 3)
    a, b = _run_op(d, True), _run_op(d, True)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    ops = _ops()
    m, arrs = next(c for c in MODELS if c[0]["name"] == "gru_bi")
    runs = []
    for _ in range(2):
        with ops.eseq_fused(True):
            model, res = run_model(m, arrs, DEV)
        runs.append([res["pred_c"].detach().cpu(), res["g_e_rep"].detach().cpu()] + [q.grad.cpu() for q in model.parameters()
                                                                                    if q.grad is not None])
    for u, v in zip(*runs):
        assert torch.equal(u, v)


@pytest.mark.parametrize("bi", [False, True], ids=["uni", "bi"])
@pytest.mark.parametrize("cell", CELLS)
def test_fused_and_composed_agree(cell, bi):
    d = _op_inputs(cell, bi, 32, 21 + bi)
    a = _run_op(d, True)
    b, tags = _tags(lambda: _run_op(d, True, fused=False))
    assert "eseq_rnn_composed" in tags and not (FUSED_TAGS & tags)
    _close_all(a, b, "fused vs composed %s bi=%s" % (cell, bi))


@pytest.mark.parametrize("cell", CELLS)
def test_requires_grad_off_leaves_the_other_gradients_unchanged(cell):
    d = _op_inputs(cell, True, 16, 41)
    full = _run_op(d, True)
    no_x = _run_op(d, True, x_grad=False)
    no_w = _run_op(d, True, w_grad=False)
    assert "dx" not in no_x and set(no_w) == {"y", "dx"}
    for k in no_x:
        assert np.array_equal(no_x[k], full[k]), k
    for k in no_w:
        assert np.array_equal(no_w[k], full[k]), k


def test_cases_outside_the_predicate_take_the_composed_path_and_match():
    ops = _ops()
    from dummynode4graphlearning_amd.subgraph_isomorphism import RNNLayer

    def composed_only(d, dtype=torch.float32):
        got, tags = _tags(lambda: _run_op(d, True, dtype=dtype))
        assert "eseq_rnn_composed" in tags and not (FUSED_TAGS & tags), tags
        return got

    # a bf16 input
    d = _op_inputs("LSTM", False, 32, 31, B=5, L=9)
    got = composed_only(d, torch.bfloat16)
    want = _reference(d, True, "bf16")
    assert float(np.abs(got["y"] - want["y"]).max()) <= 0.05 * float(np.abs(want["y"]).max())      # (bf16: 8 bits of mantissa)
    # Hd = 8 and Hd = 128
    for Hd, bi in ((8, True), (128, False)):
        d = _op_inputs("GRU", bi, Hd, 32 + Hd, B=5, L=9)
        pt = {n: torch.from_numpy(a).to(DEV) for n, a in d["params"].items()}
        assert not ops.eseq_rnn_supported(torch.from_numpy(d["x"]).to(DEV), pt, "GRU", bi)
        _close_all(composed_only(d), _reference(d, True, ("Hd", Hd)), "Hd=%d" % Hd)
    # layer norm, and dropout in training mode: the layer refuses the kernels; in eval mode it takes them
    x = torch.zeros(2, 9, 32, device=DEV)
    assert RNNLayer("LSTM", 32, 32).to(DEV).train().fused_ok(x)
    assert not RNNLayer("LSTM", 32, 32, layer_norm=True).to(DEV).fused_ok(x)
    drop = RNNLayer("LSTM", 32, 32, dropout=0.5).to(DEV)
    assert not drop.train().fused_ok(x) and drop.eval().fused_ok(x)
    m, arrs = next(c for c in MODELS if c[0]["name"] == "dropout_eval")
    m = dict(m, mode="train")
    runs = []
    for fused in (True, False):
        torch.manual_seed(5)
        with ops.eseq_fused(fused):
            (model, res), tags = _tags(lambda: run_model(m, arrs, DEV))
        assert "eseq_rnn_composed" in tags and "eseq_rnn_fwd" not in tags, tags
        runs.append(res)
    for k in ("g_e_rep", "p_e_rep", "pred_c"):                         # the same dropout draws on both runs
        R.close(runs[0][k].detach().cpu().numpy(), runs[1][k].detach().cpu().numpy(), "training-mode dropout " + k)
    assert not torch.equal(runs[0]["g_e_rep"].detach().cpu(), torch.from_numpy(arrs["out/g_e_rep"]))
