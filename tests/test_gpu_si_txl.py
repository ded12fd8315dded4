"""The TransformerXL count model on edge sequences on the GPU: dn_txl.hip behind ops.txl_attention and the model on both paths.

* the reference's goldens (tests/golden/si_txl*.npz) on the fused and on the composed path: every OutputDict tensor, every gradient; no
  case skipped on either path (a case outside the kernels' predicate -- a head width of 4 -- runs composed by itself); the
  KernelTimer tags show which path ran;
* op level against the float64 restatement of txl_ref.py on the CPU, forward and every gradient (q, k, v, k_mem, v_mem, rk, r_w_bias,
  r_r_bias), B = 3, (heads, head width) in {(1, 64), (4, 16), (2, 32), (1, 16)} x the shapes Lp = 192 at seg 64 / mem 64 (windows of
  64, 128, 128), Lp = 64 (no memory), Lp = 128 at mem 32 (a 96-key window), seg 16 / mem 0 at Lp = 48, seg 16 / mem 16, seg 48 / mem
  64 (windows of 48, 96, 112) and B = 1.  In every batch of three, sequence 1 has all-zero q, k, v rows: its softmax still runs over
  every key.  One case per (heads, width) has q scaled by 12, so that the scores reach about +-60 (the max subtraction), one has
  r_r_bias ten times larger, so that the shifted term and its wrapped entries dominate;
* forward and gradients bit-identical over two runs; requires_grad off on q, on the memory parts or on the biases leaves the other
  gradients unchanged bit for bit; a bf16 input, a head width of 8, seg 24 and training-mode dropout take the composed path (seen
  through the tags) and match.

The bound: 1e-4 of each tensor's largest magnitude, masks exact.  Inputs: standard-normal q, k, v, rk and coefficients, biases 0.5
N(0, 1), scale = 1 / sqrt(width).  At these scales torch's own fp32 run of this grid on the CPU (ops.txl_attention_composed) lies at
most 4.1e-6 of a tensor's largest magnitude from the fp64 restatement (the plain cases 1.6e-6, the sharp-score cases 4.1e-6, the
large-r_r_bias cases 2.4e-6), so the bound leaves twenty-four-fold room for another summation order and the device's expf."""
import numpy as np
import pytest
import torch

import eseq_ref as R
import txl_ref as T
from test_si_txl_host import LAYERS, MODELS, check_layer, check_model, run_layer, run_model

pytestmark = pytest.mark.gpu
DEV = "cuda"
FUSED_TAGS = {"txl_proj", "txl_attn_fwd", "txl_attn_bwd"}
ND = [(1, 64), (4, 16), (2, 32), (1, 16)]
# name: (B, Lp, seg, mem)
SHAPES = {"L192_seg64_mem64": (3, 192, 64, 64), "L64_no_memory": (3, 64, 64, 64), "L128_mem32": (3, 128, 64, 32),
          "seg16_mem0": (3, 48, 16, 0), "seg16_mem16": (3, 64, 16, 16), "seg48_mem64": (3, 144, 48, 64), "B1": (1, 128, 64, 64)}
VARIANTS = [(s, "plain") for s in SHAPES] + [("L128_mem32", "sharp"), ("seg48_mem64", "rrb10")]
NAMES = ("q", "k", "v", "k_mem", "v_mem", "rk", "r_w_bias", "r_r_bias")


def _ops():
    from dummynode4graphlearning_amd import ops
    return ops


def _tags(fn):
    ops = _ops()
    with ops.KernelTimer() as t:
        out = fn()
    torch.cuda.synchronize()
    return out, {r[0] for r in t.records}


def _kernels_apply(cfg):
    return cfg["hid_dim"] // cfg.get("num_heads", 1) in _ops().TXL_HEAD_WIDTHS


# ---------------------------------------------------------------------------------------------- goldens
@pytest.mark.parametrize("path", ["fused", "composed"])
@pytest.mark.parametrize("case", MODELS, ids=[m["name"] for m, _ in MODELS])
def test_model_goldens(case, path):
    ops = _ops()
    m, arrs = case
    with ops.eseq_fused(path == "fused"):
        (model, res), tags = _tags(lambda: run_model(m, arrs, DEV))
    check_model(m, arrs, model, res)
    fused = path == "fused" and _kernels_apply(m["cfg"])
    assert (FUSED_TAGS <= tags) == fused and ("txl_attn_fwd" in tags) == fused, tags
    assert ("txl_composed" in tags) == (not fused), tags
    assert ("eseq_filter_gate" in tags) == (path == "fused"), tags


def test_without_the_switch_the_layers_take_their_own_default():
    ops = _ops()
    m, arrs = MODELS[0]
    (model, res), tags = _tags(lambda: run_model(m, arrs, DEV))
    check_model(m, arrs, model, res)
    assert ("txl_attn_fwd" in tags) == ops.TXL_FUSED_DEFAULT and ("txl_composed" in tags) != ops.TXL_FUSED_DEFAULT, tags


def test_the_goldens_hold_cases_on_both_sides_of_the_predicate():
    inside = [m["name"] for m, _ in MODELS if _kernels_apply(m["cfg"])]
    outside = [m["name"] for m, _ in MODELS if not _kernels_apply(m["cfg"])]
    assert {"defaults", "heads4", "pre_lnorm", "mem32", "seg16", "clamp20", "layers1", "no_share", "dropout_eval"} <= set(inside)
    assert "layers3" in outside                                          # 4 heads of width 4: composed by itself
    assert any(m["heads"] == 4 and m["H"] == 64 for m, _ in LAYERS)


@pytest.mark.parametrize("path", ["fused", "composed"])
@pytest.mark.parametrize("case", LAYERS, ids=[m["name"] for m, _ in LAYERS])
def test_layer_goldens(case, path):
    m, arrs = case
    if path == "fused":
        (layer, _, y, grads), tags = _tags(lambda: run_layer(m, arrs, DEV, fused=True))
        assert FUSED_TAGS <= tags and "txl_composed" not in tags, tags
    else:
        layer, _, y, grads = run_layer(m, arrs, DEV)
    check_layer(m, arrs, layer, y, grads)


# ---------------------------------------------------------------------------------------------- op level
def op_inputs(shape, n, d, variant="plain"):
    B, Lp, seg, mem = SHAPES[shape]
    rng = np.random.default_rng(1000 + 7 * d + n + 13 * list(SHAPES).index(shape))
    f = lambda *s: rng.standard_normal(s).astype(np.float32)  # noqa: E731
    a = dict(q=f(B, Lp, n, d), k=f(B, Lp, n, d), v=f(B, Lp, n, d), rk=f(seg + mem, n, d), r_w_bias=0.5 * f(n, d), r_r_bias=0.5 * f(n, d))
    a["k_mem"], a["v_mem"] = a["k"] + 0.1 * f(B, Lp, n, d), a["v"] + 0.1 * f(B, Lp, n, d)       # (the op does not need them equal)
    if B > 1:
        for key in ("q", "k", "v", "k_mem", "v_mem"):
            a[key][1] = 0.0                                               # sequence 1: all-zero rows
    if variant == "sharp":
        a["q"] = a["q"] * 12.0
    if variant == "rrb10":
        a["r_r_bias"] = a["r_r_bias"] * 10.0
    return dict(arrays={k: a[k] for k in NAMES}, coef=f(B, Lp, n * d), seg=seg, mem=mem, scale=1.0 / np.sqrt(d))


def run_op(d, device=DEV, dtype=torch.float32, no_grad=(), composed=False):
    ops = _ops()
    ts = {k: torch.from_numpy(a).to(device, dtype).requires_grad_(k not in no_grad) for k, a in d["arrays"].items()}
    args = [ts[k] for k in NAMES] + [d["seg"], d["mem"], d["scale"]]
    if composed:
        y = ops.launch_tagged("txl_composed", lambda: ops.txl_attention_composed(*args))
    else:
        y = ops.txl_attention(*args)                                      # (the op picks its kernels by its predicate alone)
    (y.float() * torch.from_numpy(d["coef"]).to(device)).sum().backward()
    out = {"out": y.detach().float().cpu().numpy()}
    for k, t in ts.items():
        if t.grad is not None:
            out["d" + k] = t.grad.float().cpu().numpy()
    return out


_REF = {}


def reference(d, key):
    """txl_ref.attention in float64 on the CPU; computed once per case."""
    if key not in _REF:
        ts = {k: torch.from_numpy(a).double().requires_grad_(True) for k, a in d["arrays"].items()}
        y = T.attention(*[ts[k] for k in NAMES], d["seg"], d["mem"], float(d["scale"]))
        (y * torch.from_numpy(d["coef"]).double()).sum().backward()
        out = {"out": y.detach().numpy()}
        for k, t in ts.items():
            out["d" + k] = t.grad.numpy() if t.grad is not None else np.zeros(t.shape)
        _REF[key] = out
    return _REF[key]


def _close_all(got, want, what):
    assert set(got) <= set(want)
    for k in got:
        R.close(got[k], want[k], "%s %s" % (what, k))


@pytest.mark.parametrize("nd", ND, ids=lambda v: "n%d_d%d" % v)
@pytest.mark.parametrize("shape,variant", VARIANTS, ids=["%s-%s" % v for v in VARIANTS])
def test_op_against_the_float64_restatement(shape, variant, nd):
    ops = _ops()
    n, w = nd
    d = op_inputs(shape, n, w, variant)
    ts = [torch.from_numpy(d["arrays"][k]).to(DEV) for k in NAMES]
    assert ops.txl_attention_supported(*ts, d["seg"], d["mem"])
    got, tags = _tags(lambda: run_op(d))
    assert {"txl_attn_fwd", "txl_attn_bwd"} <= tags and "txl_composed" not in tags, tags
    want = reference(d, (shape, variant, nd))
    assert all(np.isfinite(v).all() for v in got.values())
    if d["mem"] == 0:                                                    # no memory: its tensors get no gradient at all
        assert "dk_mem" not in got and "dv_mem" not in got
    elif SHAPES[shape][1] == d["seg"]:                                   # one segment: no window reaches a memory row
        assert not got["dk_mem"].any() and not got["dv_mem"].any()
    else:
        assert got["dk_mem"].any() and not got["dk_mem"][:, -d["seg"]:].any()
    _close_all(got, want, "%s %s n=%d d=%d" % (shape, variant, n, w))
    if SHAPES[shape][0] > 1:                                              # the all-zero sequence: uniform attention over zero values
        assert not got["out"][1].any()
    if variant == "sharp":
        a = d["arrays"]
        s = np.einsum("ind,jnd->ijn", a["q"][0, :d["seg"]] + a["r_w_bias"], a["k"][0, :d["seg"]]) * d["scale"]
        assert 30 < np.abs(s).max() < 150


def test_forward_and_gradients_are_bitwise_reproducible():
    for shape, nd in (("L192_seg64_mem64", (1, 64)), ("seg48_mem64", (4, 16))):
        d = op_inputs(shape, *nd)
        a, b = run_op(d), run_op(d)
        assert set(a) == {"out"} | {"d" + k for k in NAMES}
        for k in a:
            assert np.array_equal(a[k], b[k]), k
    ops = _ops()
    m, arrs = next(c for c in MODELS if c[0]["name"] == "heads4")
    runs = []
    for _ in range(2):
        with ops.eseq_fused(True):
            model, res = run_model(m, arrs, DEV)
        runs.append([res["pred_c"].detach().cpu(), res["g_e_rep"].detach().cpu()] + [q.grad.cpu() for q in model.parameters()
                                                                                    if q.grad is not None])
    for u, v in zip(*runs):
        assert torch.equal(u, v)


@pytest.mark.parametrize("off", [("q",), ("k_mem", "v_mem"), ("r_w_bias", "r_r_bias"), ("rk", "k", "v")], ids=lambda v: "+".join(v))
def test_requires_grad_off_leaves_the_other_gradients_unchanged(off):
    d = op_inputs("L192_seg64_mem64", 2, 32)
    full, part = run_op(d), run_op(d, no_grad=off)
    assert set(part) == set(full) - {"d" + k for k in off}
    for k in part:
        assert np.array_equal(part[k], full[k]), k


def test_fused_and_composed_agree():
    for shape, nd in (("L128_mem32", (2, 32)), ("seg16_mem16", (1, 16))):
        d = op_inputs(shape, *nd)
        b, tags = _tags(lambda: run_op(d, composed=True))
        assert "txl_composed" in tags and "txl_attn_fwd" not in tags
        _close_all(run_op(d), b, "fused vs composed %s" % shape)


def test_cases_outside_the_predicate_take_the_composed_path_and_match():
    ops = _ops()

    def composed_only(d, dtype=torch.float32):
        got, tags = _tags(lambda: run_op(d, dtype=dtype))
        assert "txl_composed" in tags and not ({"txl_attn_fwd", "txl_attn_bwd"} & tags), tags
        return got

    # a bf16 input
    d = op_inputs("seg16_mem16", 1, 16)
    got = composed_only(d, torch.bfloat16)
    want = reference(d, "bf16")
    assert float(np.abs(got["out"] - want["out"]).max()) <= 0.05 * float(np.abs(want["out"]).max())     # (bf16: 8 bits of mantissa)
    # a head width of 8; a segment length of 24 (with a memory of 24: windows of 24 and 48)
    d = op_inputs("seg16_mem16", 2, 8)
    assert not ops.txl_attention_supported(*[torch.from_numpy(d["arrays"][k]).to(DEV) for k in NAMES], d["seg"], d["mem"])
    _close_all(composed_only(d), reference(d, "d8"), "d=8")
    SHAPES["seg24"] = (3, 72, 24, 24)
    try:
        d = op_inputs("seg24", 1, 16)
    finally:
        del SHAPES["seg24"]
    assert not ops.txl_attention_supported(*[torch.from_numpy(d["arrays"][k]).to(DEV) for k in NAMES], d["seg"], d["mem"])
    _close_all(composed_only(d), reference(d, "seg24"), "seg=24")
    # dropout in training mode: the model stays on the segment loop; in eval mode it takes the kernels
    m, arrs = next(c for c in MODELS if c[0]["name"] == "dropout_eval")
    with ops.eseq_fused(True):
        _, tags = _tags(lambda: run_model(m, arrs, DEV))
    assert "txl_attn_fwd" in tags
    m = dict(m, mode="train")
    runs = []
    for fused in (True, False):
        torch.manual_seed(5)
        with ops.eseq_fused(fused):
            (model, res), tags = _tags(lambda: run_model(m, arrs, DEV))
        assert "txl_composed" in tags and "txl_attn_fwd" not in tags, tags
        runs.append(res)
    for k in ("g_e_rep", "p_e_rep", "pred_c"):                         # the same dropout draws on both runs
        R.close(runs[0][k].detach().cpu().numpy(), runs[1][k].detach().cpu().numpy(), "training-mode dropout " + k)
    assert not torch.equal(runs[0]["g_e_rep"].detach().cpu(), torch.from_numpy(arrs["out/g_e_rep"]))
