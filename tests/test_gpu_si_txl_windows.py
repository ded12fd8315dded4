"""Every window shape the predicate of ops.txl_attention admits, a position table longer than the window, and the two fixed-order sums
of the backward pass exactly (dn_txl.hip), on the inputs, the reference and the bound of tests/test_gpu_si_txl.py (txl_ref.attention
in float64 on the CPU; 1e-4 of each tensor's largest magnitude):

* all 26 (seg, mem) pairs -- seg in {16, 32, 48, 64}, mem a multiple of 16, seg + mem <= 128 -- at B = 2, 2 heads of width 16 and
  Lp = seg (ceil(mem / seg) + 2), so that the window saturates and one more segment follows (Lp = 144 at (16, 112): a memory row then
  belongs to seven later segments in txl_fold_mem_kernel).  seg = 32 (two waves sharing the key tiles) and the 128-key windows
  reached from a short segment run at op level here, the latter also at heads of width 64 and 32;
* rk with P = seg + mem + 9 rows: out and every gradient close to the reference, d rk exactly zero past the window, everything else
  bit-identical to the run on rk[:seg + mem] (txl_reduce_rk_kernel's guard is all that keeps the unwritten rows of rk_part out);
* dn_txl_fold_mem_f32 and dn_txl_reduce_rk_f32 called directly on integer-valued partial buffers whose every entry the sums must
  not read is NaN: np.array_equal to the numpy sums, finite everywhere.

torch's own fp32 run of the 26 shapes on the CPU (ops.txl_attention_composed) lies at most 1.2e-6 of a tensor's largest magnitude from
the float64 restatement (the wider heads at the 128-key windows: 7.0e-7; the long position table: 7.7e-7), so the bound leaves
eighty-fold room for another summation order and the device's expf."""
import numpy as np
import pytest
import torch

from test_gpu_si_txl import DEV, NAMES, _close_all, _tags, reference, run_op

pytestmark = pytest.mark.gpu
PAIRS = [(seg, mem) for seg in (16, 32, 48, 64) for mem in range(0, 129 - seg, 16)]
SHORT_TO_128 = [(16, 112), (32, 96), (48, 80)]


def _ops():
    from dummynode4graphlearning_amd import ops
    return ops


def seq_len(seg, mem):
    return seg * (-(-mem // seg) + 2)


def window_inputs(seg, mem, n, d, extra_rk=0, B=2):
    """As test_gpu_si_txl.op_inputs builds them: standard-normal q, k, v, rk and coefficients, biases 0.5 N(0, 1), the memory's rows
    a perturbed copy, sequence 1 all zero; rk with seg + mem + extra_rk rows."""
    Lp = seq_len(seg, mem)
    rng = np.random.default_rng(5000 + 131 * seg + 7 * mem + 3 * d + n)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)  # noqa: E731
    a = dict(q=f(B, Lp, n, d), k=f(B, Lp, n, d), v=f(B, Lp, n, d), rk=f(seg + mem, n, d), r_w_bias=0.5 * f(n, d), r_r_bias=0.5 * f(n, d))
    a["k_mem"], a["v_mem"] = a["k"] + 0.1 * f(B, Lp, n, d), a["v"] + 0.1 * f(B, Lp, n, d)
    for key in ("q", "k", "v", "k_mem", "v_mem"):
        a[key][1] = 0.0
    coef = f(B, Lp, n * d)
    if extra_rk:
        a["rk"] = np.concatenate([a["rk"], f(extra_rk, n, d)], 0)             # (drawn last: the other tensors are those of extra_rk = 0)
    return dict(arrays={k: a[k] for k in NAMES}, coef=coef, seg=seg, mem=mem, scale=1.0 / np.sqrt(d))


def _check_window(seg, mem, n, w, d, key):
    ops = _ops()
    ts = [torch.from_numpy(d["arrays"][k]).to(DEV) for k in NAMES]
    assert ops.txl_attention_supported(*ts, seg, mem)
    got, tags = _tags(lambda: run_op(d))
    assert {"txl_attn_fwd", "txl_attn_bwd"} <= tags and "txl_composed" not in tags, tags
    assert all(np.isfinite(v).all() for v in got.values())
    if mem == 0:                                                         # no memory: its tensors get no gradient at all
        assert set(got) == {"out"} | {"d" + k for k in NAMES if k not in ("k_mem", "v_mem")}
    else:
        assert set(got) == {"out"} | {"d" + k for k in NAMES}
        for k in ("dk_mem", "dv_mem"):
            assert got[k][0].any() and not got[k][:, -seg:].any(), k    # the last segment is nobody's memory
    _close_all(got, reference(d, key), "seg %d mem %d n=%d d=%d" % (seg, mem, n, w))
    assert not got["out"][1].any()                                       # the all-zero sequence: uniform attention over zero values
    return got


@pytest.mark.parametrize("seg,mem", PAIRS, ids=["seg%d_mem%d" % p for p in PAIRS])
def test_every_window_shape_against_the_float64_restatement(seg, mem):
    ops = _ops()
    assert len(PAIRS) == 26 and seg + mem <= ops.TXL_MAX_WINDOW and seg <= ops.TXL_MAX_SEG
    Lp = seq_len(seg, mem)
    wins = ops.txl_windows(Lp, seg, mem)
    assert wins[-2][1] == mem and wins[-1][1] == mem and (mem == 0 or wins[-3][1] < mem)     # saturated, then one more segment
    _check_window(seg, mem, 2, 16, window_inputs(seg, mem, 2, 16), ("windows", seg, mem, 2, 16))


def test_the_grid_reaches_what_it_is_for():
    assert seq_len(16, 112) == 144 and max(seq_len(*p) for p in PAIRS) == seq_len(48, 64) == seq_len(64, 64) == 192
    assert all(p in PAIRS for p in SHORT_TO_128) and [p for p in PAIRS if sum(p) == 128 and p[0] < 64] == SHORT_TO_128
    later = [sum(1 for k0, mlen, q0 in _ops().txl_windows(144, 16, 112) if k0 <= pos < q0) for pos in range(144)]
    assert max(later) == 7 and later[-16:] == [0] * 16                   # a memory row of up to seven later segments


@pytest.mark.parametrize("nd", [(1, 64), (2, 32)], ids=lambda v: "n%d_d%d" % v)
@pytest.mark.parametrize("seg,mem", SHORT_TO_128, ids=["seg%d_mem%d" % p for p in SHORT_TO_128])
def test_wider_heads_at_the_128_key_windows_of_short_segments(seg, mem, nd):
    n, w = nd
    _check_window(seg, mem, n, w, window_inputs(seg, mem, n, w), ("windows", seg, mem, n, w))


@pytest.mark.parametrize("seg,mem", [(32, 16), (64, 64)], ids=["seg32_mem16", "seg64_mem64"])
def test_a_position_table_longer_than_the_window(seg, mem):
    long = window_inputs(seg, mem, 2, 16, extra_rk=9)
    exact = window_inputs(seg, mem, 2, 16)
    assert long["arrays"]["rk"].shape[0] == seg + mem + 9 and np.array_equal(long["arrays"]["rk"][:seg + mem], exact["arrays"]["rk"])
    assert all(np.array_equal(long["arrays"][k], exact["arrays"][k]) for k in NAMES if k != "rk") and np.array_equal(long["coef"], exact["coef"])
    got = _check_window(seg, mem, 2, 16, long, ("long-rk", seg, mem))
    assert got["drk"].shape == (seg + mem + 9, 2, 16)
    assert not got["drk"][seg + mem:].any() and got["drk"][:seg + mem].any()
    want = run_op(exact)
    assert set(got) == set(want)
    for k in want:
        g = got[k][:seg + mem] if k == "drk" else got[k]
        assert np.array_equal(g, want[k]), "%s differs at %d entries from the run on rk[:seg + mem]" % (k, int((g != want[k]).sum()))


# ---------------------------------------------------------------------------------------------- the two folds, exactly
def _fold_case(seg, mem, B=2, n=2, D=16, extra=9):
    Lp, P = seq_len(seg, mem), seg + mem + extra
    S = Lp // seg
    rng = np.random.default_rng(900 + seg + mem)
    wins = [(s * seg - min(mem, s * seg), min(mem, s * seg)) for s in range(S)]         # (k0, mlen) per segment
    rk_part = rng.integers(-8, 9, size=(B, S, n, P, D)).astype(np.float32)
    drk = np.zeros((P, n, D), np.float64)
    for s, (k0, mlen) in enumerate(wins):
        klen = seg + mlen
        drk[:klen] += rk_part[:, s, :, :klen].astype(np.float64).sum(0).transpose(1, 0, 2)
        rk_part[:, s, :, klen:] = np.nan
    out = dict(Lp=Lp, P=P, S=S, rk_part=rk_part, drk=drk)
    if mem > 0:
        parts = [rng.integers(-8, 9, size=(B, S, n, mem, D)).astype(np.float32) for _ in range(2)]
        sums = [np.zeros((B, Lp, n, D), np.float64) for _ in range(2)]
        for part, total in zip(parts, sums):
            for s, (k0, mlen) in enumerate(wins):
                for pos in range(k0, s * seg):
                    total[:, pos] += part[:, s, :, pos - k0]
                part[:, s, :, mlen:] = np.nan
        out.update(k_part=parts[0], v_part=parts[1], dk_mem=sums[0], dv_mem=sums[1])
    return out


@pytest.mark.parametrize("seg,mem", [(16, 112), (48, 64), (64, 0)], ids=["seg16_mem112", "seg48_mem64", "seg64_mem0"])
def test_the_two_folds_equal_the_numpy_sums(seg, mem):
    ops = _ops()
    B, n, D = 2, 2, 16
    c = _fold_case(seg, mem, B, n, D)
    assert np.isnan(c["rk_part"][:, :, :, seg + mem:]).all() and np.isnan(c["rk_part"][:, 0, :, seg:]).all()
    assert np.abs(c["drk"]).max() <= 8 * B * c["S"] < 2 ** 24
    rk_part = torch.from_numpy(c["rk_part"]).to(DEV)
    drk = torch.full((c["P"], n, D), float("nan"), device=DEV)
    ops.check(ops.lib().dn_txl_reduce_rk_f32(B, c["Lp"], n, D, seg, mem, c["P"], ops.ptr(rk_part), ops.ptr(drk), ops.stream_ptr()),
              "dn_txl_reduce_rk_f32")
    got = drk.cpu().numpy()
    assert np.isfinite(got).all() and np.array_equal(got, c["drk"]), "d rk differs at %d entries" % int((got != c["drk"]).sum())
    assert not got[seg + mem:].any() and got[:seg + mem].any()
    if mem == 0:
        return
    assert np.isnan(c["k_part"][:, 0]).all() and (seg >= mem or np.isnan(c["k_part"][:, 1, :, seg:]).all())
    assert not np.isnan(c["k_part"][:, -1]).any()
    k_part, v_part = (torch.from_numpy(c[k]).to(DEV) for k in ("k_part", "v_part"))
    dkm, dvm = (torch.full((B, c["Lp"], n, D), float("nan"), device=DEV) for _ in range(2))
    ops.check(ops.lib().dn_txl_fold_mem_f32(B, c["Lp"], n, D, seg, mem, ops.ptr(k_part), ops.ptr(v_part), ops.ptr(dkm), ops.ptr(dvm),
                                            ops.stream_ptr()), "dn_txl_fold_mem_f32")
    for got, want, name in ((dkm.cpu().numpy(), c["dk_mem"], "dk_mem"), (dvm.cpu().numpy(), c["dv_mem"], "dv_mem")):
        assert np.isfinite(got).all() and np.array_equal(got, want), "%s differs at %d entries" % (name, int((got != want).sum()))
        assert not got[:, -seg:].any() and got[:, 0].any()
