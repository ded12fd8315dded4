"""Bit-exact parity of the graph-classification kernels -- dn_segment.hip, dn_graphsum.hip, dn_gemm.hip: the path of configs 1, 2 and 4
and of bench.py's GIN leg -- on operands where the arithmetic is exact (tests/gc_exact_ref.py): integer rows, power-of-two scales,
self_coef 1.25, signed 0 / +-1 weights.  Whatever form, chunking, lane split or summation order a kernel uses, its result must then equal
the float64 index_add / matmul reference rounded once to the path's dtype, with atol = rtol = 0 -- a dropped list entry, a chunk one
short, a gradient entry routed to the wrong tied row or a lost bf16 plane changes bits here where the tolerance tests of the same
kernels (random normal operands, 1e-5 .. 2e-2) can let it pass.  The one exception is a mean over a list whose length is no power of two:
at most 1 ulp from the correctly rounded quotient (the kernels multiply by a rounded reciprocal).  Every case holds its premise first
(gc_exact_ref.check_premise; proven without a GPU by tests/test_gc_exact_premise.py): a premise failure is a failure, never a skip.
NaN semantics of the max kernels are out of scope: no operand here holds a NaN (-inf is covered)."""
from contextlib import contextmanager

import numpy as np
import pytest
import torch

import exact_ref as X
import gc_exact_ref as G

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [G.F32, G.BF16]
IDS = ["f32", "bf16"]


def _ops():
    from dummynode4graphlearning_amd import ops
    return ops


@contextmanager
def switches(**kw):
    """Set ops module switches (read at call time) and restore them whatever happens (as tests/test_gpu_exact.py does)."""
    ops = _ops()
    old = {k: getattr(ops, k) for k in kw}
    try:
        for k, v in kw.items():
            setattr(ops, k, v)
        yield
    finally:
        for k, v in old.items():
            setattr(ops, k, v)


def _d(t, dtype=None):
    """float64 / int64 CPU operand -> device tensor in the path's dtype (exact there) / int32"""
    if t is None:
        return None
    if isinstance(t, np.ndarray):
        t = torch.from_numpy(t)
    if t.is_floating_point():
        return t.to(DEV, dtype if dtype is not None else torch.float32)
    return t.to(DEV, torch.int32)


# ---- (a) gather_segsum -----------------------------------------------------------------------------------------------------------
def _gather_params():
    out = []
    for dtype, name in zip(DTYPES, IDS):
        for H in G.VEC_H[dtype] + G.SCALAR_H[dtype]:
            out.append(pytest.param(dtype, H, None, id="%s-H%d" % (name, H)))
        for H in G.ALIGN_H:
            for which in ("x", "out", "self_in"):
                out.append(pytest.param(dtype, H, which, id="%s-H%d-unaligned-%s" % (name, H, which)))
    return out


@pytest.mark.parametrize("dtype,H,misalign", _gather_params())
def test_gather_segsum_every_form_is_bit_exact(dtype, H, misalign):
    """dn_gather_segsum_*: the form is chosen inside C from H, the pointers' alignment, M / S and S (gc_exact_ref.lpr_class, list_lengths):
      H -> LPR: fp32 4, 16 -> 4 | 20 -> 8 | 64 -> 16 | 128 -> 32 | 256 -> 64 | 260, 512 -> 64 in two column passes (the block form's
                second pass waits at its barrier); bf16 8, 32 -> 4 | 64 -> 8 | 128 -> 16 | 256 -> 32 | 512 -> 64 | 520 -> 64, two passes;
      scalar form by shape: fp32 H = 1, 3 (LPR 8), 9 (LPR 64), bf16 H = 70; by alignment: H = 64 / 128 with x, out= or self_in starting
                4 bytes (fp32) / 2 bytes (bf16) into a larger allocation (misalign);
      S in {1, 2, c-1, c, c+1, 7c+1, 8c, 8c+1}, c = 2 * 256 / LPR segments per chunk (grid rounded up to 8 chunks, tail via dn_xcd_chunk);
      M / S < 16 pipelined vec kernel | 16 <= M / S < 24 vec1 kernel | M / S >= 24 and S <= 8192 workgroup per segment (vector forms only);
      list lengths from {0, 1, 7, 8, 9, LPR-1, LPR, LPR+1, 2 LPR, 2 LPR+1}: KU = 8 loads in flight, the re-fetch branch past LPR entries."""
    ops = _ops()
    n = 0
    for c in G.gather_cases(0, dtype, H, aligned=misalign is None):
        if misalign == "self_in" and c.self_in is None:
            continue
        c.premise()
        x, self_in = _d(c.x, dtype), _d(c.self_in, dtype)
        out = None
        if misalign == "x":
            x = G.unaligned(x)
        elif misalign == "self_in":
            self_in = G.unaligned(self_in)
        elif misalign == "out":
            out = G.unaligned(torch.full((c.S, H), 7.0, dtype=dtype, device=DEV))
        got = ops.gather_segsum(x, _d(c.idx), _d(c.ptr), scale=_d(c.scale), self_in=self_in, self_coef=c.self_coef, mean=c.mean, out=out)
        c.compare(got)
        n += 1
    assert n >= 8 * 3 * (2 if misalign == "self_in" else 7)


# ---- (b) hub splitting -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scaled", [False, True], ids=["unscaled", "scaled"])
@pytest.mark.parametrize("dtype,H", [(G.F32, 20), (G.F32, 128), (G.BF16, 24), (G.BF16, 128)], ids=["f32-H20", "f32-H128", "bf16-H24", "bf16-H128"])
def test_neighbor_sum_and_edge_sum_over_split_hubs_are_bit_exact(dtype, H, scaled):
    """_SplitCSR (HUB_SPLIT = 64): in- and out-degrees of exactly 63, 64 (not split), 65 (chunks of 64 + 1), 128 (two full chunks), 129 and
    600 (fp32 only: a bf16 list stays within 256 entries); with and without a power-of-two edge_scale; output and input gradient."""
    ops = _ops()
    c = G.hub_case(0, dtype, H, scaled)
    c["neighbor"].premise(dtype)
    c["edge"].premise(dtype)
    index = ops.EdgeIndex(_d(c["src"]), _d(c["dst"]), c["N"])
    nh = len(G.HUB_DEGREES[dtype])
    split = sorted(int(v) for v in index.fwd.hub_ids.tolist())
    assert split == [k for k, d in enumerate(G.HUB_DEGREES[dtype]) if d > ops.HUB_SPLIT] == sorted(int(v) for v in index.bwd.hub_ids.tolist())
    assert nh - len(split) == 2                                       # 63 and 64 stay in the main pass
    w = _d(c["w"])
    x = _d(c["x"], dtype).requires_grad_(True)
    out = ops.neighbor_sum(x, index, G.SELF_COEF, edge_scale=w)
    out.backward(_d(c["g"], dtype))
    X.assert_bits(out, c["neighbor"].out, c["neighbor"].what + " output")
    X.assert_bits(x.grad, c["neighbor"].gin, c["neighbor"].what + " input gradient")
    ef = _d(c["ef"], dtype).requires_grad_(True)
    out = ops.edge_sum(ef, index, edge_scale=w)
    out.backward(_d(c["g"], dtype))
    X.assert_bits(out, c["edge"].out, c["edge"].what + " output")
    X.assert_bits(ef.grad, c["edge"].gin, c["edge"].what + " input gradient")


# ---- (c) the tile path -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("self_coef", [1.0, 1.25])
@pytest.mark.parametrize("H", [64, 128, 256])
def test_tile_path_of_neighbor_sum_is_bit_exact(H, self_coef):
    """dn_graph_tile_sum_f32 + dn_gather_rows_sum_f32 through ops.neighbor_sum (TILE_SUM_MIN_ROWS lowered): graphs of 0, 1, 63, 64, 65 and
    200 rows packed into tiles of exactly 64 rows, empty graphs first / in the middle / last, the last tile ending at N; row lists of
    exactly 64 (lane group per row), 65 and 199 entries (workgroup per row); self loops; 255 and 256 parallel edges on one pair (the
    largest counts the bf16 adjacency holds: flag clear); wide values of up to 24 significant bits in all three bf16 planes.  self_coef
    1.0 is GIN's (1 + eps) at eps = 0, 1.25 the operand rule of the other cases (wide values then hold at most 21 bits)."""
    ops = _ops()
    c = G.tile_case(0, H, self_coef)
    c["case"].premise(G.F32)
    with switches(TILE_SUM_MIN_ROWS=1, TILE_SUM_ENABLED=True):
        index = ops.EdgeIndex(_d(c["src"]), _d(c["dst"]), c["N"], node_ptr=_d(c["nptr"]))
        plan = index.tile_plan()
        assert plan is not None and plan.covered == 6 * 64
        for rec, short, long_, _, _ in plan.dirs.values():
            assert rec.shape[0] == 6 and short.shape[0] > 0 and long_.shape[0] > 0
            deg_s, deg_l = (short[:, 2] - short[:, 1]).tolist(), (long_[:, 2] - long_[:, 1]).tolist()
            assert max(deg_s) == 64 and 65 in deg_l and 199 in deg_l
        x = _d(c["x"]).requires_grad_(True)
        out = ops.neighbor_sum(x, index, self_coef)
        assert plan.checked and int(plan.bad.item()) == 0 and index.tile_plan() is plan
        out.backward(_d(c["g"]))
        assert int(plan.bad.item()) == 0
    graph_of = np.repeat(np.arange(len(c["nptr"]) - 1), np.diff(c["nptr"]))
    X.assert_bits(out, c["case"].out, c["case"].what + " output", graph=graph_of)
    X.assert_bits(x.grad, c["case"].gin, c["case"].what + " input gradient", graph=graph_of)


@pytest.mark.parametrize("flaw", ["parallel257", "cross"])
@pytest.mark.parametrize("H", [64, 128, 256])
def test_flagged_tile_batch_falls_back_to_the_plain_gather_at_once(H, flaw):
    """257 parallel edges on one pair (the bf16 adjacency count would round) / an edge between two graphs (not a run of whole graphs):
    in-bounds inputs the tile kernel refuses by raising its flag.  The FIRST neighbor_sum call and its backward must already return the
    plain kernel's sums, the plan is gone afterwards, and a second call is exact again."""
    ops = _ops()
    c = G.tile_case(0, H, G.SELF_COEF, flaw)
    c["case"].premise(G.F32)
    with switches(TILE_SUM_MIN_ROWS=1, TILE_SUM_ENABLED=True):
        index = ops.EdgeIndex(_d(c["src"]), _d(c["dst"]), c["N"], node_ptr=_d(c["nptr"]))
        plan = index.tile_plan()
        assert plan is not None and not plan.checked
        for call in ("first", "second"):
            x = _d(c["x"]).requires_grad_(True)
            out = ops.neighbor_sum(x, index, G.SELF_COEF)
            out.backward(_d(c["g"]))
            X.assert_bits(out, c["case"].out, "%s %s call: output" % (c["case"].what, call))
            X.assert_bits(x.grad, c["case"].gin, "%s %s call: input gradient" % (c["case"].what, call))
            assert index.tile_plan() is None
        assert int(plan.bad.item()) != 0


# ---- (d) readouts and max routing ------------------------------------------------------------------------------------------------
def _readout_params():
    out = []
    for dtype, name in zip(DTYPES, IDS):
        for H in G.READOUT_H:
            out.append(pytest.param(dtype, H, False, id="%s-H%d" % (name, H)))
            if dtype == G.F32 and H in (64, 128, 256):
                out.append(pytest.param(dtype, H, True, id="%s-H%d-unaligned" % (name, H)))
    return out


@pytest.mark.parametrize("dtype,H,misalign", _readout_params())
def test_segment_readouts_are_bit_exact_and_route_ties_to_the_first_row(dtype, H, misalign):
    """segment_reduce sum / mean / max over integer rows with many ties: a whole tied segment, an all-negative one, one holding only -inf
    (max), empty ones, segments of 64 / 65 / 130 rows.  Max gradient: the lowest row among the tied maxima receives the whole upstream
    entry (stated from the inputs by gc_exact_ref.segment_max_ref).  misalign: x (and the upstream gradient) behind a view that is
    not 16-byte aligned -- the scalar family instead of the vector one.  NaNs are out of scope."""
    ops = _ops()
    rng = np.random.default_rng(H)
    view = G.unaligned if misalign else (lambda t: t)
    for kind in ("sum", "mean", "max"):
        x, ptr = G.readout_rows(rng, H, with_inf=kind == "max")
        S = len(ptr) - 1
        lens = torch.from_numpy(np.diff(ptr))
        seg = torch.repeat_interleave(torch.arange(S), lens)
        g = X.tri_coef(rng, S, H)
        xd = view(_d(x, dtype)).requires_grad_(True)
        out = ops.segment_reduce(xd, _d(ptr), kind)
        out.backward(view(_d(g, dtype)))
        what = "segment_%s %s H=%d" % (kind, str(dtype)[6:], H)
        if kind == "max":
            ref, gin = G.segment_max_ref(x, ptr, g)
            G.check_premise(ref, ref.abs(), dtype, [x], what)
            X.assert_bits(out, ref, what + " output")
            X.assert_bits(xd.grad, gin, what + " gradient", graph=seg)
            continue
        z = torch.zeros(S, H, dtype=torch.float64)
        total = z.index_add(0, seg, x)
        G.check_premise(total, z.index_add(0, seg, x.abs()), dtype, [x], what)
        if kind == "sum":
            X.assert_bits(out, total, what + " output")
            X.assert_bits(xd.grad, g[seg], what + " gradient", graph=seg)
        else:
            G.assert_mean(out, total, lens, what + " output")
            G.assert_mean(xd.grad, g[seg], lens[seg], what + " gradient")


@pytest.mark.parametrize("dtype,H,misalign", _readout_params())
def test_neighbor_max_is_bit_exact_and_routes_ties_to_the_first_edge(dtype, H, misalign):
    """neighbor_max with multi-edges (one source row gathered twice), isolated nodes, a whole tied list, an all-negative list, a list of
    -inf rows only.  Gradient: among the tied maxima of (destination, column) the edge with the lowest original edge index into that
    destination receives the whole upstream entry (gc_exact_ref.neighbor_max_ref states it from the inputs, not from the kernel's
    argmax).  misalign (fp32 v4 widths): x and the upstream gradient unaligned -- the lane-strided kernels instead of the v4 ones."""
    ops = _ops()
    rng = np.random.default_rng(H + 1)
    view = G.unaligned if misalign else (lambda t: t)
    src, dst, N = G.max_graph(rng)
    x, g = G.max_rows(rng, N, H), X.tri_coef(rng, N, H)
    ref, gin = G.neighbor_max_ref(x, src, dst, N, g)
    what = "neighbor_max %s H=%d" % (str(dtype)[6:], H)
    G.check_premise(ref, ref.abs(), dtype, [x], what)
    gb = torch.zeros_like(x).index_add(0, torch.from_numpy(src), g.abs()[torch.from_numpy(dst)])
    G.check_premise(gin, gb, dtype, [g], what + " gradient")
    assert int((ref[:, 0] == 0).sum()) >= 2 and bool(torch.isinf(ref[4]).all())
    index = ops.EdgeIndex(_d(src), _d(dst), N)
    xd = view(_d(x, dtype)).requires_grad_(True)
    out = ops.neighbor_max(xd, index)
    out.backward(view(_d(g, dtype)))
    X.assert_bits(out, ref, what + " output")
    X.assert_bits(xd.grad, gin, what + " gradient")


# ---- (e) edge_dot ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("H", G.EDGE_DOT_H)
def test_edge_dot_is_bit_exact(H, dtype):
    """dn_edge_dot_*: E in {1, 15, 16, 17, 1000} (a workgroup holds 16 / 4 lane groups), ia / ib given and None; at the fp32 v4 widths
    (64, 128, 256) also with a or b unaligned: the lane-strided kernel instead of the v4 one."""
    ops = _ops()
    for E in G.EDGE_DOT_E:
        for use_ia, use_ib in ((True, True), (False, True), (True, False), (False, False)):
            a, ia, b, ib, ref, bound, terms = G.edge_dot_case(np.random.default_rng([H, E]), dtype, H, E, use_ia, use_ib)
            what = "edge_dot %s H=%d E=%d ia=%s ib=%s" % (str(dtype)[6:], H, E, use_ia, use_ib)
            G.check_premise(ref, bound, G.F32, terms, what)
            ad, bd = _d(a, dtype), _d(b, dtype)
            X.assert_bits(ops.edge_dot(ad, _d(ia), bd, _d(ib)), ref, what)
            if dtype == G.F32 and H in (64, 128, 256):
                X.assert_bits(ops.edge_dot(G.unaligned(ad), _d(ia), bd, _d(ib)), ref, what + " a unaligned")
                X.assert_bits(ops.edge_dot(ad, _d(ia), G.unaligned(bd), _d(ib)), ref, what + " b unaligned")


# ---- (f) the any-width products --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("K,N", G.GEMM_KN)
def test_any_width_products_are_bit_exact(K, N, dtype):
    """dn_rows_gemm_* (plain with bias, transpose_w) and dn_rows_wgrad_any_* (+ column sums) over relations of 0, 1, 63, 64, 65, 511, 512,
    513 and 1025 rows: 64-row tiles and split-K chunks that end on, one before and one past a relation's end."""
    ops = _ops()
    c = G.GemmCase(0, K, N)
    c.premise(dtype)
    rp = torch.tensor(c.rel_ptr, dtype=torch.int32, device=DEV)
    tiles = ops.build_row_tables(rp, c.R, c.P, 64)
    A, Gd, W, bias = _d(c.A, dtype), _d(c.G, dtype), _d(c.W, dtype), _d(c.bias, dtype)
    rel = np.repeat(np.arange(c.R), c.sizes)
    what = "%s K=%d N=%d " % (str(dtype)[6:], K, N)
    X.assert_bits(ops.rows_gemm(A, W, tiles, bias=bias), c.Y, what + "rows_gemm", rel=rel)
    X.assert_bits(ops.rows_gemm(Gd, W, tiles, transpose_w=True), c.Yt, what + "rows_gemm transpose_w", rel=rel)
    for step in (64, 512):
        chunks = ops.build_row_tables(rp, c.R, c.P, step, want_ptr=True)
        gW, cs = ops.rows_wgrad_any(A, Gd, chunks, c.R, want_colsum=True)
        X.assert_bits(gW, c.gW, what + "rows_wgrad_any, chunks of %d" % step)
        X.assert_bits(cs, c.colsum, what + "rows_wgrad_any column sums, chunks of %d" % step)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("K,N", G.GEMM_KN)
def test_linear_any_is_bit_exact(K, N, dtype):
    """linear_any forward and all three gradients at every row count of the relation-size list ((64, 64) takes the matrix-core path)."""
    ops = _ops()
    for P in [s for s in G.REL_SIZES if s]:
        c = G.LinearCase(0, P, K, N)
        c.premise(dtype)
        x, w, b = (_d(t, dtype).requires_grad_(True) for t in (c.x, c.w, c.b))
        y = ops.linear_any(x, w, b)
        y.backward(_d(c.g, dtype))
        what = "linear_any %s P=%d K=%d N=%d " % (str(dtype)[6:], P, K, N)
        for name, got in (("y", y), ("gx", x.grad), ("gw", w.grad), ("gb", b.grad)):
            X.assert_bits(got, c.refs[name], what + name)


# ---- raw launches refuse what they cannot read -----------------------------------------------------------------------------------
def test_raw_launches_refuse_non_contiguous_tensors():
    """ops.gather_segsum / ops.edge_dot pass data_ptr() with shape[1] as the row stride: a strided view must be refused, not read as
    garbage (the autograd wrappers call .contiguous() and never get here).  _lib.require_gpu is what refuses it (DnHipError), for every
    tensor argument of both launches; edge_dot also refuses operands of different widths or dtypes."""
    ops = _ops()
    from dummynode4graphlearning_amd._lib import DnHipError
    rng = np.random.default_rng(0)
    H, n = 16, 40
    wide = _d(G.int_rows(rng, n, 2 * H, G.F32))
    idx2 = _d(torch.from_numpy(rng.integers(0, n, size=60)))
    ptr = _d(torch.arange(0, 31))
    sc2 = _d(G.scales(rng, 60))
    for kw in (dict(x=wide[:, :H], idx=idx2[:30].contiguous(), ptr_=ptr),
               dict(x=wide[:, :H].contiguous(), idx=idx2[::2], ptr_=ptr),
               dict(x=wide[:, :H].contiguous(), idx=idx2[:30].contiguous(), ptr_=ptr, scale=sc2[::2]),
               dict(x=wide[:, :H].contiguous(), idx=idx2[:30].contiguous(), ptr_=ptr, self_in=wide[:30, H:], self_coef=1.0)):
        with pytest.raises((DnHipError, AssertionError), match="contiguous"):
            ops.gather_segsum(**kw)
    a, b = wide[:, :H].contiguous(), wide[:, H:].contiguous()
    ia = idx2[:30].contiguous()
    for args in ((wide[:, :H], ia, b, ia), (a, ia, wide[:, H:], ia), (a, idx2[::2], b, ia), (a, ia, b, idx2[::2])):
        with pytest.raises((DnHipError, AssertionError), match="contiguous"):
            ops.edge_dot(*args)
    with pytest.raises(AssertionError):
        ops.edge_dot(a, ia, wide, ia)                               # 16 columns against 32: rows of b would be read at the wrong stride
    # ... and the contiguous forms of the same operands are exact
    got = ops.gather_segsum(a, ia, ptr)
    X.assert_bits(got, wide[:, :H].double().cpu()[ia.long().cpu()], "gather of the contiguous copy")
    X.assert_bits(ops.edge_dot(a, ia, b, ia), (a.double() * b.double()).sum(1)[ia.long()], "edge_dot of the contiguous copies")
