"""CPU self-tests of tests/gc_exact_ref.py (no GPU): every operand set of tests/test_gpu_gc_exact.py is built here and held to its
premise -- the float64 reference representable in the output dtype, sum |terms| / quantum < 2^24 for every output element -- and the
helpers' references (segment sums, the tie rule of the max kernels, the 1-ulp rule of the means) are checked against naive Python loops.
A premise failure is a failure of these tests; the GPU tests then compare bits on operands proven exact."""
import numpy as np
import pytest
import torch

import exact_ref as X
import gc_exact_ref as G

DTYPES = [G.F32, G.BF16]
IDS = ["f32", "bf16"]


def _gather_classes(dtype):
    return [(H, True) for H in G.VEC_H[dtype] + G.SCALAR_H[dtype]] + [(H, False) for H in G.ALIGN_H]


def _gather_params():
    return [pytest.param(dt, H, al, id="%s-H%d%s" % (name, H, "" if al else "-unaligned"))
            for dt, name in zip(DTYPES, IDS) for H, al in _gather_classes(dt)]


def _form(c):
    a = c.M // c.S
    return "pipelined" if a < 16 else ("vec1" if a < 24 else "block")


@pytest.mark.parametrize("dtype,H,aligned", _gather_params())
def test_gather_operands_hold_the_premise_and_reach_every_form(dtype, H, aligned):
    """Every gather_segsum case of one (dtype, H, alignment) class: the premise, and the three average-length forms reached at every S."""
    seen = set()
    for c in G.gather_cases(0, dtype, H, aligned):
        c.premise()
        if c.ptr is not None and c.idx is not None:
            seen.add((c.S, _form(c)))
        if dtype == G.BF16:
            assert c.lens.numel() == 0 or int(c.lens.max()) <= 257
    lpr, _ = G.lpr_class(H, dtype, aligned)
    assert seen == {(S, f) for S in G.seg_counts(lpr) for f in G.FORMS}


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_gather_shapes_reach_every_instantiation(dtype):
    """The H classes cover every launch_lpr instantiation: vector LPR 4 .. 64, the scalar form at LPR 64 (by shape and by alignment) and,
    in fp32, at LPR 8."""
    classes = {G.lpr_class(H, dtype, al) for H, al in _gather_classes(dtype)}
    assert {(lpr, True) for lpr in (4, 8, 16, 32, 64)} <= classes and (64, False) in classes
    assert dtype != G.F32 or (8, False) in classes


def test_the_dispatch_classes_are_the_ones_the_shapes_name():
    assert [G.lpr_class(H, G.F32) for H in G.VEC_H[G.F32]] == [(4, True), (4, True), (8, True), (16, True), (32, True), (64, True),
                                                                 (64, True), (64, True)]
    assert [G.lpr_class(H, G.BF16) for H in G.VEC_H[G.BF16]] == [(4, True), (4, True), (8, True), (16, True), (32, True), (64, True),
                                                                   (64, True)]
    assert [G.lpr_class(H, G.F32) for H in (1, 3, 9)] == [(8, False), (8, False), (64, False)] and G.lpr_class(70, G.BF16) == (64, False)
    assert G.lpr_class(64, G.F32, aligned=False) == (64, False) and G.lpr_class(128, G.BF16, aligned=False) == (64, False)
    assert G.seg_counts(64) == [1, 2, 7, 8, 9, 57, 64, 65] and G.seg_counts(4) == [1, 2, 127, 128, 129, 897, 1024, 1025]
    rng = np.random.default_rng(0)
    for lpr in (4, 8, 16, 32, 64):
        wanted = {0, 1, 7, 8, 9, lpr - 1, lpr, lpr + 1, 2 * lpr, 2 * lpr + 1}
        lens = G.list_lengths(rng, 8 * (512 // lpr) + 1, lpr, "pipelined")
        assert wanted <= set(int(v) for v in lens)                  # every length of the issue's set occurs


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_gather_reference_equals_a_naive_loop(dtype):
    H = 8
    lpr, _ = G.lpr_class(H, dtype)
    for combo in G.combos_of(dtype):
        c = G.GatherCase(1, dtype, H, lpr, 9, "vec1", combo)
        ptr = c.ptr.tolist() if c.ptr is not None else list(range(c.M + 1))
        want = torch.zeros(c.S, H, dtype=torch.float64)
        for s in range(c.S):
            acc = [0.0] * H
            for i in range(ptr[s], ptr[s + 1]):
                r = int(c.idx[i]) if c.idx is not None else i
                w = float(c.scale[i]) if c.scale is not None else 1.0
                for h in range(H):
                    acc[h] += w * float(c.x[r, h])
            n = ptr[s + 1] - ptr[s]
            for h in range(H):
                v = acc[h]
                if c.mean and c.self_in is not None:
                    v = v / max(n, 1)
                if c.self_in is not None:
                    v += 1.25 * float(c.self_in[s, h])
                want[s, h] = v
        assert torch.equal(want, c.ref), combo


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_the_mean_rule_accepts_a_rounded_reciprocal_and_nothing_more(dtype):
    rng = np.random.default_rng(2)
    lens = torch.tensor([0, 1, 3, 7, 8, 9, 15, 16, 17, 63, 64, 65, 129])
    total = torch.from_numpy(rng.integers(-40, 41, size=(len(lens), 64)).astype(np.float64))
    total[0] = 0.0
    inv = torch.where(lens > 0, 1.0 / lens.clamp(min=1).float(), torch.zeros(len(lens)))     # the kernels: fp32 sum x fp32 reciprocal
    kernel = (total.float() * inv.view(-1, 1)).to(dtype)
    G.assert_mean(kernel, total, lens, "restated kernel mean")
    exact = G.is_pow2(lens) | (lens == 0)
    assert torch.equal(kernel[exact].double(), (total / lens.clamp(min=1).view(-1, 1))[exact].to(dtype).double())
    dropped = total.clone()
    dropped[5, 3] -= 1.0                                                                     # one small-integer row lost from a list of 9
    with pytest.raises(AssertionError):
        G.assert_mean((dropped.float() * inv.view(-1, 1)).to(dtype), total, lens, "a dropped row")
    two = G.mean_want(total, lens, dtype).clone()
    nz = (two[6] != 0).nonzero()[0]
    bits = two.view(torch.int16 if dtype == G.BF16 else torch.int32)
    bits[6, int(nz)] += 2                                                                    # 2 ulp off on a list of 15
    with pytest.raises(AssertionError):
        G.assert_mean(two, total, lens, "two ulp")
    bits[6, int(nz)] -= 1                                                                    # 1 ulp: accepted there ...
    G.assert_mean(two, total, lens, "one ulp")
    bits[4, 0] += 1                                                                          # ... but not on a list of 8
    with pytest.raises(AssertionError):
        G.assert_mean(two, total, lens, "one ulp on a power of two")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_hub_cases_hold_the_premise(dtype):
    for H in (20 if dtype == G.F32 else 24, 128):
        for scaled in (False, True):
            c = G.hub_case(0, dtype, H, scaled)
            c["neighbor"].premise(dtype)
            c["edge"].premise(dtype)
            ind, outd = np.bincount(c["dst"], minlength=c["N"]), np.bincount(c["src"], minlength=c["N"])
            for k, d in enumerate(G.HUB_DEGREES[dtype]):
                assert ind[k] == d and outd[k] == d
    assert G.HUB_DEGREES[G.F32] == (63, 64, 65, 128, 129, 600) and G.HUB_DEGREES[G.BF16] == (63, 64, 65, 128, 129)


def test_neighbor_reference_equals_a_naive_loop():
    rng = np.random.default_rng(3)
    N, E, H = 12, 60, 3
    src, dst = rng.integers(0, N, size=E), rng.integers(0, N, size=E)
    x, g, w = G.int_rows(rng, N, H, G.F32), X.tri_coef(rng, N, H), torch.from_numpy(rng.choice([0.5, 1.0, 2.0], size=E))
    c = G.NeighborCase(x, src, dst, N, g, 1.25, w)
    out, gin = 1.25 * x.clone(), 1.25 * g.clone()
    for e in range(E):
        out[dst[e]] += w[e] * x[src[e]]
        gin[src[e]] += w[e] * g[dst[e]]
    assert torch.equal(out, c.out) and torch.equal(gin, c.gin)
    ef = G.int_rows(rng, E, H, G.F32)
    c = G.NeighborCase(ef, src, dst, N, g, 0.0, w, edge_rows=True)
    out = torch.zeros(N, H, dtype=torch.float64)
    for e in range(E):
        out[dst[e]] += w[e] * ef[e]
    assert torch.equal(out, c.out) and torch.equal(c.gin, w.view(-1, 1) * g[torch.from_numpy(dst)])


@pytest.mark.parametrize("H", [64, 128, 256])
def test_tile_cases_hold_the_premise_and_have_the_shapes_they_name(H):
    for self_coef in (1.0, 1.25):
        c = G.tile_case(0, H, self_coef)
        c["case"].premise(G.F32)
        top = 24 if self_coef == 1.0 else 21
        assert 17 <= X.sig_bits(c["x"]) <= top and X.sig_bits(c["x"]) >= top - 1     # wide values: all three bf16 planes carry bits
    src, dst, nptr, N = c["src"], c["dst"], c["nptr"], c["N"]
    assert sorted(set(np.diff(nptr))) == [0, 1, 63, 64, 65, 200] and nptr[1] == 0 and nptr[-2] == N
    tiles = G.greedy_tiles(nptr)
    assert all(b - a == 64 for a, b in tiles) and tiles[-1][1] == N and len(tiles) == 6
    big = np.repeat(np.diff(nptr) > 64, np.diff(nptr))
    ind, outd = np.bincount(dst, minlength=N), np.bincount(src, minlength=N)
    for deg in (ind, outd):
        assert {64, 65, 199} <= set(deg[big])                       # lane-group list of 64, workgroup lists of 65 and 199
    assert (src == dst).any()
    _, cnt = np.unique(src * N + dst, return_counts=True)
    assert {255, 256} <= set(cnt) and cnt.max() == 256
    graph_of = np.repeat(np.arange(len(nptr) - 1), np.diff(nptr))
    assert (graph_of[src] == graph_of[dst]).all()


@pytest.mark.parametrize("flaw", ["parallel257", "cross"])
def test_flagged_tile_batches_are_in_bounds_and_exact(flaw):
    c = G.tile_case(0, 64, 1.25, flaw)
    c["case"].premise(G.F32)
    src, dst, nptr, N = c["src"], c["dst"], c["nptr"], c["N"]
    assert src.min() >= 0 and dst.min() >= 0 and src.max() < N and dst.max() < N
    _, cnt = np.unique(src * N + dst, return_counts=True)
    graph_of = np.repeat(np.arange(len(nptr) - 1), np.diff(nptr))
    if flaw == "parallel257":
        assert cnt.max() == 257 and (graph_of[src] == graph_of[dst]).all()
    else:
        assert cnt.max() <= 256 and int((graph_of[src] != graph_of[dst]).sum()) == 1


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_readout_and_max_references_state_the_tie_rule(dtype):
    rng = np.random.default_rng(4)
    for H in (2, 7):
        x, ptr = G.readout_rows(rng, H, with_inf=True)
        S = len(ptr) - 1
        g = X.tri_coef(rng, S, H)
        out, gin = G.segment_max_ref(x, ptr, g)
        for s in range(S):
            for h in range(H):
                best, arg = 0.0, -1
                for i in range(int(ptr[s]), int(ptr[s + 1])):
                    if arg < 0 or float(x[i, h]) > best:
                        best, arg = float(x[i, h]), i
                assert float(out[s, h]) == best
                for i in range(int(ptr[s]), int(ptr[s + 1])):
                    assert float(gin[i, h]) == (float(g[s, h]) if i == arg else 0.0)
        ties = sum(int((x[ptr[s]:ptr[s + 1]] == out[s]).sum(0).gt(1).sum()) for s in range(S) if ptr[s + 1] > ptr[s])
        assert ties > H and bool(torch.isinf(out[10]).all()) and float(out[6].max()) < 0 and float(out[1].abs().max()) == 0
        src, dst, N = G.max_graph(rng, N=40, E=150)
        xm, gm = G.max_rows(rng, N, H), X.tri_coef(rng, N, H)
        out, gin = G.neighbor_max_ref(xm, src, dst, N, gm)
        want_gin = torch.zeros_like(xm)
        for v in range(N):
            for h in range(H):
                best, arg = 0.0, -1
                for e in range(len(src)):                            # original edge order
                    if dst[e] == v and (arg < 0 or float(xm[src[e], h]) > best):
                        best, arg = float(xm[src[e], h]), e
                assert float(out[v, h]) == best
                if arg >= 0:
                    want_gin[src[arg], h] += gm[v, h]
        assert torch.equal(gin, want_gin)
        assert float(out[0].abs().max()) == 0 and bool(torch.isinf(out[4]).all()) and float(out[3].max()) < 0
        key = src * N + dst
        assert len(np.unique(key)) < len(key)                        # multi-edges: one source row gathered twice
        G.check_premise(out, out.abs(), dtype, [xm], "neighbor_max output")
        G.check_premise(gin, torch.zeros_like(xm).index_add(0, torch.from_numpy(src), gm.abs()[torch.from_numpy(dst)]), dtype, [gm],
                        "neighbor_max gradient")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_readout_sums_hold_the_premise(dtype):
    for H in G.READOUT_H:
        x, ptr = G.readout_rows(np.random.default_rng(H), H, with_inf=False)
        S = len(ptr) - 1
        seg = torch.repeat_interleave(torch.arange(S), torch.from_numpy(np.diff(ptr)))
        z = torch.zeros(S, H, dtype=torch.float64)
        G.check_premise(z.index_add(0, seg, x), z.index_add(0, seg, x.abs()), dtype, [x], "segment sum H=%d" % H)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_edge_dot_operands_hold_the_premise(dtype):
    for H in G.EDGE_DOT_H:
        for E in G.EDGE_DOT_E:
            for use_ia, use_ib in ((True, True), (False, True), (True, False), (False, False)):
                a, ia, b, ib, ref, bound, terms = G.edge_dot_case(np.random.default_rng([H, E]), dtype, H, E, use_ia, use_ib)
                G.check_premise(ref, bound, G.F32, terms, "edge_dot H=%d E=%d" % (H, E))
                if E <= 17 and H <= 17:
                    for e in range(E):
                        want = sum(float(a[int(ia[e]) if use_ia else e, h]) * float(b[int(ib[e]) if use_ib else e, h]) for h in range(H))
                        assert float(ref[e]) == want


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("K,N", G.GEMM_KN)
def test_any_width_operands_hold_the_premise(K, N, dtype):
    c = G.GemmCase(0, K, N)
    c.premise(dtype)
    assert c.sizes == [0, 1, 63, 64, 65, 511, 512, 513, 1025]
    r = 4                                                            # the reference against a naive loop on one relation (65 rows)
    a, b = c.rel_ptr[r], c.rel_ptr[r + 1]
    for p in range(a, min(b, a + 5)):
        for n in range(min(N, 9)):
            assert float(c.Y[p, n]) == sum(float(c.A[p, k]) * float(c.W[r, k, n]) for k in range(K)) + float(c.bias[r, n])
        for k in range(min(K, 9)):
            assert float(c.Yt[p, k]) == sum(float(c.G[p, n]) * float(c.W[r, k, n]) for n in range(N))
    for P in [s for s in c.sizes if s]:
        G.LinearCase(0, P, K, N).premise(dtype)
