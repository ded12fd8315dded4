"""HGP-SL on the GPU (dn_hgpsl.hip): the score bit for bit on inputs whose every coefficient is a power of two, the per-graph top-k
against a stable CPU sort, the structure learning forward and backward against the float64 restatement of hgpsl_ref.py on a batch in
which both kernel classes and the composed fallback meet, the layer and the two-level stack against the reference's goldens under
both paths, and the peak memory of a layer.

Bounds (the project's, tests/test_gpu_gc_models.py / test_gpu_diffpool.py): outputs within 1e-4 (max|a - b| / max|b|), gradients within
5e-4 of their range, a gradient expected below 1e-5 stays below 1e-5."""
import numpy as np
import pytest
import torch

import hgpsl_cases as C
import hgpsl_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _ops():
    from dummynode4graphlearning_amd import ops
    return ops


# ---------------------------------------------------------------------------------------------- the score, bit for bit
def _exact_graphs():
    """(sizes, edges, weights): out-degrees (weighted) all 0, 1, 4 or 16, so every dinv is 0, 1, 1/2 or 1/4 and every coefficient a
    power of two."""
    sizes, edges, w = [], [], []
    base = 0

    def add(n, es, ws=None):
        nonlocal base
        sizes.append(n)
        for i, (a, b) in enumerate(es):
            edges.append((base + a, base + b))
            w.append(1.0 if ws is None else ws[i])
        base += n

    for n in (0, 1, 2, 64, 65):                                             # directed cycles (n = 1: a self loop), degree 1
        add(n, [(i, (i + 1) % n) for i in range(n)])
    add(64, [(i, (i + d) % 64) for i in range(64) for d in (1, 2, 3, 4)])  # 4-regular circulants, degree 4
    add(65, [(i, (i + d) % 65) for i in range(65) for d in (1, 5, 7, 11)])
    add(5, [])                                                              # isolated nodes
    add(17, [(v, 0) for v in range(1, 17)] + [(0, v) for v in range(1, 17)])   # a star: leaves -> hub, and the hub's 16 out-edges
    add(9, [(i, (i + 1) % 9) for i in range(9)], [4.0] * 9)                 # weighted cycles: degree 4 and 16 from one edge
    add(6, [(i, (i + 1) % 6) for i in range(6)], [16.0] * 6)
    add(3, [(0, 1), (1, 0)])                                                # a node without edges next to a pair
    return sizes, np.asarray(edges, dtype=np.int64).T, np.asarray(w, dtype=np.float32)


@pytest.mark.parametrize("H", [1, 70, 128])
def test_score_bit_for_bit(H):
    ops = _ops()
    sizes, ei, w = _exact_graphs()
    rng = np.random.default_rng(H)
    order = rng.permutation(ei.shape[1])
    ei, w = torch.from_numpy(np.ascontiguousarray(ei[:, order])), torch.from_numpy(w[order])
    N = sum(sizes)
    ptr = torch.tensor([0] + np.cumsum(sizes).tolist())
    x = torch.from_numpy(rng.integers(-3, 4, size=(N, H)).astype(np.float32))
    index = ops.HgpslIndex(ei[0].to(DEV), ei[1].to(DEV), ptr.to(DEV), N)
    for weights in (w, None):
        deg = torch.zeros(N, dtype=torch.float64).index_add_(0, ei[0], torch.ones(ei.shape[1], dtype=torch.float64) if weights is None else weights.double())
        assert set(deg.tolist()) <= {0.0, 1.0, 4.0, 16.0}
        want = R.score(x, ei, weights)
        wd = None if weights is None else weights.to(DEV)
        with ops.hgpsl_fused(True):
            got = ops.hgpsl_score(x.to(DEV), index, wd)
            again = ops.hgpsl_score(x.to(DEV), index, wd)
        assert got.dtype == torch.float32 and torch.equal(got.double().cpu(), want)
        assert torch.equal(got.view(torch.int32), again.view(torch.int32))
        with ops.hgpsl_fused(False):
            assert C.rel_max(ops.hgpsl_score(x.to(DEV), index, wd), want) < 1e-6      # (torch's pow(-0.5) need not be exact)


# ---------------------------------------------------------------------------------------------- top-k, exact
def _stable_topk(score, sizes, ks):
    perm, batch, inv, base = [], [], [-1] * sum(sizes), 0
    for g, (n, k) in enumerate(zip(sizes, ks)):
        order = sorted(range(n), key=lambda i: (-score[base + i], i))[:k]
        for i in order:
            inv[base + i] = len(perm)
            perm.append(base + i)
            batch.append(g)
        base += n
    return perm, batch, inv


@pytest.mark.parametrize("ratio", [0.3, 0.5, 0.8, 1.0])
def test_topk_equals_a_stable_sort(ratio):
    ops = _ops()
    limit = ops.HGPSL_TOPK_MAX_NODES
    assert limit == ops.lib().dn_hgpsl_topk_max_nodes()
    sizes = [0, 1, 2, 50, 63, 64, 65, 0, limit, limit + 1, 200]
    rng = np.random.default_rng(7)
    N = sum(sizes)
    score = rng.integers(0, 12, size=N).astype(np.float32)                   # deliberate ties, zeros among them
    ptr = torch.tensor([0] + np.cumsum(sizes).tolist())
    e = torch.zeros((2, 0), dtype=torch.long, device=DEV)
    index = ops.HgpslIndex(e[0], e[1], ptr.to(DEV), N)
    pooled = index.pooled(ratio)
    assert pooled.ks == [min(R.k_of(ratio, n), n) for n in sizes]
    if ratio == 0.3:
        assert pooled.ks[3] == 16
    perm, batch, inv = _stable_topk(score.tolist(), sizes, pooled.ks)
    for fused in (True, False):
        with ops.hgpsl_fused(fused):
            sel = ops.hgpsl_topk(torch.from_numpy(score).to(DEV), index, pooled)
        assert sel.perm.tolist() == perm and sel.batch.tolist() == batch and sel.inv.tolist() == inv, fused


# ---------------------------------------------------------------------------------------------- structure learning
def _structure_case(batch, sparse, weights, H):
    ops = _ops()
    assert (ops.HGPSL_WAVE_KEYS, ops.HGPSL_MAX_KEYS) == (64, 1024)
    lamb, slope, ratio = 0.5, 0.2, 0.8
    spec = C.STRUCT_BATCHES[batch]
    for seed in range(spec["seed0"][H], spec["seed0"][H] + 50):                 # (sparsemax: seeded until the support margin holds)
        b = C.structure_batch(H, seed, spec["sizes"], spec["scale"])
        perm, pptr, ref, (xr, ar, wr) = C.structure_reference(b, sparse, weights, lamb, slope, ratio)
        if not sparse or ref["support_margin"] > 1e-3:
            break
    assert not sparse or ref["support_margin"] > 1e-3
    assert np.diff(pptr).tolist() == spec["ks"]
    want = R.flat_blocks(ref["blocks"])
    coef = torch.from_numpy(np.random.default_rng(seed).standard_normal(want.numel()))
    (coef * want).sum().backward()
    ei = b["edge_index"].to(DEV)
    index = ops.HgpslIndex(ei[0], ei[1], torch.tensor(b["ptr"], device=DEV), b["x"].shape[0])
    pooled = index.pooled(ratio)
    assert pooled.ptr_host == pptr and pooled.big == spec["big"]
    assert pooled.max_wave == spec["max_wave"] and pooled.max_block == spec["max_block"]

    def run(fused):
        with ops.hgpsl_fused(fused):
            sel = ops.hgpsl_topk(b["score"].to(DEV), index, pooled)
            assert torch.equal(sel.perm.cpu(), perm)
            xp = b["x"].to(DEV)[sel.perm].requires_grad_(True)
            att = b["att"].to(DEV).requires_grad_(True)
            w = b["w"].to(DEV).requires_grad_(True) if weights else None
            blocks = ops.hgpsl_structure(xp, att, w, index, pooled, sel, sparse, lamb, slope)
            (coef.to(DEV).float() * blocks).sum().backward()
            eidx, _ = ops.hgpsl_compact(blocks, pooled)
        return blocks.detach(), eidx, xp.grad, att.grad, None if w is None else w.grad

    fused, composed, again = run(True), run(False), run(True)
    errs = {}
    for name, got in (("fused", fused), ("composed", composed)):
        if sparse:
            assert torch.equal((got[0] != 0).cpu(), want != 0), name            # the zero pattern
        assert torch.equal(got[1].cpu(), ref["edge_index"]), name
        errs[name] = C.rel_max(got[0], want)
        assert errs[name] < C.RTOL, (name, errs)
        errs[name + " grad xp"] = C.check_grad(got[2], xr.grad, (name, "xp"))
        errs[name + " grad att"] = C.check_grad(got[3], ar.grad, (name, "att"))
        if weights:
            errs[name + " grad w"] = C.check_grad(got[4], wr.grad, (name, "w"))
    errs["fused / composed"] = C.rel_max(fused[0], composed[0])
    assert errs["fused / composed"] < C.RTOL
    print({k: "%.1e" % v for k, v in errs.items()})
    for a, c in zip(fused, again):                                            # the same bits on the second run
        assert (a is None and c is None) or torch.equal(a, c)


@pytest.mark.parametrize("H", [6, 128])
@pytest.mark.parametrize("weights", [True, False], ids=["weights", "ones"])
@pytest.mark.parametrize("sparse", [False, True], ids=["softmax", "sparsemax"])
def test_structure_forward_and_backward(sparse, weights, H):
    assert C.STRUCT_BATCHES["classes"]["ks"] == [1, 63, 0, 64, 65, 1024, 1025]
    _structure_case("classes", sparse, weights, H)


@pytest.mark.parametrize("H", [6, 128])
@pytest.mark.parametrize("weights", [True, False], ids=["weights", "ones"])
@pytest.mark.parametrize("sparse", [False, True], ids=["softmax", "sparsemax"])
@pytest.mark.parametrize("batch", ["mid-512", "mid-256"])
def test_structure_between_the_class_limits(batch, sparse, weights, H):
    """The same over batches whose block-class launch sorts at n2 = 512 and at n2 = 256 (the batch above only meets n2 = 1024)."""
    _structure_case(batch, sparse, weights, H)


# ---------------------------------------------------------------------------------------------- the goldens under both paths
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "composed"])
@pytest.mark.parametrize("tag", C.layer_tags())
def test_layer_against_the_reference_golden(tag, fused):
    with _ops().hgpsl_fused(fused):
        errs = C.run_layer(tag, DEV)
    print(tag, {k: "%.1e" % v for k, v in errs.items()})


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "composed"])
def test_stack_against_the_reference_golden(fused):
    with _ops().hgpsl_fused(fused):
        errs = C.run_stack(DEV)
    print({k: "%.1e" % v for k, v in errs.items()})


# ---------------------------------------------------------------------------------------------- memory
@pytest.mark.parametrize("sparse", [False, True], ids=["softmax", "sparsemax"])
def test_layer_memory_stays_below_the_dense_matrix(sparse):
    """64 graphs of 32 nodes at ratio 0.8: N' = 64 x 26 = 1664.  The reference's dense [N', N'] float matrix alone is 4 N'^2 =
    11.1 MB; one layer's forward + backward here must peak below that."""
    ops = _ops()
    from dummynode4graphlearning_amd.graph_classification import HGPSLPool
    B, n, H = 64, 32, 32
    rng = np.random.default_rng(0)
    pairs = sorted({(g * n + int(a), g * n + int(b)) for g in range(B) for a, b in rng.integers(n, size=(4 * n, 2))})
    ei = torch.tensor(pairs, dtype=torch.long, device=DEV).t().contiguous()
    x = torch.from_numpy(rng.standard_normal((B * n, H)).astype(np.float32)).to(DEV).requires_grad_(True)
    w = torch.from_numpy(rng.uniform(0.2, 2.0, size=ei.shape[1]).astype(np.float32)).to(DEV).requires_grad_(True)
    batch = torch.arange(B, device=DEV).repeat_interleave(n)
    index = ops.HgpslIndex(ei[0], ei[1], torch.arange(0, B * n + 1, n, device=DEV), B * n)
    layer = HGPSLPool(H, ratio=0.8, sparse=sparse).to(DEV)
    for fused in (True, False):
        with ops.hgpsl_fused(fused):
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            xo, eo, ea, bo = layer(x, ei, w, batch, index=index)
            (xo.sum() + (ea * ea).sum()).backward()
            torch.cuda.synchronize()
            peak = torch.cuda.max_memory_allocated() - base
        assert xo.shape[0] == 1664
        print("fused" if fused else "composed", "peak %.2f MB of %.2f MB" % (peak / 1e6, 4 * 1664 ** 2 / 1e6))
        assert peak < 4 * 1664 ** 2, (fused, peak)
        x.grad = w.grad = layer.att.grad = None


# ---------------------------------------------------------------------------------------------- read-backs
def test_a_layer_reads_nothing_back_but_the_pair_count():
    """Under torch's sync debug mode "error" (after checking that this build honours it): with the batch's index at hand, the score,
    the top-k, the gather, the structure learning and the whole backward read nothing back, and neither does the pooled batch's
    index, which is built from host sizes.  The compaction's nonzero is the layer's one sync and stays outside."""
    ops = _ops()
    b = C.structure_batch(6, C.STRUCT_SEED0[6])
    ei = b["edge_index"].to(DEV)
    index = ops.HgpslIndex(ei[0], ei[1], torch.tensor(b["ptr"], device=DEV), b["x"].shape[0])       # (the one read-back)
    pooled = index.pooled(0.8)
    x, att, w = b["x"].to(DEV).requires_grad_(True), b["att"].to(DEV).requires_grad_(True), b["w"].to(DEV).requires_grad_(True)

    def run():
        sel = ops.hgpsl_topk(ops.hgpsl_score(x, index, w), index, pooled)
        blocks = ops.hgpsl_structure(ops.gather_rows(x, sel.perm32), att, w, index, pooled, sel, True, 0.5, 0.2)
        blocks.sum().backward()
        return blocks

    with ops.hgpsl_fused(True):
        e1, _ = ops.hgpsl_compact(run(), pooled)                              # (first use: library load, allocator; the sync)
        probe = torch.ones(1, device=DEV)
        torch.cuda.synchronize()
        prev = torch.cuda.get_sync_debug_mode()
        torch.cuda.set_sync_debug_mode("error")
        try:
            with pytest.raises(RuntimeError):
                probe.item()                                                   # the mode is honoured: a plain read-back raises
            run()
            nxt = ops.HgpslIndex(e1[0], e1[1], pooled.graph_ptr, pooled.num_rows, sizes=pooled.ks)
        finally:
            torch.cuda.set_sync_debug_mode(prev)
    assert nxt.sizes == pooled.ks and nxt.num_edges == e1.shape[1]
