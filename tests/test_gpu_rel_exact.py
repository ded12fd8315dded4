"""Bit-exact parity of the aggregate-then-transform ("two-pass") relation path and of everything only RGCN uses, on operands where the
arithmetic is exact (tests/rel_exact_ref.py):
  A. ops.RelIndex (dn_rel_index_build_i32): the ten tables, num_segments and rel_ptr_host against the numpy restatement, torch.equal;
     the three row tables decoded as their consumers read them;
  B. ops.rel_agg_transform: output and both gradients against float64 index_add + autograd rounded once, fp32 in both arithmetic modes
     and bf16, with and without an edge scale that differs inside the segments, at the edges of the chunk tables of both
     weight-gradient forms;
  C. graph_classification RGCNConv (mean / add, root, bias) on that path;
  D. subgraph_isomorphism RGCNLayer with edge_norm none / in / both on both of its formulations, ops.degrees and ops.edge_norm.
Every comparison is atol = rtol = 0; the one exception is the mean over 3 and 5 edges, held to the 1-ulp rule of
gc_exact_ref.assert_mean.  Every case holds its premise first (proven without a GPU by tests/test_rel_exact_premise.py) and asserts the
path it took (ops.KernelTimer tags).  A dropped edge, a scale taken in the other pass's edge order, a chunk one row short at a relation
boundary or a norm applied on the wrong side changes bits here where the tolerance tests of the same code (1e-4 .. 5e-3) can pass."""
import os
import threading
import time
from contextlib import contextmanager, nullcontext

import numpy as np
import pytest
import torch

import exact_ref as X
import gc_exact_ref as G
import rel_exact_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FUZZ_SECONDS = float(os.environ.get("DN_REL_EXACT_FUZZ_SECONDS", "4"))


def _ops():
    from dummynode4graphlearning_amd import ops
    return ops


def _t(a):
    return torch.as_tensor(np.asarray(a, dtype=np.int64), device=DEV)


@contextmanager
def traced():
    """-> record: ['tags'] of the launches inside the block, ['any'] = calls of ops.rows_wgrad_any (which carries no tag)"""
    ops = _ops()
    rec = {"tags": [], "any": 0}
    timer, inner = ops.KernelTimer(), ops.rows_wgrad_any

    def counted(*a, **kw):
        rec["any"] += 1
        return inner(*a, **kw)
    ops.rows_wgrad_any = counted
    try:
        with timer:
            yield rec
    finally:
        ops.rows_wgrad_any = inner
        rec["tags"] = [r[0] for r in timer.records]


# ---- A. the relation index -------------------------------------------------------------------------------------------------------
def _check_index(ix, src, dst, et, N, Rn, what):
    ops = _ops()
    ref = R.rel_index_ref(src, dst, et, N, Rn)
    assert ix.num_segments == ref["P"], "%s: num_segments %d, want %d" % (what, ix.num_segments, ref["P"])
    assert ix.rel_ptr_host == ref["rel_ptr_host"], "%s: rel_ptr_host %s, want %s" % (what, ix.rel_ptr_host[:12], ref["rel_ptr_host"][:12])
    for k in R.INDEX_TABLES:
        got, want = getattr(ix, k), torch.from_numpy(ref[k])
        assert got.dtype == torch.int32 and got.shape == want.shape, "%s: %s has shape %s, want %s" % (what, k, tuple(got.shape), tuple(want.shape))
        if not torch.equal(got.cpu().long(), want):
            bad = (got.cpu().long() != want).nonzero().reshape(-1)
            raise AssertionError("%s: %s differs at %d of %d positions, first %d: got %d, want %d" % (
                what, k, bad.numel(), want.numel(), int(bad[0]), int(got[int(bad[0])]), int(want[int(bad[0])])))
    rp = ref["rel_ptr_host"]
    tiles, m = ix.gemm_tiles
    assert m == tiles.shape[0]
    R.check_row_table(tiles.cpu().numpy(), rp, 64, None, what + " gemm_tiles")
    for name, step in (("gemm_chunks", 1024), ("chunk_table", ops.WGRAD_CHUNK_ROWS)):
        table, pptr, m = getattr(ix, name)
        assert m == table.shape[0]
        R.check_row_table(table.cpu().numpy(), rp, step, pptr.cpu().numpy(), "%s %s" % (what, name))
    return ref


@pytest.mark.parametrize("name", list(R.INDEX_CASES))
def test_rel_index_equals_the_restatement(name):
    ops = _ops()
    assert ops.WGRAD_CHUNK_ROWS == R.WGRAD_CHUNK_ROWS          # (the sizes of 'table-edges' sit at this step's edges)
    src, dst, et, N, Rn = R.INDEX_CASES[name]
    ix = ops.RelIndex(_t(src), _t(dst), _t(et), N, Rn)
    _check_index(ix, src, dst, et, N, Rn, name)
    again = ops.RelIndex(_t(src), _t(dst), _t(et), N, Rn)
    for k in R.INDEX_TABLES:
        assert torch.equal(getattr(ix, k), getattr(again, k)), k


def _synthetic(raw):
    from dummynode4graphlearning_amd import transforms
    keys = ("node_ptr", "edge_ptr", "src", "dst", "node_id", "node_label", "edge_id", "edge_label")
    aug = transforms.dummy_augment_si(*(torch.from_numpy(raw[k]).to(DEV) for k in keys), raw["max_nv"], raw["max_nvl"], raw["max_ne"],
                                      raw["max_nel"])
    return tuple(aug[k].long().cpu().numpy() for k in ("src", "dst", "edge_label", "node_ptr", "edge_ptr"))


def test_rel_index_of_a_dummy_augmented_si_batch_and_of_a_gc_batch():
    from dummynode4graphlearning_amd import BatchedGraph, synthetic
    from dummynode4graphlearning_amd.graph import GraphBatch, rel_index_of
    raw = synthetic.config3(seed=3, graphs=24)
    src, dst, et, nptr, eptr = _synthetic(raw)
    N, Rn = int(nptr[-1]), raw["num_rels"]
    assert set(int(v) for v in et) >= {Rn - 2, Rn - 1}                # the dummy relations are there
    g = BatchedGraph(_t(src), _t(dst), N, _t(np.diff(nptr)), _t(np.diff(eptr)))
    etype = _t(et)
    ix = g.rel_index(etype, Rn)
    _check_index(ix, src, dst, et, N, Rn, "SI batch")
    assert g.rel_index(etype, Rn) is ix                               # cached on the graph
    b = synthetic.config1(seed=1)
    N = int(b["node_ptr"][-1])
    data = GraphBatch(torch.zeros(N, 3, device=DEV), torch.stack([_t(b["src"]), _t(b["dst"])]),
                      batch=_t(np.repeat(np.arange(len(b["node_ptr"]) - 1), np.diff(b["node_ptr"]))))
    et = b["edge_label"] - 1
    ix = rel_index_of(data, _t(et), 4)
    _check_index(ix, b["src"], b["dst"], et, N, 4, "GC batch")


def test_rel_index_random_sweep():
    """About 200 seeded builds of mixed sizes (E up to 3,000) against the restatement, for at most DN_REL_EXACT_FUZZ_SECONDS."""
    ops = _ops()
    rng = np.random.default_rng(77)
    t0, n = time.time(), 0
    while n < 200 and (n < 10 or time.time() - t0 < FUZZ_SECONDS):
        src, dst, et, N, Rn = R.sweep_case(rng)
        _check_index(ops.RelIndex(_t(src), _t(dst), _t(et), N, Rn), src, dst, et, N, Rn, "sweep build %d (N=%d R=%d E=%d)" % (n, N, Rn, len(src)))
        n += 1
    assert n >= 10


# ---- B. rel_agg_transform --------------------------------------------------------------------------------------------------------
def _agg_inputs(c):
    ops = _ops()
    ix = ops.RelIndex(_t(c.src), _t(c.dst), _t(c.et), c.N, c.R)
    x, W, g = (t.to(DEV, c.dtype) for t in (c.x, c.W, c.g))
    scale = c.scale.to(DEV, torch.float32) if c.scale is not None else None
    return ix, x, W, g, scale


def _agg_run(ix, x, W, g, scale):
    ops = _ops()
    x, W = x.clone().requires_grad_(True), W.clone().requires_grad_(True)
    out = ops.rel_agg_transform(x, W, ix, edge_scale=scale)
    out.backward(g)
    return out.detach(), x.grad, W.grad


@pytest.mark.parametrize("p", R.agg_params(), ids=R.agg_ids())
def test_rel_agg_transform_is_bit_exact(p):
    ops = _ops()
    c = R.agg_case(*p)
    c.premise()
    ix, x, W, g, scale = _agg_inputs(c)
    assert ix.rel_ptr_host == c.ix["rel_ptr_host"]
    mode = ops.f32_exact(True) if c.mode == "f32x" else nullcontext()
    with mode, traced() as rec:
        got = _agg_run(ix, x, W, g, scale)
    tags = rec["tags"]
    if c.square:                                                       # the matrix-core form gathers g by seg_dst itself
        assert tags.count("rows_wgrad") == 1 and rec["any"] == 0, (tags, rec["any"])
    else:
        assert "rows_wgrad" not in tags and rec["any"] == 1, (tags, rec["any"])
    assert tags.count("rows_gemm") == 2 and tags.count("gather_segsum") == 4, tags
    seg_rel = np.repeat(np.arange(c.R), np.diff(c.ix["rel_ptr_host"]))
    X.assert_bits(got[0], c.out, c.what + " output")
    X.assert_bits(got[1], c.gx, c.what + " input gradient")
    X.assert_bits(got[2], c.gW, c.what + " weight gradient", rel=np.arange(c.R))
    assert got[2].dtype == c.dtype and len(seg_rel) == ix.num_segments
    with mode:
        again = _agg_run(ix, x, W, g, scale)
    for a, b, n in zip(got, again, ("output", "input gradient", "weight gradient")):
        assert torch.equal(a, b), "%s: the second call's %s differs" % (c.what, n)


@pytest.mark.parametrize("fwd_exact", [True, False], ids=["forward-exact", "forward-split"])
@pytest.mark.parametrize("where", ["context", "thread"])
def test_rel_agg_transform_backward_keeps_the_forward_mode(fwd_exact, where):
    """_backward_in_forward_mode: a backward run after the fp32 mode has changed -- inside another `with`, or from a thread with its own
    override -- gives the bits of the forward's mode.  Operands of 24 significant bits, on which the two modes differ (required)."""
    ops = _ops()
    c = R.agg_case(64, 64, "f32s", True)
    ix = ops.RelIndex(_t(c.src), _t(c.dst), _t(c.et), c.N, c.R)
    gen = torch.Generator().manual_seed(5)
    x, g = torch.randn(c.N, 64, generator=gen).to(DEV), torch.randn(c.N, 64, generator=gen).to(DEV)
    W = torch.randn(c.R, 64, 64, generator=gen).to(DEV)
    scale = c.scale.to(DEV, torch.float32)
    with ops.f32_exact(True):
        exact = _agg_run(ix, x, W, g, scale)
    with ops.f32_exact(False):
        split = _agg_run(ix, x, W, g, scale)
    assert not torch.equal(exact[2], split[2]), "the two modes agree on these operands: the test would show nothing"
    want = exact if fwd_exact else split
    xg, Wg = x.clone().requires_grad_(True), W.clone().requires_grad_(True)
    with ops.f32_exact(fwd_exact):
        out = ops.rel_agg_transform(xg, Wg, ix, edge_scale=scale)
    if where == "context":
        with ops.f32_exact(not fwd_exact):
            out.backward(g)
    else:
        def work():
            with ops.f32_exact(not fwd_exact):
                out.backward(g)
        th = threading.Thread(target=work)
        th.start()
        th.join()
    torch.cuda.synchronize()
    assert torch.equal(out.detach(), want[0]) and torch.equal(xg.grad, want[1])
    assert torch.equal(Wg.grad, want[2]), "the weight gradient ran in the mode of the backward's caller"


# ---- C. GC RGCNConv --------------------------------------------------------------------------------------------------------------
def _conv(c_fin, c_fout, Rn, aggr, root, bias, dtype, p):
    from dummynode4graphlearning_amd.graph_classification import RGCNConv
    conv = RGCNConv(c_fin, c_fout, Rn, aggr=aggr, root_weight=root, bias=bias).to(DEV).to(dtype)
    X.load_params(conv, p)
    return conv


def _conv_run(conv, x, src, dst, et, g):
    from dummynode4graphlearning_amd.graph import GraphBatch
    for q in conv.parameters():
        q.grad = None
    x = x.clone().requires_grad_(True)
    data = GraphBatch(x, torch.stack([_t(src), _t(dst)]))
    with traced() as rec:
        out = conv(x, data, _t(et))
        out.backward(g)
    return rec, out.detach(), x.grad, {k: v.grad for k, v in conv.named_parameters()}


_FUSED_TAGS = ("conv_graphs", "rows_close", "rows_selfsum", "layer_graphs_fwd")


def _is_pipeline(tags):
    return any(t.startswith("rows_transform") or t in _FUSED_TAGS for t in tags)


@pytest.mark.parametrize("p", R.conv_params(), ids=[R.conv_id(p) for p in R.conv_params()])
def test_rgcn_conv_is_bit_exact(p):
    fin, fout, aggr, root, bias, dt = p
    c = R.conv_case(*p)
    c.premise()
    conv = _conv(fin, fout, c.R, aggr, root, bias, c.dtype, c.p)
    x, g = c.x.to(DEV, c.dtype), c.g.to(DEV, c.dtype)
    rec, out, gx, gp = _conv_run(conv, x, c.src, c.dst, c.et, g)
    tags = rec["tags"]
    if c.fused:                                                        # add + root at H = 64: the row-factorised pipeline
        assert _is_pipeline(tags) and "rows_gemm" not in tags, tags
    else:                                                              # everything else, every mean among it: the two-pass path
        assert not _is_pipeline(tags) and tags.count("rows_gemm") == 2, tags
        assert (tags.count("rows_wgrad") == 1 and rec["any"] == 0) if fin == fout == 64 else (rec["any"] == 1 and "rows_wgrad" not in tags), tags
    X.assert_bits(out, c.out, c.what + " output")
    X.assert_bits(gx, c.gx, c.what + " input gradient")
    assert set(gp) == set(c.gp)
    for k, v in gp.items():
        X.assert_bits(v, c.gp[k], c.what + " gradient of " + k, rel=np.arange(c.R) if k == "weight" else None)
    rec2, out2, gx2, gp2 = _conv_run(conv, x, c.src, c.dst, c.et, g)
    assert torch.equal(out, out2) and torch.equal(gx, gx2) and all(torch.equal(gp[k], gp2[k]) for k in gp)


@pytest.mark.parametrize("H,dt", [(32, "f32"), (32, "bf16"), (64, "f32"), (64, "bf16")])
def test_rgcn_conv_mean_over_3_and_5_edges_within_one_ulp(H, dt):
    """The stated exception: 1 / 3 and 1 / 5 are rounded, so the output and the input gradient are held to gc_exact_ref.assert_mean --
    bit-exact where the segment's length is a power of two (or the node has no edge), at most 1 ulp from the correctly rounded quotient
    elsewhere (rel_exact_ref.MeanCase: every element is ONE source entry times the reciprocal)."""
    c = R.MeanCase(H, dt)
    c.premise()
    conv = _conv(H, H, c.R, "mean", False, False, c.dtype, {"weight": c.W})
    rec, out, gx, _ = _conv_run(conv, c.x.to(DEV, c.dtype), c.src, c.dst, c.et, c.g.to(DEV, c.dtype))
    assert not _is_pipeline(rec["tags"]) and rec["tags"].count("rows_gemm") == 2, rec["tags"]
    G.assert_mean(out, c.out_total, c.out_lens, "RGCNConv mean H=%d %s output" % (H, dt))
    G.assert_mean(gx, c.gx_total, c.gx_lens, "RGCNConv mean H=%d %s input gradient" % (H, dt))


# ---- D. SI RGCNLayer, degrees, edge_norm -----------------------------------------------------------------------------------------
def _graph(batch):
    from dummynode4graphlearning_amd import BatchedGraph
    src, dst, et, nptr, eptr = batch
    return BatchedGraph(_t(src), _t(dst), int(nptr[-1]), _t(np.diff(nptr)), _t(np.diff(eptr)), node_ptr=_t(nptr).to(torch.int32),
                        edge_ptr=_t(eptr).to(torch.int32))


def _layer_run(layer, g, c, et):
    for q in layer.parameters():
        q.grad = None
    x = c.x.to(DEV, c.dtype).clone().requires_grad_(True)
    with traced() as rec:
        out, _ = layer(g, x, et)
        out.backward(c.coef.to(DEV, c.dtype))
    return rec, out.detach(), x.grad, {k: v.grad for k, v in layer.named_parameters()}


@pytest.mark.parametrize("name", list(R.LAYER_CASES))
def test_rgcn_layer_is_bit_exact(name):
    from dummynode4graphlearning_amd.subgraph_isomorphism import RGCNLayer
    c = R.layer_case(name)
    c.premise()
    layer = RGCNLayer(c.fin, c.fout, num_rels=c.R, edge_norm=c.edge_norm, self_loop=c.self_loop, act_func=c.act, **c.kw).to(DEV).to(c.dtype)
    X.load_params(layer, c.p)
    et = _t(c.batch[2])

    def norms_are_exact(gr, when):
        n = c.norms
        assert torch.equal(gr.ndata["in_deg"].cpu(), torch.from_numpy(n["in_deg"])), when + ": in-degrees"
        X.assert_bits(gr.ndata["in_norm"].view(-1), n["in_norm"], "%s in_norm (%s)" % (name, when))
        if c.edge_norm == "both":
            assert torch.equal(gr.ndata["out_deg"].cpu(), torch.from_numpy(n["out_deg"])), when + ": out-degrees"
            X.assert_bits(gr.ndata["out_norm"].view(-1), n["out_norm"], "%s out_norm (%s)" % (name, when))
        X.assert_bits(gr.edata["norm"].view(-1), n["edge_in" if c.edge_norm == "in" else "edge_both"], "%s edge norm (%s)" % (name, when))
        assert gr.ndata["in_norm"].dtype == torch.float32 and gr.edata["norm"].dtype == torch.float32

    # the norms first, on a graph object of their own, bit for bit against float64: a failure here is the norm kernels', not the layer's
    if c.edge_norm != "none":
        g0 = _graph(c.batch)
        layer._norms(g0)
        norms_are_exact(g0, "direct call")
    g = _graph(c.batch)                                                # a fresh graph: the first forward computes and caches the norms
    assert "norm" not in g.edata and "in_norm" not in g.ndata
    rec, out, gx, gp = _layer_run(layer, g, c, et)
    tags = rec["tags"]
    if c.edge_norm != "none":
        norms_are_exact(g, "cached by the first forward")
    if not c.fused:                                                    # generic: per-edge norm in the first gather, self loop in torch
        assert tags.count("rows_gemm") == 2 and not _is_pipeline(tags), tags
    elif c.dtype == torch.bfloat16 and c.fin == 64 and c.self_loop:
        # one whole-graph launch per direction.  Only with the self loop: dn_conv_graphs_bf16 computes the self-loop term itself
        # (ops.conv_graphs_ok asks for it), so H = 64 bf16 WITHOUT the loop is on the row pipeline like the other widths
        assert tags.count("conv_graphs") == 2 and "rows_gemm" not in tags, tags
    else:
        assert "rows_transform:conv" in tags and "conv_graphs" not in tags and "rows_gemm" not in tags, tags
    ref_out, ref_gx, ref_gp = c.ref
    X.assert_bits(out, ref_out, c.what + " output", graph=c.graph_of_row)
    X.assert_bits(gx, ref_gx, c.what + " input gradient", graph=c.graph_of_row)
    assert set(gp) == set(ref_gp)
    for k, v in gp.items():
        X.assert_bits(v, ref_gp[k], c.what + " gradient of " + k)
    # again on the same graph object: this call reads the cached norm / in_norm / out_norm and the cached index
    rec2, out2, gx2, gp2 = _layer_run(layer, g, c, et)
    assert rec2["tags"] == tags
    assert torch.equal(out, out2) and torch.equal(gx, gx2) and all(torch.equal(gp[k], gp2[k]) for k in gp), "the second call differs"


@pytest.mark.parametrize("name", list(R.DEGREE_CASES))
def test_degrees_and_edge_norm_are_exact(name):
    """ops.degrees: integer counts, identical and repeatable; ops.edge_norm in both modes and under both self_loop flags against float64
    1 / (d + loop) (0 for degree 0 without the loop) rounded once -- the node norms at every degree (a hub of 5,000 among them), the edge
    norm of mode 'in' and of mode 'both' everywhere (mode 'both': the fp32 restatement sqrt(out_norm[src] * in_norm[dst]), which is the
    float64 value where the degrees are powers of four)."""
    ops = _ops()
    src, dst, N = R.DEGREE_CASES[name]
    s, d = _t(src).to(torch.int32), _t(dst).to(torch.int32)
    ind, outd = ops.degrees(s, d, N)
    ind2, outd2 = ops.degrees(s, d, N)
    assert torch.equal(ind, ind2) and torch.equal(outd, outd2)
    for self_loop in (True, False):
        n = R.norms_ref(src, dst, N, self_loop)
        assert torch.equal(ind.cpu().long(), torch.from_numpy(n["in_deg"])) and torch.equal(outd.cpu().long(), torch.from_numpy(n["out_deg"]))
        in_norm, none, en = ops.edge_norm("in", self_loop, s, d, ind, ind)
        assert none is None and in_norm.shape == (N, 1) and en.shape == (len(src),)
        X.assert_bits(in_norm.view(-1), n["in_norm"], "%s in_norm (mode in, loop %d)" % (name, self_loop))
        X.assert_bits(en, n["edge_in"], "%s edge norm (mode in, loop %d)" % (name, self_loop))
        in_norm, out_norm, en = ops.edge_norm("both", self_loop, s, d, ind, outd)
        X.assert_bits(in_norm.view(-1), n["in_norm"], "%s in_norm (mode both, loop %d)" % (name, self_loop))
        X.assert_bits(out_norm.view(-1), n["out_norm"], "%s out_norm (mode both, loop %d)" % (name, self_loop))
        # mode 'both' per edge: the fp32 square root of the fp32 product of the two fp32 norms, every step correctly rounded --
        # restated in numpy fp32 and compared bit for bit at every degree; where the degrees are powers of four it is the float64 value too
        f32 = lambda t: t.numpy().astype(np.float32)  # noqa: E731
        want = np.sqrt(f32(n["out_norm"])[src] * f32(n["in_norm"])[dst])
        assert want.dtype == np.float32
        X.assert_bits(en, torch.from_numpy(want.astype(np.float64)), "%s edge norm (mode both, loop %d)" % (name, self_loop))
        if name == "powers-of-four" and not self_loop:
            X.assert_bits(en, n["edge_both"], "%s edge norm (mode both) against float64" % name)
        if not self_loop:                                              # every case holds a node without in-edges: its norm is 0, not inf
            zero = torch.from_numpy(n["in_deg"] == 0)
            assert bool(zero.any()) and bool((in_norm.view(-1).cpu()[zero] == 0).all()) and bool(torch.isfinite(in_norm).all())
