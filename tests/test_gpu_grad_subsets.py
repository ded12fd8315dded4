"""Every backward branch that `requires_grad` selects, bit for bit.  ops.py's autograd functions read ctx.needs_input_grad and then
skip a launch, form an operand by another route (_RowTransformFn rebuilds the backward pre-aggregated rows with gather_segsum when x
takes no gradient) or call a kernel nothing else calls (_LinearActFn: dn_relu_bwd_* with frozen weights); the rest of the suite makes
every leaf require a gradient.  Here a case is one operator, one shape, one dtype (tests/grad_subset_ref.py; operands proven exact by
tests/test_grad_subsets_premise.py) and it runs under every subset of its differentiable inputs -- all inputs, each subset, all inputs
again, on index objects built once per shape, so that a subset run can leave nothing behind that a later run reads:
  1. the output equals the float64 reference rounded once to the operator's dtype;
  2. an input outside the subset has .grad None;
  3. an input inside it has the reference's gradient, bit for bit, in the input's dtype and shape;
  4. the launch tags (ops.KernelTimer) say which branch ran, where the branch shows there.
BatchNorm is the one operator compared within a bound (the bound of test_batch_norm_rows_matches_torch in tests/test_gpu_kernels.py).

Left out on purpose: _HgtAttnFn, _SegAttnFn, _LrpPoolFn, _WeightedSegsumFn, _SegmentReduce, _NeighborMax, _EdgeSum, _GatherRows, the
pool functions and _BddDenseFn have no branch on needs_input_grad; their backward is pinned by their own files.  The fused H = 256 MLP
backward (from MLP_BWD_FUSED_MIN_ROWS rows on) is covered by tests/test_gpu_mlp_bwd_fused.py."""
import contextlib
import types
from collections import Counter

import numpy as np
import pytest
import torch

import exact_ref as X
import grad_subset_ref as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _ops():
    from dummynode4graphlearning_amd import ops
    return ops


@contextlib.contextmanager
def switches(**kw):
    ops = _ops()
    old = {k: getattr(ops, k) for k in kw}
    try:
        for k, v in kw.items():
            setattr(ops, k, v)
        yield
    finally:
        for k, v in old.items():
            setattr(ops, k, v)


def _dev(t, dtype=None):
    return t.to(DEV) if dtype is None else t.to(DEV).to(dtype)


def _i32(t):
    return t.to(DEV).to(torch.int32)


def _run(c, sub, call, used=None):
    """One forward and backward of the operator with the inputs of `sub` requiring gradients
    -> (outputs, {name: .grad}, forward tags, backward tags)"""
    ops = _ops()
    used = tuple(range(len(c.coefs))) if used is None else tuple(used)
    leaves = {k: _dev(v, c.in_dtype.get(k, c.dtype)).requires_grad_(k in sub) for k, v in c.ins.items()}
    with ops.f32_exact(c.mode == "f32x"):
        with ops.KernelTimer() as tf:
            outs = call(leaves)
        outs = outs if isinstance(outs, tuple) else (outs,)
        with ops.KernelTimer() as tb:
            torch.autograd.backward([outs[i] for i in used], [_dev(c.coefs[i], outs[i].dtype) for i in used])
    torch.cuda.synchronize()
    return outs, {k: v.grad for k, v in leaves.items()}, [r[0] for r in tf.records], [r[0] for r in tb.records]


def _check(c, sub, got, used=None, what=""):
    outs, grads = got[0], got[1]
    ref_outs, ref_grads = c.run(sub, used)
    what = "%s%s, gradients to %s: " % (what, c.what, "+".join(sub))
    for i, (o, r) in enumerate(zip(outs, ref_outs)):
        assert o.dtype == c.dtype, (what, o.dtype)
        X.assert_bits(o, r, what + "output %d" % i)
    for k in c.names:
        if k not in sub:
            assert grads[k] is None, what + "%s takes no gradient but got one" % k
            continue
        assert grads[k] is not None, what + "no gradient for " + k
        assert grads[k].dtype == c.in_dtype.get(k, c.dtype) and tuple(grads[k].shape) == tuple(c.ins[k].shape), (what, k)
        X.assert_bits(grads[k], ref_grads[k], what + "gradient of " + k)


def _sweep(c, subs, call, tag_check=None):
    """all inputs, each subset, all inputs again; tag_check(subset, forward tags, backward tags, the all-inputs run's backward tags)"""
    assert tuple(subs[0]) == c.names
    first = None
    for n, sub in enumerate(S.run_order(subs)):
        got = _run(c, sub, call)
        _check(c, sub, got, what="run %d: " % n)
        if first is None:
            first = got
        if tag_check is not None:
            tag_check(tuple(sub), got[2], got[3], first[3])
    return first


def _proper_sub_multiset(a, b):
    a, b = Counter(a), Counter(b)
    return all(b[k] >= v for k, v in a.items()) and sum(a.values()) < sum(b.values())


def test_the_mirrored_constants_are_the_librarys():
    ops = _ops()
    assert ops.HUB_SPLIT == S.HUB_SPLIT
    assert (ops.DUAL_EDGE, ops.DUAL_SUB, ops.DUAL_MULT) == (S.DUAL_EDGE, S.DUAL_SUB, S.DUAL_MULT)


# ---- relu_bwd (dn_relu_bwd_bf16 / _f32) -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["bf16", "f32"])
@pytest.mark.parametrize("slope", [0.0, 0.25])
@pytest.mark.parametrize("numel", S.RELU_BWD_NUMEL)
def test_relu_bwd(numel, slope, mode):
    """(y > 0) ? g : slope * g against torch.where on small integers -- exact by construction; ties at 0 take the slope"""
    ops = _ops()
    g, y, want = S.relu_bwd_case(numel, slope, mode)
    dt = S.DTYPES[mode]
    gd, yd = _dev(g, dt), _dev(y, dt)
    out = ops.relu_bwd(gd, yd, slope)
    assert out.dtype == dt and out.shape == gd.shape
    X.assert_bits(out, want, "relu_bwd numel=%d slope=%g %s" % (numel, slope, mode))
    X.assert_bits(out, torch.where(yd > 0, gd, slope * gd).double().cpu(), "relu_bwd against torch.where on the device")
    X.assert_bits(gd, g, "relu_bwd changed its input")
    X.assert_bits(yd, y, "relu_bwd changed its mask")


# ---- linear_act ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,H,mode,relu,bias", S.LINEAR_ACT)
def test_linear_act(rows, H, mode, relu, bias):
    ops = _ops()
    c = S.linear_act_case(rows, H, mode, relu, bias)
    called = []
    real = ops.relu_bwd

    def rec(*a, **k):
        called.append(1)
        return real(*a, **k)

    def call(t):
        return ops.linear_act(t["x"], t["w0"], t.get("b0"), relu=relu, exact=False if mode == "f32s" else None)

    def tags(sub, tf, tb, tb_all):
        n = len(called)
        del called[:]
        assert tf == ["rows_transform:dense"], tf
        if sub == ("x",):
            # frozen weight and bias: no weight-gradient launch; with a ReLU the mask is applied by relu_bwd instead
            assert "rows_wgrad" not in tb and tb == ["rows_transform:dense"], tb
            assert n == (1 if relu else 0), n
        else:
            assert tb.count("rows_wgrad") == 1 and n == 0, (tb, n)
            assert ("rows_transform:dense" in tb) == ("x" in sub), (sub, tb)

    with switches(relu_bwd=rec):
        _sweep(c, S.subsets(c.names), call, tags)


# ---- relu_mlp --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,H,mode,slope,rows", S.RELU_MLP)
def test_relu_mlp_with_and_without_an_input_gradient(L, H, mode, slope, rows):
    ops = _ops()
    c = S.relu_mlp_case(L, H, mode, slope, rows)
    assert rows < ops.MLP_BWD_FUSED_MIN_ROWS

    def call(t):
        lin = [types.SimpleNamespace(weight=t["w%d" % i], bias=t["b%d" % i]) for i in range(L)]
        assert ops.relu_mlp_supported(t["x"], lin)
        return ops.relu_mlp(t["x"], lin, slope)

    def tags(sub, tf, tb, tb_all):
        assert "mlp_bwd_fused" not in tb, tb
        if L == 2:                                             # the chain paths: one launch forward, three backward, x or no x
            assert tf == ["rows_chain2"] and sorted(tb) == ["rows_chain2", "rows_wgrad", "rows_wgrad"], (tf, tb)
        else:                                                  # the generic loop: its last input-gradient launch only where x asks
            assert tf == ["rows_transform:dense"] * L and tb.count("rows_wgrad") == L, (tf, tb)
            assert tb.count("rows_transform:dense") == (L if "x" in sub else L - 1), (sub, tb)

    _sweep(c, S.subsets(c.names, "first"), call, tags)


# ---- rel_transform_fused ---------------------------------------------------------------------------------------------------------
_CONV_INDEX = {}


def _conv_index(c):
    """one RowIndexSet per graph, shared by the widths, dtypes and subsets (built once: its tables are cached on it)"""
    ops = _ops()
    if c.hubs not in _CONV_INDEX:
        _CONV_INDEX[c.hubs] = ops.RowIndexSet(_dev(c.src), _dev(c.dst), _dev(c.et), c.N, c.R, True)
    return _CONV_INDEX[c.hubs]


@pytest.mark.parametrize("H,mode,hubs", S.CONV)
def test_rel_transform_fused(H, mode, hubs):
    ops = _ops()
    c = S.conv_case(H, mode, hubs)
    iset = _conv_index(c)
    ix = iset.index
    if hubs:
        # relation 1 (every edge into node 0) is collapsed forward, relation 2 (every edge out of node 1) backward: the index says so
        assert ix.num_aux_f > 0 and ix.num_aux_b > 0, (ix.num_aux_f, ix.num_aux_b, ix.modes)
        assert ix.modes == [ops.RowIndex.EDGE, ops.RowIndex.AGG, ops.RowIndex.TF], ix.modes
    else:
        assert ix.num_aux_b == 0 and ix.num_aux_f == 0 and ix.modes == [ops.RowIndex.EDGE] * 3, ix.modes

    def call(t):
        assert ops.fused_path_supported(t["x"], t["W"])
        return ops.rel_transform_fused(t["x"], t["W"], t["bias"], iset, W_loop=t["W_loop"])

    def tags(sub, tf, tb, tb_all):
        if "x" not in sub:
            # no backward message pass: the weight-gradient launch, and the gather that rebuilds the backward pre-aggregated rows
            assert tb.count("rows_wgrad") == 1 and _proper_sub_multiset(tb, tb_all), (sub, tb, tb_all)
            assert tb == (["gather_segsum"] if hubs else []) + ["rows_wgrad"], tb
        elif sub == ("x",):
            assert "rows_wgrad" not in tb and _proper_sub_multiset(tb, tb_all), (tb, tb_all)
        else:
            assert Counter(tb) == Counter(tb_all), (sub, tb, tb_all)

    _sweep(c, S.subsets(c.names), call, tags)


# ---- the RGIN layer functions ------------------------------------------------------------------------------------------------------
def _batched_graph(batch):
    from dummynode4graphlearning_amd import BatchedGraph
    src, dst, et, nptr, eptr = batch
    t = lambda a: torch.as_tensor(np.asarray(a, dtype=np.int64), device=DEV)  # noqa: E731
    return BatchedGraph(t(src), t(dst), int(nptr[-1]), t(np.diff(nptr)), t(np.diff(eptr)), node_ptr=t(nptr).to(torch.int32),
                        edge_ptr=t(eptr).to(torch.int32))


@pytest.mark.parametrize("fn,H,mode,R_", S.LAYERS)
def test_rgin_layer_functions_with_and_without_an_input_gradient(fn, H, mode, R_):
    """The layer functions compute every gradient regardless: x.grad None with x frozen, exact parameter gradients either way."""
    ops = _ops()
    c = S.layer_case(fn, H, mode, R_)
    g = _batched_graph(c.batch)
    sw = dict(MLP_BWD_FUSED_MIN_ROWS=0, WIDE_LAYER_MAX_ROWS=0) if fn == "chain" else {}     # (chain: every batch counts as a large one)
    with switches(**sw):
        iset = g.row_index(_dev(c.et), R_, True, closing_hint=(H, c.dtype))
        ix = iset.index
        assert ix.num_aux_f > 0 and ix.num_aux_b > 0                                        # the dummy nodes: hubs on both sides
        ok = getattr(ops, "rgin_layer_%s_ok" % fn)
        run = getattr(ops, "rgin_layer_" + fn)
        want_tag = {"f32": "rows_wgrad_multi", "small": "rows_wgrad_multi", "wide": "rows_wgrad_multi", "chain": "chain_combine"}[fn]

        def call(t):
            lin = [types.SimpleNamespace(weight=t["mlp.%d.weight" % i], bias=t["mlp.%d.bias" % i]) for i in (0, 2)]
            args = (t["x"], t["weight"], t["loop_weight"], t["bias"], lin)
            with ops.f32_exact(False):
                # (the chain function's predicate asks for an x that takes a gradient: it is the caller's gate for that function)
                assert ok(*args, iset) == (fn != "chain" or t["x"].requires_grad), (fn, t["x"].requires_grad)
                if fn == "chain":
                    assert ok(t["x"].detach().requires_grad_(True), *args[1:], iset)
                return run(*args, c.slope, iset)

        def tags(sub, tf, tb, tb_all):
            assert want_tag in tb and Counter(tb) == Counter(tb_all), (sub, tb, tb_all)

        _sweep(c, S.subsets(c.names, "first"), call, tags)


# ---- neighbor_sum ----------------------------------------------------------------------------------------------------------------
_EDGE_INDEX = {}


def _edge_index(key, src, dst, N):
    if key not in _EDGE_INDEX:
        _EDGE_INDEX[key] = _ops().EdgeIndex(_dev(src), _dev(dst), N)
    return _EDGE_INDEX[key]


@pytest.mark.parametrize("H,mode,self_coef", S.NEIGHBOR_SUM)
def test_neighbor_sum(H, mode, self_coef):
    ops = _ops()
    c = S.neighbor_sum_case(H, mode, self_coef)
    ix = _edge_index("neighbor_sum", c.src, c.dst, c.N)
    assert ix.fwd.hub_ids is not None and ix.bwd.hub_ids is not None            # in- and out-lists over HUB_SPLIT

    def call(t):
        return ops.neighbor_sum(t["x"], ix, self_coef=float(self_coef), edge_scale=t["edge_scale"])

    def tags(sub, tf, tb, tb_all):
        assert ("gather_segsum" in tb) == ("x" in sub), (sub, tb)               # the scale's gradient alone: no row sums at all

    _sweep(c, S.subsets(c.names), call, tags)
    # with the scale alone: d s_e = <x[src_e], g[dst_e]> (dn_edge_dot_*), x.grad None
    got = _run(c, ("edge_scale",), call)
    assert got[1]["x"] is None and got[1]["edge_scale"].dtype == torch.float32
    X.assert_bits(got[1]["edge_scale"], S.edge_dot_ref(c), c.what + ": the edge_dot of x[src] and g[dst]")


# ---- rel_agg_transform -----------------------------------------------------------------------------------------------------------
_REL_INDEX = {}


@pytest.mark.parametrize("fin,fout,mode,scaled", S.REL_AGG)
def test_rel_agg_transform(fin, fout, mode, scaled):
    ops = _ops()
    c = S.rel_agg_case(fin, fout, mode, scaled)
    a = c.agg
    if a.square not in _REL_INDEX:
        _REL_INDEX[a.square] = ops.RelIndex(_dev(c.src), _dev(c.dst), _dev(c.et), a.N, a.R)
    ix = _REL_INDEX[a.square]
    scale = _dev(a.scale, torch.float32) if scaled else None

    def call(t):
        return ops.rel_agg_transform(t["x"], t["W"], ix, scale)

    def tags(sub, tf, tb, tb_all):
        assert tf.count("rows_gemm") == 1
        assert tb.count("rows_gemm") == (1 if "x" in sub else 0), (sub, tb)
        # the matrix-core weight gradient at the square width (the any-width launch carries no tag)
        assert tb.count("rows_wgrad") == (1 if ("W" in sub and a.square) else 0), (sub, tb)

    with ops.f32_exact(False):
        assert ops.wgrad_supported(_dev(a.x[:1], c.dtype), _dev(a.g[:1], c.dtype)) == a.square == (fin == 64)
        _sweep(c, S.subsets(c.names), call, tags)


# ---- linear_any ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,fin,fout,mode", S.LINEAR_ANY)
def test_linear_any(rows, fin, fout, mode):
    ops = _ops()
    c = S.linear_any_case(rows, fin, fout, mode)

    def call(t):
        return ops.linear_any(t["x"], t["weight"], t["bias"])

    def tags(sub, tf, tb, tb_all):
        assert tf == ["rows_gemm"] and tb.count("rows_gemm") == (1 if "x" in sub else 0), (sub, tf, tb)

    # (the bias alone: its column sum comes from the launch it shares with the weight gradient)
    _sweep(c, S.subsets(c.names), call, tags)


# ---- si_embed --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,H,mode", S.SI_EMBED)
def test_si_embed(N, H, mode):
    ops = _ops()
    c = S.si_embed_case(N, H, mode)
    keys = [_i32(k) for k in c.key]
    encs = [_dev(e, c.dtype) for e in c.enc]

    def call(t):
        return ops.si_embed(keys[0], encs[0], t["W1"], keys[1], encs[1], t["W2"])

    def tags(sub, tf, tb, tb_all):
        assert tf == ["si_embed"] and tb == ["si_embed_wgrad"] * len(sub), (sub, tb)        # one frozen table: exactly one launch

    _sweep(c, S.subsets(c.names), call, tags)
    assert all(e.grad is None for e in encs)


# ---- dual_agg, dmp_edge_update -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode_op,kind,H,mode", S.DUAL_AGG)
def test_dual_agg(mode_op, kind, H, mode):
    ops = _ops()
    c = S.dual_agg_case(mode_op, kind, H, mode)
    ix = _edge_index(("dual", kind), c.u, c.v, c.N)
    rev, scale = c.rev.to(DEV), _dev(c.scale, torch.float32)

    def call(t):
        assert ops.dual_supported(t["ef"], t["x"])
        return ops.dual_agg(t["ef"], t["x"], ix, rev, scale, mode_op)

    def tags(sub, tf, tb, tb_all):
        assert ("dual_agg_bwd_edge" in tb) == ("ef" in sub) and ("dual_agg_bwd_node" in tb) == ("x" in sub), (sub, tb)

    _sweep(c, S.subsets(c.names), call, tags)
    # one output left out of the loss (its gradient arrives as None), then the other; and all inputs once more
    for used in ((0,), (1,), (0, 1)):
        got = _run(c, c.names, call, used)
        _check(c, c.names, got, used, what="outputs %s in the loss: " % (used,))


@pytest.mark.parametrize("kind,H,mode", S.DMP_EDGE)
def test_dmp_edge_update(kind, H, mode):
    ops = _ops()
    c = S.dmp_edge_case(kind, H, mode)
    ix = _edge_index(("dual", kind), c.u, c.v, c.N)
    ix._dmp_coef = _dev(c.coef, torch.float32)                  # small integers in place of 2 (1 + log2(1 + out-degree))
    rev = c.rev.to(DEV)
    subs = S.subsets(c.names, "singles")
    assert len(subs) == 11

    def call(t):
        return ops.dmp_edge_update(t["p_loop"], t["p_diff"], t["xd"], t["xs"], t["ebias"], ix, rev)

    def tags(sub, tf, tb, tb_all):
        assert tf == ["dual_edge_update"]
        assert ("dual_edge_update_bwd" in tb) == ("p_diff" in sub), (sub, tb)
        assert tb.count("dual_agg") == (2 if ("xd" in sub or "xs" in sub) else 0), (sub, tb)

    try:
        _sweep(c, subs, call, tags)
    finally:
        del ix._dmp_coef


# ---- typed_linear, hgt_pair_expand, hgt_pair_reduce ------------------------------------------------------------------------------
_HGT_INDEX = {}


@pytest.mark.parametrize("kind,graph,mode", S.TYPED)
def test_typed_products(kind, graph, mode):
    ops = _ops()
    c = S.typed_case(kind, graph, mode)
    src, dst, et = c.graph
    if (kind == "typed", graph) not in _HGT_INDEX:
        if kind == "typed":
            _HGT_INDEX[(True, graph)] = ops.TypeIndex(_dev(c.types), c.R)
        else:
            _HGT_INDEX[(False, graph)] = ops.HgtIndex(_dev(S._i64(src)), _dev(S._i64(dst)), _dev(S._i64(et)), c.N, c.R)
    ix = _HGT_INDEX[(kind == "typed", graph)]
    if kind != "typed":
        assert torch.equal(ix.row_dst_l.cpu(), c.row_dst) and torch.equal(ix.row_rel_l.cpu(), c.row_rel)
    types_d = _dev(c.types) if kind == "typed" else None

    def call(t):
        if kind == "typed":
            return ops.typed_linear(t["x"], t["W"], types_d, ix)
        if kind == "expand":
            return ops.hgt_pair_expand(t["q"], t["W"], ix)
        return ops.hgt_pair_reduce(t["U"], t["W"], ix)

    def tags(sub, tf, tb, tb_all):
        assert tf.count("rows_gemm") == 1 and tb.count("rows_gemm") == (1 if c.rows_name in sub else 0), (sub, tf, tb)

    _sweep(c, S.subsets(c.names), call, tags)


# ---- batchnorm_rows --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,C,mode", S.BATCHNORM)
def test_batchnorm_rows_with_unused_statistics_outputs(N, C, mode):
    """Only y feeds the loss: the statistics outputs' gradients arrive as None (set_materialize_grads(False)).  Compared within the
    bound of test_batch_norm_rows_matches_torch (tests/test_gpu_kernels.py); the statistics, exact at a power-of-two row count, within its
    bound too."""
    ops = _ops()
    c = S.batchnorm_case(N, C, mode)
    bf = c.dtype == torch.bfloat16
    tol = dict(rtol=2e-2, atol=6e-2) if bf else dict(rtol=2e-4, atol=2e-4)
    gt = dict(rtol=3e-2, atol=0.15) if bf else dict(rtol=1e-3, atol=1e-3)
    pt = dict(rtol=3e-2 if bf else 1e-3, atol=(0.5 if bf else 1e-3) * max(1.0, N ** 0.5 / 10))
    bt = dict(rtol=3e-2 if bf else 1e-4, atol=(0.5 if bf else 1e-3) * max(1.0, N ** 0.5 / 10))
    mean, var = c.stats()
    for sub in S.run_order([c.names, ("x",), ("weight", "bias"), ("weight",), ("bias",), ("x", "weight")]):
        leaves = {k: _dev(v, c.dtype).requires_grad_(k in sub) for k, v in c.ins.items()}
        y, m, v = ops.batch_norm_rows(leaves["x"], leaves["weight"], leaves["bias"], c.EPS)
        assert not m.requires_grad and not v.requires_grad
        y.backward(_dev(c.coefs[0], c.dtype))
        (ref_y,), ref = c.run(sub)
        torch.testing.assert_close(m.cpu().double(), mean, rtol=1e-5, atol=1e-4)
        torch.testing.assert_close(v.cpu().double(), var, rtol=2e-4, atol=1e-5)
        torch.testing.assert_close(y.detach().cpu().double(), ref_y, **tol)
        for k, t in (("x", gt), ("weight", pt), ("bias", bt)):
            if k not in sub:
                assert leaves[k].grad is None, (sub, k)
            else:
                assert leaves[k].grad.dtype == c.dtype and leaves[k].grad.shape == leaves[k].shape
                torch.testing.assert_close(leaves[k].grad.cpu().double(), ref[k], **t)
