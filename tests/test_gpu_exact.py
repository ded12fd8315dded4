"""Bit-exact parity of the RGIN layer paths, their gradients and the kernels round 6 changed, on operands where the arithmetic is exact
(tests/exact_ref.py): integer rows with few nonzeros, signed-permutation weights, small-integer biases, upstream gradients in {-1, 0, 1}.
Whatever the summation order, split-K chunking, tile split or storage points of a path, its output, input gradient and every parameter
gradient must then equal the float64 reference rounded once to the path's dtype -- a dropped edge, a chunk one row short or a transposed
tile changes bits here where the tolerance tests of the same paths (relative L2 of 5e-3 .. 0.12) let it pass.  Every test checks its
premise on absolute values first (exact_ref.check_premise) and the path it took (ops.KernelTimer tags)."""
import os
import time
from contextlib import contextmanager

import numpy as np
import pytest
import torch
import torch.nn as nn

import exact_ref as X
from oracle import layers as OL

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FUZZ_SECONDS = float(os.environ.get("DN_EXACT_FUZZ_SECONDS", "15"))


@contextmanager
def switches(**kw):
    """Set ops module switches (read at call time) and restore them whatever happens."""
    from dummynode4graphlearning_amd import ops
    old = {k: getattr(ops, k) for k in kw}
    try:
        for k, v in kw.items():
            setattr(ops, k, v)
        yield
    finally:
        for k, v in old.items():
            setattr(ops, k, v)


def _t(a):
    return torch.as_tensor(np.asarray(a, dtype=np.int64), device=DEV)


def _graph(batch, with_ptrs=True):
    from dummynode4graphlearning_amd import BatchedGraph
    src, dst, et, nptr, eptr = batch
    N = int(nptr[-1])
    if not with_ptrs:
        return BatchedGraph(_t(src), _t(dst), N)
    return BatchedGraph(_t(src), _t(dst), N, _t(np.diff(nptr)), _t(np.diff(eptr)), node_ptr=_t(nptr).to(torch.int32),
                        edge_ptr=_t(eptr).to(torch.int32))


class Case:
    """One exact RGIN layer problem: batch, float64 parameters, input rows, upstream gradient; the reference on the GPU in float64."""

    def __init__(self, seed, batch, H, R, dtype, mlp=2, self_loop=True, regularizer="basis", num_bases=-1, act="relu", s=1, nnz=2,
                 max_exp=0, zero_rows=0.25, param_limit=None, coef_rows=1.0):
        rng = np.random.default_rng(seed)
        self.batch, self.H, self.R, self.dtype = batch, H, R, dtype
        self.kw = dict(regularizer=regularizer, num_bases=num_bases, num_mlp_layers=mlp)
        self.act, self.slope = act, (0.25 if act == "leaky_relu" else 0.0)
        self.self_loop = self_loop
        src, dst, et, nptr, eptr = batch
        N = int(nptr[-1])
        self.N = N
        self.p = {k: v.to(DEV) for k, v in X.layer_params(rng, H, R, mlp, self_loop, regularizer, num_bases, s).items()}
        split = dtype == torch.float32
        x = X.split_rows(rng, N, H, nnz) if split else X.sparse_rows(rng, N, H, nnz, max_exp)
        x[torch.from_numpy(rng.random(N) < zero_rows)] = 0.0       # rows whose pre-activations are bias sums: ties at 0
        self.x = x.to(DEV)
        coef = X.tri_coef(rng, N, H)
        coef[torch.from_numpy(rng.random(N) >= coef_rows)] = 0.0  # (sparse upstream rows keep 1/16-quantum gradients within 256 quanta)
        self.coef = coef.to(DEV)
        self.src, self.dst, self.et = _t(src), _t(dst), _t(et)
        self.graph_of_row = np.repeat(np.arange(len(nptr) - 1), np.diff(nptr))
        # the reference (float64; exact on these operands)
        xr = X.leaf(self.x, DEV)
        pr = {k: X.leaf(v, DEV) for k, v in self.p.items()}
        st = {}
        out = X.rgin_ref(xr, self.src, self.dst, self.et, pr, R, act=act, slope=self.slope, stages=st, **self.kw)
        out.backward(self.coef)
        self.ref = (out.detach(), xr.grad, {k: v.grad for k, v in pr.items()})
        # the premise, on absolute values, in quanta of the terms each stage sums (forward: the operands and stages; backward: the
        # upstream gradient and every gradient reaching a stage -- 1/16 behind two leaky masks)
        q_f = X.quantum(self.x, *self.p.values(), *(v for v in st.values()))
        q_b = X.quantum(self.coef, *(v.grad for v in st.values() if v.grad is not None))
        b = X.layer_bounds(self.x, self.src, self.dst, self.et, self.p, R, self.coef, **self.kw)
        if param_limit is not None and float(b["g:weight"].abs().max()) > param_limit * q_b:
            raise X.PremiseError("stage g:weight reaches %g (limit %g)" % (float(b["g:weight"].abs().max()), param_limit * q_b))
        X.check_premise(b, "f32" if split else "bf16", q_fwd=q_f, q_bwd=q_b)
        if split:                                                # bf16 split: the wide operand <= 16 bits, the narrow one <= 8
            # (the collapsed relations' pre-aggregated rows enter products too: sums of source rows forward, sums of the gradient rows
            #  reaching h backward -- a dummy node's 60 summed gradients easily hold more than 8 bits)
            gh, kf, kb = st["h"].grad, self.dst * R + self.et, self.src * R + self.et
            agg_f = self.x.new_zeros(N * R, H).index_add(0, kf, self.x[self.src])          # per (destination, relation)
            agg_b = gh.new_zeros(N * R, H).index_add(0, kb, gh[self.dst])                  # per (source, relation)
            wide = [self.x, agg_f] + [st[k] for k in st if k in ("h", "a0")]
            narrow = [st[k].grad for k in st if st[k].grad is not None] + [self.coef, agg_b]
            for t in wide:
                if X.sig_bits(t) > 16:
                    raise X.PremiseError("a split product's wide operand holds %d significant bits" % X.sig_bits(t))
            for t in narrow:
                if X.sig_bits(t) > 8:
                    raise X.PremiseError("a split product's narrow operand holds %d significant bits" % X.sig_bits(t))
        self.ties = int((st["z0"] == 0).sum()) if "z0" in st else int((st["h"] == 0).sum())

    def layer(self):
        from dummynode4graphlearning_amd.subgraph_isomorphism import RGINLayer
        layer = RGINLayer(self.H, self.H, num_rels=self.R, self_loop=self.self_loop, act_func=self.act, **self.kw)
        for m in layer.modules():
            if isinstance(m, nn.LeakyReLU):
                m.negative_slope = 0.25
        layer = layer.to(DEV).to(self.dtype)
        X.load_params(layer, self.p)
        return layer

    def run(self, layer, g):
        """-> (kernel tags, output, input gradient, {name: gradient})"""
        from dummynode4graphlearning_amd import ops
        for q in layer.parameters():
            q.grad = None
        x = self.x.to(self.dtype).clone().requires_grad_(True)
        with ops.KernelTimer() as timer:
            out, _ = layer(g, x, self.et)
            out.backward(self.coef.to(self.dtype))
        return [r[0] for r in timer.records], out, x.grad, {k: v.grad for k, v in layer.named_parameters()}

    def check(self, got, what=""):
        _, out, gx, gp = got
        ref_out, ref_gx, ref_gp = self.ref
        X.assert_bits(out, ref_out, what + "output", graph=self.graph_of_row)
        X.assert_bits(gx, ref_gx, what + "input gradient", graph=self.graph_of_row)
        for k, v in gp.items():
            rel = np.arange(v.shape[0]) if k == "weight" else None
            X.assert_bits(v, ref_gp[k], what + "gradient of " + k, rel=rel)


def _config3_like(rng, G=48, R=8):
    """config-3-shaped graphs, one without edges among them and single-node graphs"""
    a = X.si_batch(rng, G, R, 49, 2.1)
    empty = X.si_batch(rng, 1, R, 5, 0.0, dummy=False)                    # nodes, no edges
    single = X.si_batch(rng, 3, R, 1, 0.0, dummy=False)                   # three one-node graphs
    b = X.si_batch(rng, G // 2, R, 40, 2.0)
    return X.concat_batches(a, empty, single, b)


def _synthetic(raw, G=None):
    from dummynode4graphlearning_amd import transforms
    keys = ("node_ptr", "edge_ptr", "src", "dst", "node_id", "node_label", "edge_id", "edge_label")
    aug = transforms.dummy_augment_si(*(torch.from_numpy(raw[k]).to(DEV) for k in keys), raw["max_nv"], raw["max_nvl"], raw["max_ne"],
                                      raw["max_nel"])
    return tuple(aug[k].long().cpu().numpy() for k in ("src", "dst", "edge_label", "node_ptr", "edge_ptr"))


# ---- A. layer paths -------------------------------------------------------------------------------------------------------------
def test_premise_oracle_pin_on_gpu():
    """The per-relation reference equals oracle.layers.rgin_layer bit for bit (output and every gradient) on a small exact batch."""
    rng = np.random.default_rng(1)
    batch = X.si_batch(rng, 6, 5, 9, 2.0)
    for act in ("relu", "leaky_relu"):
        c = Case(11, batch, 64, 5, torch.bfloat16, act=act, coef_rows=0.3)
        xr = X.leaf(c.x.cpu())
        pr = {k: X.leaf(v.cpu()) for k, v in c.p.items()}
        old = OL.LEAKY_RELU_A
        OL.LEAKY_RELU_A = 0.25                               # the slope the exact tests give the layer's LeakyReLU modules
        try:
            out = OL.rgin_layer(xr, c.src.cpu(), c.dst.cpu(), c.et.cpu(), pr, num_rels=5, act=act,
                                **{k: c.kw[k] for k in ("regularizer", "num_bases")})
        finally:
            OL.LEAKY_RELU_A = old
        out.backward(c.coef.cpu())
        _pinned(c, out, xr, pr)


def _pinned(c, out, xr, pr):
    assert torch.equal(out.detach(), c.ref[0].cpu()) and torch.equal(xr.grad, c.ref[1].cpu()), c.act
    for k in pr:
        assert torch.equal(pr[k].grad, c.ref[2][k].cpu()), k


@pytest.mark.parametrize("sw", [{}, {"LAYER_GRAPHS_ENABLED": False}, {"LAYER_SMALL_ENABLED": False}, {"CONV_GRAPHS_ENABLED": False}])
@pytest.mark.parametrize("act", ["relu", "leaky_relu"])
def test_bf16_h64_whole_graph_path(sw, act):
    rng = np.random.default_rng(3)
    c = Case(5, _config3_like(rng), 64, 8, torch.bfloat16, act=act, nnz=3, coef_rows=1.0 if act == "relu" else 0.1)
    assert c.ties > 0 and int(np.diff(c.batch[4])[48]) == 0 and int(np.diff(c.batch[3])[48]) > 1     # the graph without edges
    with switches(**sw):
        g = _graph(c.batch)
        got = c.run(c.layer(), g)
        ix = g.row_index(c.et, c.R, True).parts[0][2]
    tags = [t for t in got[0] if t != "gather_segsum"]     # (aux rows of graphs without the dummy node: one gather launch)
    if not sw:
        assert tags == ["layer_graphs_fwd", "layer_graphs_bwd", "rows_wgrad_multi"], tags
    elif "LAYER_GRAPHS_ENABLED" in sw:
        assert sorted(tags) == ["conv_graphs", "conv_graphs", "rows_chain2", "rows_chain2", "rows_wgrad_multi"], tags
    elif "LAYER_SMALL_ENABLED" in sw:
        assert tags.count("conv_graphs") == 2 and tags.count("rows_wgrad") == 3 and "rows_wgrad_multi" not in tags, tags
    else:
        assert "conv_graphs" not in tags and "layer_graphs_fwd" not in tags, tags
    if "conv_graphs" in tags or "layer_graphs_fwd" in tags:
        assert int(ix._cg_err[0].item()) == 0
    c.check(got)


@pytest.mark.parametrize("shape,whole", [
    ((64, [65] * 15 + [49]), True),                      # 64 nodes, 1,024 edges, 16 relations: the launch's limits, 1-edge tails
    ((65, [65] * 15 + [49]), False),                     # 65 nodes
    ((64, [65] * 15 + [50]), False),                     # 1,025 edges
    ((64, [60] * 17), False),                            # 17 relations
])
def test_bf16_h64_at_the_whole_graph_limits(shape, whole):
    rng = np.random.default_rng(7)
    nodes, sizes = shape
    R = len(sizes)
    lim = X.limit_graph(rng, nodes, sizes)
    small = X.si_batch(rng, 5, R, 12, 2.0, dummy=False)
    c = Case(9, X.concat_batches(small, lim, small), 64, R, torch.bfloat16, nnz=1, s=1)
    g = _graph(c.batch)
    got = c.run(c.layer(), g)
    assert ("layer_graphs_fwd" in got[0]) == whole, got[0]
    if whole:
        assert int(g.row_index(c.et, R, True).parts[0][2]._cg_err[0].item()) == 0
    c.check(got)


def test_bf16_h128_row_factorised():
    rng = np.random.default_rng(4)
    c = Case(6, _config3_like(rng), 128, 8, torch.bfloat16, nnz=4)
    got = c.run(c.layer(), _graph(c.batch))
    assert "layer_graphs_fwd" not in got[0] and "rows_transform:conv" in got[0], got[0]
    c.check(got)


_C5 = {}


def _config5(G):
    if G not in _C5:
        from dummynode4graphlearning_amd import synthetic
        _C5[G] = _synthetic(synthetic.config5(seed=5, graphs=G))
    return _C5[G]


@pytest.mark.parametrize("wide", [True, False])
def test_bf16_h256_wide_function_against_separate_functions(wide):
    from dummynode4graphlearning_amd import ops
    b = _config5(2048)
    c = Case(12, b, 256, 16, torch.bfloat16, nnz=8, s=2)
    g = _graph(b)
    ix = g.row_index(c.et, 16, True, closing_hint=(256, torch.bfloat16)).parts[0][2]
    total = ix.num_rows + 2 * c.N
    with switches(WIDE_LAYER_MAX_ROWS=total if wide else total - 1):
        got = c.run(c.layer(), g)
    assert (got[0].count("rows_wgrad_multi") == 1) == wide and ("rows_wgrad" in got[0]) != wide, got[0]
    assert "rows_close" in got[0] or "rows_selfsum" in got[0], got[0]
    c.check(got)


# (tags present / absent, fold absorbed, sweep order, chunked multi-graph tiles) of each setting on the sweep-sized batch
_SWITCH_PATHS = [
    ({}, {"rows_close", "rows_wgrad_multi"}, {"rows_selfsum", "fold_tail", "gather_segsum"}, True, True, False),
    ({"SWEEP_ENABLED": False}, {"rows_close", "rows_wgrad_multi"}, {"rows_selfsum", "fold_tail"}, True, False, False),
    ({"SELFSUM_ENABLED": False}, {"rows_wgrad", "gather_segsum"}, {"rows_close", "rows_selfsum", "rows_wgrad_multi"}, None, None, None),
    ({"CLOSE_RING_ENABLED": False}, {"rows_selfsum", "overflow_rows_add", "fold_tail", "rows_wgrad_multi"}, {"rows_close"}, False, True,
     False),
    ({"CLOSE_SINGLE_ENABLED": False}, {"rows_close", "rows_wgrad_multi"}, {"rows_selfsum", "fold_tail"}, True, True, True),
    # (every config-5 graph fits one tile: without the chunked form the path is the default's -- graphs over 32 nodes: the
    #  PROTEINS-shaped test)
    ({"CLOSE_MULTI_ENABLED": False}, {"rows_close", "rows_wgrad_multi"}, {"rows_selfsum", "fold_tail"}, True, True, False),
    ({"FOLD_ENABLED": False}, {"rows_close", "gather_segsum", "rows_wgrad_multi"}, {"fold_tail"}, None, None, None),
    ({"CLOSE_AGG_ENABLED": False}, {"rows_close", "fold_tail", "rows_wgrad_multi"}, {"rows_selfsum"}, False, True, False),
]


@pytest.mark.parametrize("sw,present,absent,absorbed,sweep,multi", _SWITCH_PATHS)
def test_bf16_h256_switches_on_a_sweep_sized_batch(sw, present, absent, absorbed, sweep, multi):
    from dummynode4graphlearning_amd import ops
    b = _config5(4608)
    c = Case(13, b, 256, 16, torch.bfloat16, nnz=8, s=2)
    with switches(**sw):
        g = _graph(b)
        got = c.run(c.layer(), g)
        ix = g.row_index(c.et, 16, True).parts[0][2]
        assert ops._sweep_wanted(ix) == ("SWEEP_ENABLED" not in sw)
    tags = set(got[0])
    assert present <= tags and not (absent & tags), (sw, sorted(tags))
    fold = ix._fold.get("f")
    if absorbed is None:
        assert "FOLD_ENABLED" not in sw or fold is None
    else:
        assert fold is not None and (fold.graph_tiles is not None) == absorbed
        assert (getattr(fold, "sweep_tiles", None) is not None) == sweep and (getattr(fold, "multi", None) is not None) == multi
    c.check(got, "%s: " % sw)


def test_bf16_h256_proteins_shaped():
    """PROTEINS-shaped batch: graphs over 32 nodes (the fold in the chunked multi-graph tiles, builder verdict 2), one graph of 1,120 + 600
    edges (over 1,024: the graph-local builder's second launch), and a hub of 37 rows (more than SELFSUM_SLOTS, at most
    OVERFLOW_INSIDE_MAX_LIST) -- on the closing units, then on the slot tables with the hub's rows walked inside the launch and, below
    OVERFLOW_INSIDE_MAX_ROWS / _MAX_LIST, by the overflow launch."""
    from dummynode4graphlearning_amd import ops, synthetic
    b = _synthetic(synthetic.proteins_si(seed=2, graphs=600))
    assert np.diff(b[3]).max() > 32
    rng = np.random.default_rng(8)
    big = X.limit_graph(rng, 300, [80] * 14 + [0, 0])                 # 1,120 edges (+ none to a dummy)
    hub = X.limit_graph(rng, 40, [ops.SELFSUM_SLOTS + 3] * 4 + [0] * 12)
    hub = (hub[0], np.zeros_like(hub[1]), hub[2], hub[3], hub[4])       # every edge into node 0: 36 rows + its self loop
    b = X.concat_batches(b, big, hub)
    c = Case(14, b, 256, 16, torch.bfloat16, nnz=4, s=1)
    longest = 4 * (ops.SELFSUM_SLOTS + 3) + 1                          # the hub's list: its 36 rows and its self loop
    for sw, overflow in (({}, None), ({"CLOSE_MULTI_ENABLED": False}, None), ({"CLOSE_RING_ENABLED": False}, False),
                         ({"CLOSE_RING_ENABLED": False, "OVERFLOW_INSIDE_MAX_ROWS": 0}, True),
                         ({"CLOSE_RING_ENABLED": False, "OVERFLOW_INSIDE_MAX_LIST": longest - 1}, True)):
        with switches(**sw):
            g = _graph(b)
            got = c.run(c.layer(), g)
            ix = g.row_index(c.et, 16, True).parts[0][2]
        tags = set(got[0])
        assert ix.built_by == "local" and ix.max_graph[1] > 1024, (ix.built_by, ix.max_graph)
        assert ix._absorb["f"][2] == 2 and ix._absorb["b"][2] == 2, {d: v[2] for d, v in ix._absorb.items()}
        if overflow is None:
            assert "rows_close" in tags and "rows_selfsum" not in tags, (sw, sorted(tags))
            fold = ix._fold["f"]
            assert (getattr(fold, "multi", None) is not None) == ("CLOSE_MULTI_ENABLED" not in sw), sw
        else:
            assert "rows_selfsum" in tags and "rows_close" not in tags, (sw, sorted(tags))
            assert ix._slots["f"][1][-1] in (None, longest)                   # the hub: the longest forward list
            assert ("overflow_rows_add" in tags) == overflow, (sw, sorted(tags))
        c.check(got, "%s: " % sw)


@pytest.mark.parametrize("H", [64, 128])
@pytest.mark.parametrize("sw", [{}, {"CHAIN2_F32_ENABLED": False}, {"LAYER_F32_ENABLED": False}, "exact"])
def test_fp32_layer_function(H, sw):
    from dummynode4graphlearning_amd import ops
    rng = np.random.default_rng(20 + H)
    c = Case(15, _config3_like(rng, G=32), H, 8, torch.float32, nnz=3)
    if sw == "exact":
        with ops.f32_exact(True):
            got = c.run(c.layer(), _graph(c.batch))
    else:
        with switches(**sw):
            got = c.run(c.layer(), _graph(c.batch))
    multi = sw != "exact" and "LAYER_F32_ENABLED" not in (sw if isinstance(sw, dict) else {})
    assert (got[0].count("rows_wgrad_multi") == 1) == multi, got[0]
    c.check(got)


def test_fp32_h256_separate_functions():
    rng = np.random.default_rng(30)
    c = Case(16, _config3_like(rng, G=24), 256, 8, torch.float32, nnz=3)
    got = c.run(c.layer(), _graph(c.batch))
    assert "rows_wgrad_multi" not in got[0]
    c.check(got)


def test_fp32_rep_net_residual_in_the_launches():
    """RGINRepNet, three layers, rep_residual: x + layer(x) carried in the fp32 layer function's own launches."""
    from dummynode4graphlearning_amd.subgraph_isomorphism import RGINRepNet
    from dummynode4graphlearning_amd import ops
    rng = np.random.default_rng(31)
    batch = X.si_batch(rng, 24, 8, 30, 2.0, dummy=False)       # (no hub: the gradients three residual layers sum stay within 8 bits)
    H, R, L = 64, 8, 3
    g = _graph(batch)
    src, dst, et = _t(batch[0]), _t(batch[1]), _t(batch[2])
    g.edata["label"] = et
    N = int(batch[3][-1])
    ps = [{k: v.to(DEV) for k, v in X.layer_params(rng, H, R, 2, True).items()} for _ in range(L)]
    x0 = X.split_rows(rng, N, H, 1, scale=1).to(DEV, torch.float32)
    coef = (X.tri_coef(rng, N, H) * torch.from_numpy(rng.random((N, 1)) < 0.5)).to(DEV)
    net = RGINRepNet(H, R, num_layers=L, rep_residual=True).to(DEV)
    for layer, p in zip(net.rgin, ps):
        X.load_params(layer, p)
    # reference and premise: every layer's input <= 16 significant bits, every gradient that meets it <= 8, every stage of every layer
    # below 2^24 on absolute values (with the gradient that actually reaches the layer)
    xr = X.leaf(x0, DEV)
    prs = [{k: X.leaf(v, DEV) for k, v in p.items()} for p in ps]
    h, ins, outs, sts = xr, [], [], []
    for p in prs:
        ins.append(h)
        st = {}
        o = X.rgin_ref(h, src, dst, et, p, R, stages=st)
        o.retain_grad()
        outs.append(o)
        sts.append(st)
        h = h + o
    h.backward(coef)
    for t, o, st, p in zip(ins, outs, sts, ps):
        for w in [t, t.new_zeros(N * R, H).index_add(0, dst * R + et, t[src]), st["h"], st["a0"]]:
            if X.sig_bits(w) > 16:
                raise X.PremiseError("a layer operand holds %d significant bits" % X.sig_bits(w))
        gh = st["h"].grad
        for gt in [o.grad, gh.new_zeros(N * R, H).index_add(0, src * R + et, gh[dst])] + [v.grad for v in st.values() if v.grad is not None]:
            if X.sig_bits(gt) > 8:
                raise X.PremiseError("a gradient operand holds %d significant bits" % X.sig_bits(gt))
        X.check_premise(X.layer_bounds(t.detach(), src, dst, et, p, R, o.grad), "f32")
    x = x0.clone().requires_grad_(True)
    with ops.KernelTimer() as timer:
        out = net(g, x)
        out.backward(coef)
    tags = [r[0] for r in timer.records]
    assert tags.count("rows_wgrad_multi") == L, tags
    X.assert_bits(out, h, "output")
    X.assert_bits(x.grad, xr.grad, "input gradient")
    for i, (layer, p) in enumerate(zip(net.rgin, prs)):
        for k, v in layer.named_parameters():
            X.assert_bits(v.grad, p[k].grad, "layer %d gradient of %s" % (i, k))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("var", [dict(regularizer="bdd", num_bases=4), dict(regularizer="basis", num_bases=3), dict(self_loop=False),
                                 dict(mlp=0), dict(mlp=1), dict(act="leaky_relu")])
def test_layer_variants(var, dtype):
    rng = np.random.default_rng(40)
    batch = _config3_like(rng, G=12 if var.get("num_bases") != 3 else 2)
    lim = X.BF16_LIMIT if (dtype == torch.bfloat16 and var.get("num_bases") == 3) else None   # w_comp's gradient: torch's product of a
    c = Case(17, batch, 64, 8, dtype, nnz=2, param_limit=lim, coef_rows=0.1 if var.get("act") else 1.0,
             **var)                                                                              # stored bf16 dense gradient
    got = c.run(c.layer(), _graph(batch))
    whole = var.get("self_loop", True) and var.get("mlp", 2) == 2        # one autograd function for the whole layer
    if dtype == torch.bfloat16:
        assert ("layer_graphs_fwd" in got[0]) == whole, (var, got[0])
    assert ("rows_wgrad_multi" in got[0]) == whole, (var, got[0])
    c.check(got, "%s: " % var)


@pytest.mark.parametrize("sw", [{"LOCAL_INDEX_ENABLED": False}, {"CONV_INDEX_ENABLED": False}, {}])
def test_index_builders_give_the_same_bits(sw):
    b = _config5(512)
    c = Case(18, b, 256, 16, torch.bfloat16, nnz=8, s=2)
    with switches(**sw):
        g = _graph(b)
        ix = g.row_index(c.et, 16, True, closing_hint=(256, torch.bfloat16)).parts[0][2]
        one_call = bool(ix._units)                          # dn_conv_index_build_i32 returned status 0: both unit streams came with it
        got = c.run(c.layer(), g)
    assert ix.built_by == ("general" if "LOCAL_INDEX_ENABLED" in sw else "local")
    assert one_call == (not sw), (sw, one_call)
    assert got[0].count("rows_wgrad_multi") == 1 and "rows_close" in got[0], got[0]
    c.check(got, "%s: " % sw)


@pytest.mark.parametrize("order", [(64, 256, 128), (128, 256, 64)])
def test_one_index_across_widths_and_dtypes(order):
    """One BatchedGraph and one etype tensor at several widths / dtypes: the index cache ignores the closing hint after its first
    build, so later widths run on what the first one decided.  Every step exact; a repeat on the cached index gives the same bits."""
    rng = np.random.default_rng(50)
    batch = X.concat_batches(_config3_like(rng, G=40, R=16), X.si_batch(rng, 8, 16, 40, 3.0, nmin=33))
    g = _graph(batch)
    et = _t(batch[2])
    for H in order:
        dtype = torch.float32 if H == 128 else torch.bfloat16
        c = Case(19 + H, batch, H, 16, dtype, nnz=2)
        c.et = et
        layer = c.layer()
        got = c.run(layer, g)
        assert got[0].count("rows_wgrad_multi") == 1 and (("layer_graphs_fwd" in got[0]) == (H == 64)), (H, got[0])
        c.check(got, "H=%d %s: " % (H, dtype))
        again = c.run(layer, g)
        for a, b2 in zip(got[1:3], again[1:3]):
            assert torch.equal(a, b2)


# ---- B. kernels -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_linear_any_exact_over_k_and_n(dtype):
    """linear_any on non-square weights: dn_rows_gemm_* through _single_rel_table (fp32: the exact-f32 MFMA product whatever the
    module's fp32 mode, k-steps of 32 below K = 128 and of 128 from it) and dn_rows_wgrad_any_* with its 64-row chunks."""
    from dummynode4graphlearning_amd import ops
    rng = np.random.default_rng(60)
    for K in (1, 31, 32, 33, 127, 128, 129, 200, 255, 256, 257, 300):
        for Nn in (1, 2, 7, 63, 64, 65, 130):
            M = int(rng.choice([1, 15, 16, 63, 64, 65, 127, 128, 129, 3001]))
            x = X.sparse_rows(rng, M, K, nnz=3, max_exp=2)
            w = X.signed_weight(rng, Nn, K, s=2) if K >= 2 else X.small_ints(rng, Nn, K, lo=-1, hi=1)
            bias = X.small_ints(rng, Nn) if (K + Nn) % 2 else None
            g = X.tri_coef(rng, M, Nn)
            X.check_premise(X.linear_bounds(x, w, bias, g), "bf16" if dtype == torch.bfloat16 else "f32")
            xr, wr = X.leaf(x), X.leaf(w)
            br = X.leaf(bias) if bias is not None else None
            ref = torch.nn.functional.linear(xr, wr, br)
            ref.backward(g)
            xd = x.to(DEV, dtype).requires_grad_(True)
            wd = w.to(DEV, dtype).requires_grad_(True)
            bd = bias.to(DEV, dtype).requires_grad_(True) if bias is not None else None
            with ops.KernelTimer() as timer:
                y = ops.linear_any(xd, wd, bd)
                y.backward(g.to(DEV, dtype))
            assert [r[0] for r in timer.records].count("rows_gemm") == 2
            what = "K=%d N=%d M=%d %s: " % (K, Nn, M, dtype)
            X.assert_bits(y, ref, what + "output")
            X.assert_bits(xd.grad, xr.grad, what + "input gradient")
            X.assert_bits(wd.grad, wr.grad, what + "weight gradient")
            if bias is not None:
                X.assert_bits(bd.grad, br.grad, what + "bias gradient")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_rows_gemm_explicit_tables_relation_sizes(dtype):
    """rows_gemm forward and its backward products (rows_gemm on the transposed weights, rows_wgrad_any) through explicit tile / chunk
    tables over relations of 0 .. 3,001 rows."""
    from dummynode4graphlearning_amd import ops
    rng = np.random.default_rng(61)
    sizes = [0, 1, 15, 16, 63, 64, 65, 127, 128, 129, 3001]
    rp = np.concatenate([[0], np.cumsum(sizes)])
    R, P = len(sizes), int(rp[-1])
    rp_d = torch.tensor(rp, dtype=torch.int32, device=DEV)
    tiles = ops.build_row_tables(rp_d, R, P, 64)
    chunks = ops.build_row_tables(rp_d, R, P, 128, want_ptr=True)
    rel = np.repeat(np.arange(R), sizes)
    storage = "bf16" if dtype == torch.bfloat16 else "f32"
    for K, Nn, tw in ((33, 65, False), (129, 7, True), (257, 130, False), (128, 64, True)):
        A = X.sparse_rows(rng, P, K, nnz=2, max_exp=1)
        W = torch.stack([X.signed_weight(rng, Nn, K, 2) if tw else X.signed_weight(rng, K, Nn, 2) for _ in range(R)])
        bias = X.small_ints(rng, R, Nn)
        gY = X.tri_coef(rng, P, Nn)
        for r in range(R):
            a, b_ = int(rp[r]), int(rp[r + 1])
            wk = W[r] if tw else W[r].t()                                # [N, K]: the Linear layout linear_bounds takes
            X.check_premise(X.linear_bounds(A[a:b_], wk, bias[r], gY[a:b_]), storage)
        what = "rows_gemm K=%d N=%d transpose=%s" % (K, Nn, tw)
        Y = ops.rows_gemm(A.to(DEV, dtype), W.to(DEV, dtype), tiles, transpose_w=tw, bias=bias.to(DEV, dtype))
        X.assert_bits(Y, X.per_relation_linear(A, W, rp, transpose_w=tw, bias=bias), what, rel=rel)
        gA = ops.rows_gemm(gY.to(DEV, dtype), W.to(DEV, dtype), tiles, transpose_w=not tw)
        X.assert_bits(gA, X.per_relation_linear(gY, W, rp, transpose_w=not tw), what + " input gradient", rel=rel)
        gW = ops.rows_wgrad_any(A.to(DEV, dtype), gY.to(DEV, dtype), chunks, R)          # [R, K, N]: sum A^T gY per relation
        ref = torch.stack([A[int(rp[r]):int(rp[r + 1])].t() @ gY[int(rp[r]):int(rp[r + 1])] for r in range(R)])
        X.assert_bits(gW, ref, what + " weight gradient", rel=np.arange(R))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_dense_mlp_weight_gradients_where_the_chunk_changes(dtype):
    """The MLP weight gradients through _dense_table: 128-row chunks up to 32,768 rows, 192 from 32,769, ragged tails."""
    from dummynode4graphlearning_amd import ops
    rng = np.random.default_rng(62)
    H = 64
    for M in (1, 127, 129, 32767, 32768, 32769, 40001):
        x = X.sparse_rows(rng, M, H, nnz=1, max_exp=0)
        w = X.signed_weight(rng, H, H, 1)
        g = X.tri_coef(rng, M, H)
        X.check_premise(X.linear_bounds(x, w, torch.zeros(H, dtype=torch.float64), g), "bf16" if dtype == torch.bfloat16 else "f32")
        xr, wr, br = X.leaf(x), X.leaf(w), X.leaf(torch.zeros(H, dtype=torch.float64))
        ref = torch.nn.functional.linear(xr, wr, br)
        ref.backward(g)
        xd = x.to(DEV, dtype).requires_grad_(True)
        wd = w.to(DEV, dtype).requires_grad_(True)
        bd = torch.zeros(H, dtype=dtype, device=DEV, requires_grad=True)
        y = ops.linear_act(xd, wd, bd, exact=True if dtype == torch.float32 else None)
        y.backward(g.to(DEV, dtype))
        assert ops._dense_table(M, xd.device)[1][2] == -(-M // max(128, min(ops.WGRAD_CHUNK_CAP, -(-M // 256 // 64) * 64)))
        X.assert_bits(y, ref, "M=%d output" % M)
        X.assert_bits(wd.grad, wr.grad, "M=%d weight gradient" % M)
        X.assert_bits(bd.grad, br.grad, "M=%d bias gradient" % M)
        X.assert_bits(xd.grad, xr.grad, "M=%d input gradient" % M)


@pytest.mark.parametrize("H", [64, 128, 256, 32])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_edge_dot_and_neighbor_max_exact(H, dtype):
    from dummynode4graphlearning_amd import ops
    rng = np.random.default_rng(70 + H)
    # segment lengths 0 .. 9 around the unroll of 4, integer ties everywhere
    lens = np.tile(np.arange(10), 6)
    N = len(lens)
    dst = np.repeat(np.arange(N), lens)
    src = rng.integers(0, N, size=len(dst))
    x = X.small_ints(rng, N, H, lo=-2, hi=2)
    coef = X.tri_coef(rng, N, H)
    b = X.small_ints(rng, N, H, lo=-3, hi=3)
    # premise: the max picks a stored value; per-source gradient sums and the edge dots on absolute values within the limits
    if (float(torch.zeros(N, H, dtype=torch.float64).index_add(0, torch.from_numpy(src), coef.abs()[torch.from_numpy(dst)]).max())
            > X.BF16_LIMIT or float((x.abs()[src] * b.abs()[dst]).sum(1).max()) >= X.F32_LIMIT):
        raise X.PremiseError("neighbor_max / edge_dot operands not exact")
    g = _graph((src, dst, np.zeros_like(src), np.array([0, N]), np.array([0, len(src)])))
    ix = g.edge_index()
    # first maximum in slot order (the in-edge list of ix), 0 for isolated nodes
    ref = torch.zeros(N, H, dtype=torch.float64)
    arg = torch.full((N, H), -1, dtype=torch.long)
    sbd, ip = ix.src_by_dst.long().cpu(), ix.in_ptr.long().cpu()
    for v in range(N):
        a, e = int(ip[v]), int(ip[v + 1])
        if e > a:
            vals = x[sbd[a:e]]
            m = vals.max(0).values
            ref[v] = m
            arg[v] = sbd[a:e][(vals == m).float().argmax(0)]
    gref = torch.zeros(N, H, dtype=torch.float64)
    has = arg >= 0
    cols = torch.arange(H).expand(N, H)
    gref.index_put_((arg[has], cols[has]), coef[has], accumulate=True)
    big = torch.zeros(N * H + 2, dtype=dtype, device=DEV)
    for name, xin in (("contiguous", x.to(DEV, dtype)), ("4-byte-offset view", big[2 if dtype == torch.bfloat16 else 1:][:N * H].view(N, H))):
        if name != "contiguous":
            xin.copy_(x.to(DEV, dtype))
        xd = xin.detach().requires_grad_(True)                        # (detach keeps the view's storage offset)
        out = ops.neighbor_max(xd, ix)
        X.assert_bits(out, ref, "neighbor_max H=%d %s" % (H, name))
        out.backward(coef.to(DEV, dtype))
        X.assert_bits(xd.grad, gref, "neighbor_max gradient H=%d %s" % (H, name))
        ia, ib = _t(src).to(torch.int32), _t(dst).to(torch.int32)
        d = ops.edge_dot(xd.detach(), ia, b.to(DEV, dtype), ib)
        X.assert_bits(d, (x[src] * b[dst]).sum(1), "edge_dot H=%d %s" % (H, name))


def _gin_batch(rng, G, n, reps):
    """G graphs of n nodes and 120 random edges, graph 0 with `reps` parallel edges 3 -> 7 on top."""
    src, dst = [], []
    for gi in range(G):
        src += list(gi * n + rng.integers(0, n, size=120))
        dst += list(gi * n + rng.integers(0, n, size=120))
    src += [3] * reps
    dst += [7] * reps
    order = np.argsort(np.asarray(src) // n, kind="stable")
    src, dst = np.asarray(src)[order], np.asarray(dst)[order]
    return src, dst, np.zeros_like(src), np.arange(G + 1) * n, np.concatenate([[0], np.cumsum(np.bincount(src // n, minlength=G))])


@pytest.mark.parametrize("N,reps", [(1000, 256), (5000, 256), (5000, 257)])
def test_neighbor_sum_tile_plan_and_parallel_edges(N, reps):
    """GIN aggregation, both directions: fp32 integers of 20 significant bits (all three bf16 planes of the tile sum) with 256 parallel
    edges on one pair (the tile plan keeps them) or 257 (its `bad` flag: the batch falls back to the plain gather), N on both sides
    of TILE_SUM_MIN_ROWS (4,096); and the bf16 gather."""
    from dummynode4graphlearning_amd import ops
    rng = np.random.default_rng(80 + N + reps)
    H, n = 64, 50
    batch = _gin_batch(rng, N // n, n, reps)
    src, dst = batch[0], batch[1]
    mag = rng.integers(1 << 19, 1 << 20, size=(N, H)).astype(np.float64)
    mag[[3, 7]] = rng.integers(1, 1 << 15, size=(2, H))               # the parallel pair's ends: 257 x < 2^24 both ways
    x = torch.from_numpy(np.where(rng.random((N, H)) < 0.5, -mag, mag))
    gy = torch.from_numpy(np.where(rng.random((N, H)) < 0.5, -mag, mag))
    assert X.sig_bits(x) == 20
    s_, d_ = torch.from_numpy(src), torch.from_numpy(dst)
    for t, a, b_ in ((x, s_, d_), (gy, d_, s_)):
        if float(t.abs().index_add(0, b_, t.abs()[a]).max()) >= X.F32_LIMIT:
            raise X.PremiseError("neighbor_sum operands not exact")
    tile = N >= ops.TILE_SUM_MIN_ROWS
    with switches(TILE_SUM_ENABLED=True):
        ix = _graph(batch).edge_index()
        xd = x.to(DEV, torch.float32).requires_grad_(True)
        with ops.KernelTimer() as timer:
            out = ops.neighbor_sum(xd, ix, self_coef=1.0)
            out.backward(gy.to(DEV, torch.float32))
        kept = tile and ix.tile_plan() is not None         # (below TILE_SUM_MIN_ROWS the plan is never asked for)
    tags = [r[0] for r in timer.records]
    assert kept == (tile and reps <= 256), (N, reps, kept)
    assert tags.count("graph_tile_sum") == (2 if kept else 1 if tile else 0), tags
    X.assert_bits(out, x.clone().index_add(0, d_, x[s_]), "neighbor_sum fp32 N=%d reps=%d" % (N, reps))
    X.assert_bits(xd.grad, gy.clone().index_add(0, s_, gy[d_]), "neighbor_sum fp32 backward N=%d reps=%d" % (N, reps))
    # bf16: the hub pass (in-degree over HUB_SPLIT) keeps its 64-entry chunk partials and the hub sum as bf16 rows -- storage points by
    # design, exact while every partial stays within 256: at most 200 parallel edges of +-1 here (257 would round a partial)
    keep = np.ones(len(src), dtype=bool)
    keep[np.nonzero((src == 3) & (dst == 7))[0][200:]] = False
    sb, db = src[keep], dst[keep]
    nptr = batch[3]
    eb = np.concatenate([[0], np.cumsum(np.bincount(sb // n, minlength=N // n))])
    xb = X.small_ints(rng, N, H, lo=-1, hi=1)
    sb_, db_ = torch.from_numpy(sb), torch.from_numpy(db)
    if float(xb.abs().index_add(0, db_, xb.abs()[sb_]).max()) > X.BF16_LIMIT:
        raise X.PremiseError("bf16 neighbor_sum operands not exact")
    outb = ops.neighbor_sum(xb.to(DEV, torch.bfloat16), _graph((sb, db, np.zeros_like(sb), nptr, eb)).edge_index(), self_coef=1.0)
    X.assert_bits(outb, xb.clone().index_add(0, db_, xb[sb_]), "neighbor_sum bf16 N=%d" % N)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_segment_reduce_exact(dtype):
    from dummynode4graphlearning_amd import ops
    rng = np.random.default_rng(90)
    lens = np.array([0, 1, 2, 3, 4, 5, 7, 9, 31, 64, 65, 200, 0, 1])
    ptr_ = np.concatenate([[0], np.cumsum(lens)])
    N, H = int(ptr_[-1]), 48
    x = X.small_ints(rng, N, H, lo=-1, hi=1)
    segs = [x[ptr_[i]:ptr_[i + 1]] for i in range(len(lens))]
    if max(float(s.abs().sum(0).max()) if len(s) else 0.0 for s in segs) > X.BF16_LIMIT:
        raise X.PremiseError("segment sums not exact in bf16")
    xd = x.to(DEV, dtype)
    p = torch.tensor(ptr_, dtype=torch.int32, device=DEV)
    s_ref = torch.stack([s.sum(0) if len(s) else torch.zeros(H, dtype=torch.float64) for s in segs])
    X.assert_bits(ops.segment_reduce(xd, p, "sum"), s_ref, "segment sum")
    m_ref = torch.stack([s.max(0).values if len(s) else torch.zeros(H, dtype=torch.float64) for s in segs])
    X.assert_bits(ops.segment_reduce(xd, p, "max"), m_ref, "segment max")
    mean = ops.segment_reduce(xd, p, "mean").double().cpu()
    want = (s_ref / torch.from_numpy(np.maximum(lens, 1)).double().view(-1, 1)).to(dtype).double()
    ulp = (want.abs().clamp(min=2.0 ** -126).log2().floor() - (7 if dtype == torch.bfloat16 else 23)).exp2()
    assert bool(((mean - want).abs() <= ulp).all()), "segment mean beyond 1 ulp of the correctly rounded quotient"


# ---- C. exact fuzz ------------------------------------------------------------------------------------------------------------------
def test_exact_fuzz():
    """Random batches, widths, dtypes and switch settings, bit equality with the reference; DN_EXACT_FUZZ_SECONDS (15 s default)."""
    rng = np.random.default_rng(int(os.environ.get("DN_EXACT_FUZZ_SEED", "2024")))
    flips = ["LAYER_GRAPHS_ENABLED", "LAYER_SMALL_ENABLED", "CONV_GRAPHS_ENABLED", "CHAIN2_F32_ENABLED", "LAYER_F32_ENABLED",
             "SELFSUM_ENABLED", "FOLD_ENABLED", "CLOSE_AGG_ENABLED", "LOCAL_INDEX_ENABLED"]
    t0, runs = time.time(), 0
    while time.time() - t0 < FUZZ_SECONDS or runs < 3:
        H = int(rng.choice([64, 128, 256]))
        dtype = torch.bfloat16 if rng.random() < 0.6 else torch.float32
        R = int(rng.integers(3, 17))
        G = int(rng.integers(1, 60))
        batch = X.si_batch(rng, G, R, int(rng.integers(1, 64)), float(rng.uniform(0, 6)), dummy=bool(rng.random() < 0.8))
        if len(batch[0]) == 0:
            continue
        sw = {k: bool(rng.random() < 0.7) for k in flips}
        act = "leaky_relu" if rng.random() < 0.3 else "relu"
        try:
            c = Case(int(rng.integers(1 << 30)), batch, H, R, dtype, act=act, nnz=int(rng.integers(1, 4)),
                     coef_rows=float(rng.choice([0.1, 1.0])))
        except X.PremiseError:
            continue
        with switches(**sw):
            got = c.run(c.layer(), _graph(batch))
        c.check(got, "fuzz run %d (H=%d %s R=%d G=%d %s %s): " % (runs, H, dtype, R, G, act, sw))
        runs += 1
    assert runs >= 3
