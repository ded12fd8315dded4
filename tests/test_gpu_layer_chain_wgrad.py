"""The RGIN layer function that derives Linear 1's weight gradient from the conv's (ops._RginLayerChainFn, DN_LAYER_CHAIN_WGRAD; bf16,
H = 256, large batches) against the separate functions it replaces (the switch off), on config-5-shaped batches of 8 / 96 / 600 graphs
(fewer tiles than workgroups; one round; more than one tile a workgroup and several chunks a relation) with the row thresholds at 0:
  1. what must not move is bit-identical: out, x.grad, dW2, db2, the g0 rows, the per-graph sums of g1 (= gather_segsum), run to run;
  2. the five parameter gradients that are re-derived, against the layer in float64 with the GPU run's activation patterns;
  3. all seven parameter gradients bit for bit on integer operands (tests/exact_ref.py);
  4. dn_layer_chain_wgrad_combine alone against float64;
  5. which batches take the new launches (ops.KernelTimer tags)."""
import numpy as np
import pytest
import torch

import exact_ref as X
import test_gpu_exact as E

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H, R = 256, 16
GRAPHS = (8, 96, 600)
PARAMS5 = ("weight", "loop_weight", "bias", "mlp.0.weight", "mlp.0.bias")     # re-derived by the combine launch
LARGE = dict(MLP_BWD_FUSED_MIN_ROWS=0, WIDE_LAYER_MAX_ROWS=0)                  # every batch counts as a large one
ON = dict(LAYER_CHAIN_WGRAD_ENABLED=True)                                      # (the switch is set explicitly: either default)


def _batch(G, drop_rel=None):
    """config-5 graphs after the dummy augmentation as (src, dst, etype, node_ptr, edge_ptr); drop_rel: that relation's edges are
    relabelled to the next one (a relation without an edge)."""
    src, dst, et, nptr, eptr = E._config5(G)
    if drop_rel is not None:
        et = np.where(et == drop_rel, drop_rel + 1, et)
    return src, dst, et, nptr, eptr


def _layer(act, seed=23):
    from dummynode4graphlearning_amd.subgraph_isomorphism import RGINLayer
    torch.manual_seed(seed)
    layer = RGINLayer(H, H, num_rels=R, regularizer="basis", num_bases=-1, num_mlp_layers=2, act_func=act).to(DEV).to(torch.bfloat16)
    with torch.no_grad():
        layer.bias.copy_((torch.randn(H, device=DEV) * 0.1).to(torch.bfloat16))          # (initialised to zeros: c b^T would vanish)
    return layer


def _run(layer, g, et, x, coef, chain):
    """One step with the chain function on / off -> dict(tags, out, gx, grads, g1, g0, sums)."""
    from dummynode4graphlearning_amd import ops
    for p in layer.parameters():
        p.grad = None
    xs = x.clone().requires_grad_(True)
    seen = {}
    real_dgrad, real_fused = ops.layer_chain_dgrad, ops.mlp_bwd_fused

    def rec_dgrad(g1, w1, tiles):
        g0, sums = real_dgrad(g1, w1, tiles)
        seen.update(g1=g1, g0=g0, sums=sums)
        return g0, sums

    def rec_fused(g_, a, w, chunks, mask_in_bits=None, mask_out_bits=None, slope=0.0):
        res = real_fused(g_, a, w, chunks, mask_in_bits=mask_in_bits, mask_out_bits=mask_out_bits, slope=slope)
        if mask_in_bits is None:
            seen.update(g1=g_, g0=res[2])                                                 # (launch B of the separate functions)
        return res

    timer = ops.KernelTimer()
    with E.switches(LAYER_CHAIN_WGRAD_ENABLED=chain, layer_chain_dgrad=rec_dgrad, mlp_bwd_fused=rec_fused, **LARGE):
        with timer:
            out, _ = layer(g, xs, et)
            out.backward(coef)
    tags = [r[0] for r in timer.records]
    assert ("chain_dgrad" in tags) == chain and ("chain_combine" in tags) == chain, tags
    return dict(tags=tags, out=out.detach(), gx=xs.grad.detach(), grads={k: p.grad.detach().clone() for k, p in layer.named_parameters()},
                **seen)


def _bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int16), b.view(torch.int16))


_CASES = {}


def _case(G, act, drop_rel=None):
    """(layer, graph, et, x, coef, new run, old run) of one configuration: computed once, shared by the tests, never changed."""
    key = (G, act, drop_rel)
    if key not in _CASES:
        b = _batch(G, drop_rel)
        g, et = E._graph(b), E._t(b[2])
        N = int(b[3][-1])
        layer = _layer(act)
        gen = torch.Generator(device=DEV).manual_seed(5 + G)
        x = torch.randn(N, H, device=DEV, generator=gen).to(torch.bfloat16)
        coef = torch.randn(N, H, device=DEV, generator=gen).to(torch.bfloat16)
        new = _run(layer, g, et, x, coef, True)
        old = _run(layer, g, et, x, coef, False)
        _CASES[key] = (layer, g, et, x, coef, new, old, b)
    return _CASES[key]


CONFIGS = [(G, act, None) for G in GRAPHS for act in ("relu", "leaky_relu")] + [(96, "relu", 3)]
# ... and one batch on which the ring runs in its steady state: 36 tiles a workgroup (8 stages, 32-slot record ring, batches of 8 tiles
# all wrap several times) -- the bit-identity test only
STEADY = (9216, "relu", None)


@pytest.mark.parametrize("G,act,drop_rel", CONFIGS + [STEADY])
def test_unchanged_results_are_bit_identical(G, act, drop_rel):
    from dummynode4graphlearning_amd import ops
    layer, g, et, x, coef, new, old, b = _case(G, act, drop_rel)
    if drop_rel is not None:
        ix = g.row_index(et, R, True).parts[0][2]
        assert ix.rel_ptr_host[drop_rel + 1] == ix.rel_ptr_host[drop_rel]
    assert new["tags"].count("mlp_bwd_fused") == 1 and old["tags"].count("mlp_bwd_fused") == 2, (new["tags"], old["tags"])
    assert _bits(new["out"], old["out"]), "out"
    assert _bits(new["gx"], old["gx"]), "x.grad"
    for k in ("mlp.2.weight", "mlp.2.bias"):
        assert _bits(new["grads"][k], old["grads"][k]), k
    assert _bits(new["g1"], old["g1"]) and _bits(new["g0"], old["g0"]), "g1 / g0 rows"
    ix = g.row_index(et, R, True).parts[0][2]
    assert ix.num_aux_b == len(b[3]) - 1
    if (G, act, drop_rel) == STEADY:
        assert -(-G // 256) > 32
    want = ops.gather_segsum(new["g1"], ix.aux_b_idx, ix.aux_b_ptr, ix.num_aux_b)
    assert _bits(new["sums"], want), "per-graph sums of g1: %d elements differ" % int((new["sums"] != want).sum())
    again = _run(layer, g, et, x, coef, True)
    assert _bits(again["out"], new["out"]) and _bits(again["gx"], new["gx"])
    for k, v in new["grads"].items():
        assert _bits(again["grads"][k], v), "run to run: " + k
    if (G, act, drop_rel) == STEADY:
        del _CASES[STEADY]                                   # (a gigabyte of rows no other test reads)


def _rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def _rel_max(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


def _fp64_grads(layer, b, x, coef, et, g, slope):
    """Parameter gradients of the layer in float64 on the same bf16 parameters and inputs: the layer (rgin.py:102-160 + its MLP) written
    out per relation here, nothing rounded, with the GPU run's own activation patterns (its h1 / h2 > 0, recomputed with the same
    deterministic launches) in place of the activations -- oracle.layers.rgin_layer takes no mask and gathers [E, H, H] weights."""
    from dummynode4graphlearning_amd import ops
    with torch.no_grad():
        W_all = torch.cat([layer.weight, layer.loop_weight.unsqueeze(0)], 0)
        pre_gpu = ops.rel_transform_fused(x, W_all, layer.bias, g.row_index(et, R, True))
        h1_gpu, h2_gpu = ops.rows_chain2(pre_gpu, layer.mlp[0].weight, layer.mlp[0].bias, True, layer.mlp[2].weight, layer.mlp[2].bias, True,
                                         slope=slope)
    one = torch.ones((), dtype=torch.float64, device=DEV)
    m1, m2 = torch.where(h1_gpu > 0, one, one * slope), torch.where(h2_gpu > 0, one, one * slope)
    p = {k: v.detach().double().requires_grad_(True) for k, v in layer.named_parameters()}
    xr = x.double()
    src, dst = E._t(b[0]), E._t(b[1])
    h = xr @ p["loop_weight"] + p["bias"]
    for r in range(R):
        e = (et == r).nonzero().reshape(-1)
        if e.numel():
            h = h.index_add(0, dst[e], xr[src[e]] @ p["weight"][r])
    h1 = (h @ p["mlp.0.weight"].t() + p["mlp.0.bias"]) * m1
    out = (h1 @ p["mlp.2.weight"].t() + p["mlp.2.bias"]) * m2
    out.backward(coef.double())
    return {k: v.grad for k, v in p.items()}


@pytest.mark.parametrize("G,act,drop_rel", CONFIGS)
def test_parameter_gradients_against_fp64(G, act, drop_rel):
    """Relative L2 distance to float64 of the five re-derived gradients: the new path's at most 1.1 x the separate functions' on the same
    inputs, and within the existing pipeline test's 5e-3 (2e-2 of the maximum).  Measured on the MI355X: docs/LAB_NOTES.md, round 8."""
    layer, g, et, x, coef, new, old, b = _case(G, act, drop_rel)
    slope = 0.0 if act == "relu" else float(layer.act.negative_slope)
    ref = _fp64_grads(layer, b, x, coef, et, g, slope)
    for k in PARAMS5:
        dn, do = _rel_l2(new["grads"][k], ref[k]), _rel_l2(old["grads"][k], ref[k])
        mx = _rel_max(new["grads"][k], ref[k])
        print("G=%d %s drop=%s %-13s rel-L2 to fp64: new %.3e  old %.3e  (new max %.3e)" % (G, act, drop_rel, k, dn, do, mx))
        assert dn <= 1.1 * do, (k, dn, do)
        assert dn < 5e-3 and mx < 2e-2, (k, dn, mx)


@pytest.mark.parametrize("G,act", [(8, "relu"), (96, "leaky_relu"), (600, "relu")])
def test_exact_on_integer_operands(G, act):
    """Integer rows, signed sparse weights, small-integer biases, gradients in {-1, 0, 1} (exact_ref.check_premise: every stored row
    within 256 quanta, every fp32 sum below 2^24 -- M_r = A_r^T g1 and the per-graph sums of g1 included): the new path, the separate
    functions and float64 agree bit for bit on all seven parameter gradients, the output and the input gradient."""
    b = _batch(G)
    # (leaky_relu: gradients behind two masks at 0.25 are multiples of 1/16, so a stored gradient row holds 16 at most -- one nonzero
    #  a weight column and upstream gradients on one row in fifty keep the dummy nodes' sums of 30 rows inside that)
    kw = dict(nnz=8, s=2) if act == "relu" else dict(nnz=8, s=1, coef_rows=0.02)
    c = E.Case(12 + G, b, H, R, torch.bfloat16, act=act, **kw)
    # the premise of what only the new path forms: g1 = the gradient reaching z0 (a stage: within 256 quanta, checked by Case), its
    # per-graph sums (stored as bf16 rows) and M_r = A_r^T g1, whose absolute bound |A_r|^T |g1| is that of A_r^T g0 up to W1's signed
    # permutation of the columns (the weight gradient's bound, checked by Case)
    xr = X.leaf(c.x, DEV)
    pr = {k: X.leaf(v, DEV) for k, v in c.p.items()}
    st = {}
    X.rgin_ref(xr, c.src, c.dst, c.et, pr, R, act=act, slope=c.slope, stages=st, **c.kw).backward(c.coef)
    g1 = st["z0"].grad
    graph = torch.as_tensor(c.graph_of_row, device=DEV)
    sums = g1.new_zeros(len(b[3]) - 1, H).index_add(0, graph, g1)
    X.check_premise({"gagg": sums}, "bf16", q_bwd=X.quantum(g1))
    g = E._graph(b)
    layer = c.layer()
    with E.switches(**ON, **LARGE):
        new = c.run(layer, g)
    with E.switches(LAYER_CHAIN_WGRAD_ENABLED=False, **LARGE):
        old = c.run(layer, g)
    assert "chain_combine" in new[0] and new[0].count("mlp_bwd_fused") == 1, new[0]
    assert "chain_combine" not in old[0] and old[0].count("mlp_bwd_fused") == 2, old[0]
    c.check(new, "chain: ")
    c.check(old, "separate: ")
    assert len(new[3]) == 7
    for k in new[3]:
        assert _bits(new[3][k], old[3][k]), k


def _ulp_distance(got, want):
    """|got - want| in units of want's bf16 ulp (2^-7 of its binade; the smallest normal binade for zeros and subnormals)."""
    w = want.double().abs().clamp_min(2.0 ** -126)
    ulp = torch.exp2(torch.floor(torch.log2(w)) - 7)
    return (got.double() - want.double()).abs() / ulp


@pytest.mark.parametrize("rels", [1, 16])
def test_combine_launch_alone(rels):
    """dn_layer_chain_wgrad_combine on random fp32 M (full mantissas: M rounded to bf16 would show at 2^-9) and bf16 weights against
    float64: EVERY output within one bf16 ulp of the rounded float64 value, relative L2 <= 2e-3 -- for normal operands of both signs
    (sums that cancel far below their terms: an fp32 accumulation misses the ulp of such outputs, the fp64 one does not) and for
    positive operands (no cancellation at all).  The positive operands carry a factor in [1, 2) per row and column: sums of 256 alike
    positive terms all sit at one spot of one binade, and where that spot is low a correctly rounded bf16 tensor is itself 2.0e-3
    from float64 (measured: 2.007e-3 with exact sums); spread over their binades the values round at 1.5e-3 .. 1.8e-3."""
    from dummynode4graphlearning_amd import ops
    gen = torch.Generator(device=DEV).manual_seed(40 + rels)

    def rnd(*shape, signed, scale=1.0):
        if signed:
            return torch.randn(*shape, device=DEV, generator=gen) * scale
        return (torch.rand(*shape, device=DEV, generator=gen) * 0.5 + 0.5) * scale

    def spread(t, *dims):                                 # positive operands: a factor in [1, 2) along each of dims
        for d in dims:
            shape = [n if i == d % t.dim() else 1 for i, n in enumerate(t.shape)]
            t = t * (torch.rand(shape, device=DEV, generator=gen) + 1.0)
        return t

    for signed in (True, False):
        M = rnd(rels + 1, H, H, signed=signed, scale=8.0)
        c = rnd(H, signed=signed, scale=64.0)
        w1, Wc, WL, bias = (rnd(*s, signed=signed) for s in ((H, H), (rels, H, H), (H, H), (H,)))
        if not signed:
            M, c, w1, Wc, WL, bias = spread(M, -2, -1), spread(c, -1), spread(w1, -1), spread(Wc, -1), spread(WL, -1), spread(bias, -1)
        w1, Wc, WL, bias = (t.to(torch.bfloat16) for t in (w1, Wc, WL, bias))
        assert not torch.equal(M.to(torch.bfloat16).float(), M)
        dWc, db, dW1, db1 = ops.layer_chain_wgrad_combine(M, c, w1, Wc, WL, bias)
        Md, cd, w1d = M.double(), c.double(), w1.double()
        Wall = torch.cat([Wc, WL.unsqueeze(0)], 0).double()
        ref = {"dWc": Md @ w1d, "db": cd @ w1d, "dW1": torch.einsum("rij,rih->jh", Md, Wall) + torch.outer(cd, bias.double()), "db1": cd}
        for name, got in (("dWc", dWc), ("db", db), ("dW1", dW1), ("db1", db1)):
            d = _ulp_distance(got, ref[name].to(torch.bfloat16))
            l2 = _rel_l2(got, ref[name])
            print("R=%d signed=%s %-4s max ulp distance %.2f over %d outputs, rel-L2 %.3e" % (rels, signed, name, float(d.max()), d.numel(), l2))
            assert got.dtype == torch.bfloat16 and float(d.max()) <= 1.0, (name, signed, float(d.max()))
            assert l2 <= 2e-3, (name, signed, l2)


def _tags(layer, g, et, x, coef, **sw):
    from dummynode4graphlearning_amd import ops
    xs = x.clone().requires_grad_(True)
    timer = ops.KernelTimer()
    with E.switches(**sw):
        with timer:
            out, _ = layer(g, xs, et)
            out.backward(coef)
    return [r[0] for r in timer.records]


def test_dispatch():
    from dummynode4graphlearning_amd import ops, synthetic
    layer = _layer("relu")

    def operands(b):
        N = int(b[3][-1])
        gen = torch.Generator(device=DEV).manual_seed(9)
        return (E._graph(b), E._t(b[2]), torch.randn(N, H, device=DEV, generator=gen).to(torch.bfloat16),
                torch.randn(N, H, device=DEV, generator=gen).to(torch.bfloat16))

    # a qualifying batch: launch A only, the conv's weight-gradient launch only, the two new launches
    small = _batch(96)
    tags = _tags(layer, *operands(small), **ON, **LARGE)
    assert tags.count("mlp_bwd_fused") == 1 and tags.count("rows_wgrad") == 1 and "rows_wgrad_multi" not in tags, tags
    assert tags.count("chain_dgrad") == 1 and tags.count("chain_combine") == 1 and "gather_segsum" not in tags, tags
    today = _tags(layer, *operands(small), LAYER_CHAIN_WGRAD_ENABLED=False, **LARGE)
    assert today.count("mlp_bwd_fused") == 2 and today.count("rows_wgrad") == 1 and "chain_dgrad" not in today, today
    # ... whose input needs no gradient keeps today's launches
    g, et, x, coef = operands(small)
    with E.switches(**ON, **LARGE):
        with ops.KernelTimer() as timer:
            layer(g, x, et)[0].backward(coef)
    assert "chain_dgrad" not in [r[0] for r in timer.records]
    # one graph over 32 nodes: the fold is not absorbed by single-tile units -> today's launches
    big = synthetic.si_uniform_batch(7, 1, 40, 80, 14)
    big.update(max_nv=40, max_nvl=4, max_ne=80, max_nel=14, num_rels=R)
    mixed = X.concat_batches(_batch(8), E._synthetic(big), _batch(8))
    assert int(np.diff(mixed[3]).max()) == 41
    tags = _tags(layer, *operands(mixed), **ON, **LARGE)
    assert "chain_dgrad" not in tags and "chain_combine" not in tags and tags.count("mlp_bwd_fused") == 2, tags
    # the default thresholds keep a 2,048-graph batch where it is (the wide function's one weight-gradient launch)
    assert ops.MLP_BWD_FUSED_MIN_ROWS > 2048 * 31
    tags = _tags(layer, *operands(E._config5(2048)), **ON)
    assert "chain_dgrad" not in tags and "mlp_bwd_fused" not in tags and tags.count("rows_wgrad_multi") == 1, tags
