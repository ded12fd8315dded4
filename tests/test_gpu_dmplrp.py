"""GPU tests of the SI count model DMPLRP (subgraph_isomorphism/dmplrp.py), ops.lrp_pool_linear / ops.LrpIndex.collapsed and the
collapsed-index kernels of dn_lrp.hip.

* the collapsed index, entry for entry (col_ptr, rows ascending per node, int64 counts), against np.unique per node over the rows
  of the restated materialised index: every golden batch, lrp_ref.exact_graphs() (a hub one past the LDS staging limit of the fused
  kernels, one at it, a dummy hub past the pair-table limit), a hand-made graph (an isolated node, egos shorter than the sequence,
  kind-2 egos with n' = 0 and 1, two dummy neighbours, parallel and reversed edges) and a dummy hub of 40 leaves; two builds are
  torch.equal; a self-loop still raises;
* exact parity: on small-integer operands (premise pinned by tests/test_dmplrp_host.py) lrp_pool_linear(pool="sum") and its
  gradients into x, edge_feat, weight and bias are torch.equal to the float64 restatement and to ops.lrp_pool(act="none",
  factor=None, pool="sum") on the composed path; two forwards give the same bits; a width of 24 runs;
* pool="mean" on random fp32 operands and the layer and model goldens of the reference (tests/golden/si_dmplrp.npz) to
  RTOL = 1e-4 of each tensor's largest magnitude, on the collapsed path and on the lrp_pool(act="none") path, the path read from
  the launch tags.  The gradients of the shifts in front of a BatchNorm are zero in exact arithmetic and rounding noise in the
  goldens: they are held to 1e-4 of the largest weight gradient of their layer (dmplrp_ref.bn_shift)."""
import functools

import numpy as np
import pytest
import torch

import dmplrp_ref as DR
import lrp_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RTOL = 1e-4
CASES = DR.load_golden()
MODELS = sorted(n for n in CASES if CASES[n]["kind"] == "model")
LAYERS = sorted(n for n in CASES if CASES[n]["kind"] == "layer")
INDEX = DR.index_graphs()
EXACT = DR.exact_cases()
OUT_KEYS = ("p_v_emb", "p_e_emb", "g_v_emb", "g_e_emb", "p_v_rep", "p_e_rep", "g_v_rep", "g_e_rep", "p_v_mask", "p_e_mask",
            "g_v_mask", "g_e_mask", "pred_c", "pred_v", "pred_e")
REPS = ("p_v_rep", "p_e_rep", "g_v_rep", "g_e_rep")
LEAVES = ("x", "ef", "weight", "bias")


def _bare_graph(d):
    from dummynode4graphlearning_amd import BatchedGraph
    t = lambda a: torch.as_tensor(np.asarray(a)).to(DEV)                          # noqa: E731
    nd = {} if d.get("dummy") is None else {"is_dummy": t(d["dummy"])}
    ed = {} if d.get("rev") is None else {"is_reversed": t(d["rev"])}
    return BatchedGraph(t(d["u"]), t(d["v"]), int(np.sum(d["sizes"])), batch_num_nodes=torch.as_tensor(np.asarray(d["sizes"])),
                        batch_num_edges=torch.as_tensor(np.asarray(d["esizes"])), ndata=nd, edata=ed)


def _tags(fn):
    from dummynode4graphlearning_amd import ops
    with ops.KernelTimer() as timer:
        res = fn()
        return res, set(timer.summary())


class _path:
    """collapsed: the collapsed index; else lrp_pool(act="none") on the composed path."""

    def __init__(self, collapsed):
        from dummynode4graphlearning_amd import ops
        self.cms = (ops.lrp_collapsed(collapsed), ops.lrp_composed())

    def __enter__(self):
        for c in self.cms:
            c.__enter__()

    def __exit__(self, *exc):
        for c in reversed(self.cms):
            c.__exit__(*exc)
        return False


def _assert_path(tags, collapsed, backward=True):
    fused = {"lrp_pool_fwd", "lrp_pool_bwd"}
    if collapsed:
        assert "lrp_collapsed" in tags and (not backward or "lrp_collapsed_bwd" in tags) and not (fused & tags), tags
    else:
        assert "gather_segsum" in tags and not ({"lrp_collapsed", "lrp_collapsed_bwd"} | fused) & tags, tags


# ------------------------------------------------------------------------------------------------ the index
@pytest.mark.parametrize("case", INDEX, ids=lambda c: c[0])
def test_collapsed_index_equals_the_histogram_of_the_materialised_rows(case):
    from dummynode4graphlearning_amd import ops
    name, d, L = case
    col = _bare_graph(d).lrp_index(L).collapsed()
    assert isinstance(col, ops.LrpCollapsed)
    assert col.col_ptr.dtype == col.col_rows.dtype == torch.int32 and col.col_cnt.dtype == torch.int64
    ptr, rows, cnt = DR.collapsed_by_enumeration(d, L)
    assert np.array_equal(col.col_ptr.cpu().numpy(), ptr), name
    assert np.array_equal(col.col_rows.cpu().numpy(), rows), name
    assert np.array_equal(col.col_cnt.cpu().numpy(), cnt), name
    again = _bare_graph(d).lrp_index(L).collapsed()
    for a, b in zip(col, again):
        assert torch.equal(a, b)


def test_a_self_loop_still_raises():
    from dummynode4graphlearning_amd._lib import DnHipError
    d = dict(DR.hand_made_graph())
    d["u"], d["v"] = np.array(d["u"], copy=True), np.array(d["v"], copy=True)
    d["v"][0] = d["u"][0]                                                         # 1 -> 1
    with pytest.raises(DnHipError, match="self-loop.*node 1 of graph 0"):
        _bare_graph(d).lrp_index(4).collapsed()


# ------------------------------------------------------------------------------------------------ exact parity
@functools.lru_cache(maxsize=None)
def _exact_reference(i):
    """The operands of exact case i and the float64 reference (output, gradients), computed once."""
    name, d, L, H, in_dim = EXACT[i]
    rng = np.random.default_rng(5)
    t = R.exact_inputs(rng, int(np.sum(d["sizes"])), len(d["u"]), H, L, in_dim)
    w = {k: t[k].double().requires_grad_(True) for k in LEAVES}
    want = DR.pool_linear(w["x"], w["ef"], w["weight"], w["bias"], R.perm_index(d, L), "sum")
    want.backward(t["g"].double())
    R.exact_premise(want, *(w[k].grad for k in LEAVES))
    return t, want.detach(), {k: w[k].grad for k in LEAVES}


def _run_op(t, graph, L, pool, bias=True):
    from dummynode4graphlearning_amd import ops
    leaves = {k: t[k].to(DEV).requires_grad_(True) for k in LEAVES}
    out = ops.lrp_pool_linear(leaves["x"], leaves["ef"], leaves["weight"], leaves["bias"] if bias else None, graph, L, pool=pool)
    out.backward(t["g"].to(DEV))
    return out.detach(), {k: (None if v.grad is None else v.grad.detach()) for k, v in leaves.items()}


@pytest.mark.parametrize("i", range(len(EXACT)), ids=lambda i: "%s_L%d_H%d" % (EXACT[i][0], EXACT[i][2], EXACT[i][3]))
def test_exact_op_and_gradients_on_the_collapsed_and_the_composed_path(i):
    from dummynode4graphlearning_amd import ops
    name, d, L, H, in_dim = EXACT[i]
    t, want, want_grads = _exact_reference(i)
    graph = _bare_graph(d)
    with ops.f32_exact(True), _path(True):
        (out, grads), tags = _tags(lambda: _run_op(t, graph, L, "sum"))
        out2, _ = _run_op(t, graph, L, "sum")
    _assert_path(tags, True)
    assert torch.equal(out.double().cpu(), want), (name, "out")
    assert torch.equal(out2, out), (name, "a second forward")
    for k in LEAVES:
        assert torch.equal(grads[k].double().cpu(), want_grads[k]), (name, k)
    with ops.f32_exact(True), _path(False):
        (out_c, grads_c), tags = _tags(lambda: _run_op(t, graph, L, "sum"))
    _assert_path(tags, False)
    assert torch.equal(out_c, out), (name, "composed out")
    for k in LEAVES:
        assert torch.equal(grads_c[k], grads[k]), (name, "composed", k)
    with ops.f32_exact(True), ops.lrp_composed():
        leaves = {k: t[k].to(DEV) for k in LEAVES}
        direct = ops.lrp_pool(leaves["x"], leaves["ef"], leaves["weight"], leaves["bias"], None, graph, L, act="none", pool="sum")
    assert torch.equal(direct, out), (name, "ops.lrp_pool")


def test_a_width_of_24_runs():
    from dummynode4graphlearning_amd import ops
    d, L, H = DR.hand_made_graph(), 3, 24
    rng = np.random.default_rng(8)
    t = R.exact_inputs(rng, int(np.sum(d["sizes"])), len(d["u"]), H, L)
    w = {k: t[k].double().requires_grad_(True) for k in LEAVES}
    want = DR.pool_linear(w["x"], w["ef"], w["weight"], w["bias"], R.perm_index(d, L), "sum")
    want.backward(t["g"].double())
    with ops.f32_exact(True), _path(True):
        (out, grads), tags = _tags(lambda: _run_op(t, _bare_graph(d), L, "sum"))
    _assert_path(tags, True)
    assert torch.equal(out.double().cpu(), want.detach())
    assert all(torch.equal(grads[k].double().cpu(), w[k].grad) for k in LEAVES)


# ------------------------------------------------------------------------------------------------ mean
@pytest.mark.parametrize("case", [("hand_made", DR.hand_made_graph(), 4, 16), ("hand_made", DR.hand_made_graph(), 2, 32),
                                  ("dummy_hub_40", DR.dummy_star(40), 4, 16),
                                  ("golden", R.batch(CASES["dmplrp_no_share"], "g"), 3, 64)], ids=lambda c: "%s_L%d_H%d" % (c[0], c[2], c[3]))
@pytest.mark.parametrize("bias", [True, False])
def test_mean_pooling_against_float64(case, bias):
    name, d, L, H = case
    rng = np.random.default_rng(21)
    N, E = int(np.sum(d["sizes"])), len(d["u"])
    f = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(np.float32))      # noqa: E731
    t = dict(x=f(N, H), ef=f(E, H), weight=f(H, H, L * L) * 0.2, bias=f(H), g=f(N, H))
    w = {k: t[k].double().requires_grad_(True) for k in LEAVES}
    want = DR.pool_linear(w["x"], w["ef"], w["weight"], w["bias"] if bias else None, R.perm_index(d, L), "mean")
    want.backward(t["g"].double())
    bad = []
    for collapsed in (True, False):
        with _path(collapsed):
            (out, grads), tags = _tags(lambda: _run_op(t, _bare_graph(d), L, "mean", bias))
        _assert_path(tags, collapsed)
        checks = [("out", out, want)] + [("d " + k, grads[k], w[k].grad) for k in LEAVES if bias or k != "bias"]
        assert bias or grads["bias"] is None
        for tag, got, ref in checks:
            e = R.rel_max(got, ref)
            print("%s L=%d H=%d bias=%s collapsed=%s %s rel_max %.3e" % (name, L, H, bias, collapsed, tag, e))
            if not e < RTOL:
                bad.append((collapsed, tag, e))
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ goldens
@pytest.mark.parametrize("collapsed", [True, False])
@pytest.mark.parametrize("name", LAYERS)
def test_layer_matches_the_reference_goldens(name, collapsed):
    from dummynode4graphlearning_amd.subgraph_isomorphism import DMPLRPPoolLayer
    case = CASES[name]
    a = case["arrays"]
    torch.manual_seed(case["seed"])
    layer = DMPLRPPoolLayer(16, 16, **case["kw"])
    layer.load_state_dict({k: torch.from_numpy(np.array(a["param/" + k])) for k in case["keys"]}, strict=True)
    layer = layer.to(DEV).train()
    graph = R.make_graph(R.batch(case, "g"), DEV)
    x = torch.from_numpy(a["in/x"]).to(DEV).requires_grad_(True)
    ef = torch.from_numpy(a["in/ef"]).to(DEV).requires_grad_(True)

    def step():
        with _path(collapsed):
            out, eo = layer(graph, x, ef)
            ((out * torch.from_numpy(a["in/coef"]).to(DEV)).sum() + (eo * torch.from_numpy(a["in/coef_e"]).to(DEV)).sum()).backward()
        return out, eo

    (out, eo), tags = _tags(step)
    _assert_path(tags, collapsed)
    checks = [("out", out, a["out/node_out"]), ("edge out", eo, a["out/edge_out"]), ("d x", x.grad, a["grad_in/x"]),
              ("d ef", ef.grad, a["grad_in/ef"])]
    assert [k for k, p in layer.named_parameters() if p.grad is None] == case["none_grad"]
    bad = []
    kw = case["kw"]
    for k, p in layer.named_parameters():
        if p.grad is None:
            continue
        if DR.bn_shift(kw.get("batch_norm", True), kw.get("num_mlp_layers", 2), k):   # true gradient zero: see dmplrp_ref.bn_shift
            bound, got = RTOL * DR.layer_weight_grad_scale(case, k), float(p.grad.abs().max())
            print("%s collapsed=%s d %s |max| %.3e bound %.3e" % (name, collapsed, k, got, bound))
            if not got < bound:
                bad.append((k, got))
            continue
        checks.append(("d " + k, p.grad, a["grad/" + k]))
    sd = layer.state_dict()
    checks += [("buffer " + k, sd[k], a["after/" + k]) for k in case["buffers"] if not k.endswith("num_batches_tracked")]
    for tag, got, want in checks:
        e = R.rel_max(got, want)
        print("%s collapsed=%s %s rel_max %.3e" % (name, collapsed, tag, e))
        if not e < RTOL:
            bad.append((tag, e))
    assert not bad, bad


def _run_model(case, eight_args=False, model=None, graphs=None):
    from dummynode4graphlearning_amd.subgraph_isomorphism import DMPLRP
    if model is None:
        torch.manual_seed(case["seed"])
        model = DMPLRP(**case["cfg"])
        model.load_state_dict(R.state_dict(case, "param"), strict=True)
        model = model.to(DEV).train()
    p, g = graphs or (R.make_graph(R.batch(case, "p"), DEV), R.make_graph(R.batch(case, "g"), DEV))
    if eight_args:
        res = model(p, None, None, None, g, g.lrp_index(case["cfg"]["lrp_seq_len"]), None, None)
    else:
        res = model(p, g)
    for k in REPS:
        res[k].retain_grad()
    B = case["B"]
    loss = (res["pred_c"] * (torch.arange(1, B + 1, dtype=torch.float32, device=DEV).view(-1, 1) / B)).sum()
    for k in ("pred_v", "pred_e"):
        c = case["arrays"].get("coef/" + k)
        if res[k] is not None and c is not None:
            loss = loss + (res[k] * torch.from_numpy(c).to(DEV)).sum()
    loss.backward()
    return model, res, (p, g)


@pytest.mark.parametrize("collapsed", [True, False])
@pytest.mark.parametrize("name", MODELS)
def test_model_matches_the_reference_goldens(name, collapsed):
    case = CASES[name]
    a = case["arrays"]
    with _path(collapsed):
        (model, res, _), tags = _tags(lambda: _run_model(case))
    _assert_path(tags, collapsed)
    assert list(res.keys()) == list(OUT_KEYS)
    assert [k for k in OUT_KEYS if res[k] is None] == case["none_out"]
    bad = []

    def check(tag, got, want):
        e = R.rel_max(got, want)
        print("%s collapsed=%s %s rel_max %.3e" % (name, collapsed, tag, e))
        if not e < RTOL:
            bad.append((tag, e))

    for k in OUT_KEYS:
        if res[k] is None:
            continue
        want = a["out/" + k]
        assert tuple(res[k].shape) == tuple(want.shape), k
        if res[k].dtype == torch.bool:
            assert torch.equal(res[k].cpu(), torch.from_numpy(want)), k
        else:
            check("out " + k, res[k], want)
    assert [k for k, p in model.named_parameters() if p.grad is None] == case["none_grad"]
    cfg = case["cfg"]
    for k, p in model.named_parameters():
        if p.grad is None:
            continue
        if "_rep_net." in k and DR.bn_shift(cfg["rep_dmpnn_batch_norm"], cfg["rep_dmpnn_num_mlp_layers"], k):
            bound, got = RTOL * DR.layer_weight_grad_scale(case, k), float(p.grad.abs().max())
            print("%s collapsed=%s grad %s |max| %.3e bound %.3e" % (name, collapsed, k, got, bound))
            if not got < bound:
                bad.append((k, got))
            continue
        check("grad " + k, p.grad, a["grad/" + k])
    assert [k for k in REPS if res[k].grad is None] == case["none_rep"]
    for k in REPS:
        if res[k].grad is not None:
            check("grad_rep " + k, res[k].grad, a["grad_rep/" + k])
    sd = model.state_dict()
    for k in case["buffers"]:
        src = "after/" + case["alias"].get(k, k)
        if k.endswith("num_batches_tracked"):
            assert int(sd[k]) == int(a[src]), k
        else:
            check("buffer " + k, sd[k], a[src])
    assert not bad, bad


def test_the_eight_argument_call_and_a_repeated_forward_on_a_cached_index():
    case = CASES["dmplrp_no_share"]                                              # no BatchNorm: a second step sees the same state
    with _path(True):
        model, res, graphs = _run_model(case)
        _, res8, _ = _run_model(case, eight_args=True)
        assert graphs[1].lrp_index(case["cfg"]["lrp_seq_len"])._collapsed is not None
        _, again, _ = _run_model(case, model=model, graphs=graphs)
    for k in OUT_KEYS:
        if res[k] is not None:
            assert torch.equal(res[k], res8[k]), k                               # no atomics on this path: bit-identical
            assert torch.equal(res[k], again[k]), k
