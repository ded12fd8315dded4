"""GPU tests of the SI count model LRP (subgraph_isomorphism/lrp.py), ops.lrp_pool / ops.lrp_perm_index and dn_lrp.hip.

* the materialised ego-net index against the reference's own COO lists on every golden batch, order included; a self-loop raises;
* exact parity: on small-integer operands (premise pinned by tests/test_lrp_host.py: every intermediate of the float64 reference
  is an integer below 2^24) the fused op, pool = sum, relu, and its gradients into x, edge_feat, weight, bias and factor are
  torch.equal to tests/lrp_ref.py -- H = 16 and 64, L = 3 and 4, a batch with an isolated node, a hub one past the kernel's LDS
  staging limit, one exactly at it, a dummy hub past the pair-table limit, parallel edges; and the composed path gives the same bits;
* layer and model goldens of the reference (tests/golden/si_lrp.npz) to RTOL = 1e-4 of each tensor's largest magnitude on the
  fused and on the composed path, with the path that ran read from the launch tags."""
import contextlib

import numpy as np
import pytest
import torch

import lrp_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RTOL = 1e-4
CASES = R.load_golden()
MODELS = sorted(n for n in CASES if CASES[n]["kind"] == "model")
LAYERS = sorted(n for n in CASES if CASES[n]["kind"] == "layer")
EXACT = R.exact_graphs()
OUT_KEYS = ("p_v_emb", "p_e_emb", "g_v_emb", "g_e_emb", "p_v_rep", "p_e_rep", "g_v_rep", "g_e_rep", "p_v_mask", "p_e_mask",
            "g_v_mask", "g_e_mask", "pred_c", "pred_v", "pred_e")
REPS = ("p_v_rep", "p_e_rep", "g_v_rep", "g_e_rep")


def _seq_len(case):
    return case["cfg"]["lrp_seq_len"] if case["kind"] == "model" else case["kw"]["lrp_seq_len"]


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


def _path(fused):
    from dummynode4graphlearning_amd import ops
    return ops.lrp_fused() if fused else ops.lrp_composed()


def _assert_path(tags, fused):
    if fused:
        assert {"lrp_pool_fwd", "lrp_pool_bwd"} <= tags and "gather_segsum" not in tags, tags
    else:
        assert "gather_segsum" in tags and not ({"lrp_pool_fwd", "lrp_pool_bwd"} & tags), tags


# ------------------------------------------------------------------------------------------------ the index
@pytest.mark.parametrize("name", MODELS + LAYERS)
def test_perm_index_equals_the_reference_lists(name):
    from dummynode4graphlearning_amd import ops
    case = CASES[name]
    L = _seq_len(case)
    for side in (("p", "g") if case["kind"] == "model" else ("g",)):
        d = R.batch(case, side)
        pi = ops.lrp_perm_index(_bare_graph(d), L)
        assert pi.perm_ptr.dtype == pi.perm_nodes.dtype == pi.perm_edges.dtype == torch.int32
        node_row, node_col, edge_row, edge_col, split = R.golden_lists(case, side)
        assert np.array_equal(np.diff(pi.perm_ptr.cpu().numpy()), split)
        got = R.index_lists(pi.perm_nodes.cpu().numpy().astype(np.int64), pi.perm_edges.cpu().numpy().astype(np.int64))
        for g, w, tag in zip(got, (node_row, node_col, edge_row, edge_col), ("node_row", "node_col", "edge_row", "edge_col")):
            assert np.array_equal(g, w), (side, tag)


@pytest.mark.parametrize("case", EXACT, ids=lambda c: c[0])
def test_perm_index_equals_the_restatement_on_the_exact_graphs(case):
    from dummynode4graphlearning_amd import ops
    name, d, L, H = case
    pi = ops.lrp_perm_index(_bare_graph(d), L)
    ptr, nodes, edges = R.perm_index(d, L)
    assert np.array_equal(pi.perm_ptr.cpu().numpy(), ptr) and np.array_equal(pi.perm_nodes.cpu().numpy(), nodes)
    assert np.array_equal(pi.perm_edges.cpu().numpy(), edges)


def test_a_self_loop_raises_and_names_the_graph():
    from dummynode4graphlearning_amd import ops
    from dummynode4graphlearning_amd._lib import DnHipError
    d = dict(R.batch(CASES["lrp_no_dummy"], "g"))
    first = int(np.sum(d["sizes"][:2]))                                           # first node of graph 2
    e = int(np.sum(d["esizes"][:2]))
    d["u"], d["v"] = np.array(d["u"], copy=True), np.array(d["v"], copy=True)
    d["u"][e] = d["v"][e] = first + 1
    with pytest.raises(DnHipError, match="self-loop.*node 1 of graph 2"):
        ops.lrp_perm_index(_bare_graph(d), 4)
    d["rev"] = np.zeros(len(d["u"]), bool)
    d["rev"][e] = True                                                            # a reversed edge does not count
    ops.lrp_perm_index(_bare_graph(d), 4)
    with pytest.raises(ValueError, match="lrp_seq_len"):
        ops.lrp_perm_index(_bare_graph(d), 5)


# ------------------------------------------------------------------------------------------------ exact parity
def _run_op(t, graph, L, act, pool, with_factor=True):
    from dummynode4graphlearning_amd import ops
    leaves = {k: t[k].to(DEV).requires_grad_(True) for k in ("x", "ef", "weight", "bias", "factor")}
    out = ops.lrp_pool(leaves["x"], leaves["ef"], leaves["weight"], leaves["bias"], leaves["factor"] if with_factor else None,
                       graph, L, act=act, pool=pool)
    out.backward(t["g"].to(DEV))
    return out.detach(), {k: (None if v.grad is None else v.grad.detach()) for k, v in leaves.items()}


@pytest.mark.parametrize("case", EXACT, ids=lambda c: c[0])
def test_exact_fused_op_and_gradients_and_the_composed_path(case):
    from dummynode4graphlearning_amd import ops
    name, d, L, H = case
    rng = np.random.default_rng(5)
    N, E = int(np.sum(d["sizes"])), len(d["u"])
    t = R.exact_inputs(rng, N, E, H, L)
    graph = _bare_graph(d)
    index = R.perm_index(d, L)
    if name == "past_stage_limit":
        deg = np.diff(graph.lrp_index(L).uptr.cpu().numpy())
        assert (int(deg.max()) + 1) * L * H * 4 > ops.LRP_STAGE_BYTES >= int(deg.max()) * L * H * 4
    if name == "at_stage_limit":
        deg = np.diff(graph.lrp_index(L).uptr.cpu().numpy())
        assert (int(deg.max()) + 2) * L * H * 4 > ops.LRP_STAGE_BYTES >= (int(deg.max()) + 1) * L * H * 4
    for act, with_factor in (("relu", True), ("none", False)):
        w = {k: t[k].double().requires_grad_(True) for k in ("x", "ef", "weight", "bias", "factor")}
        want, _ = R.lrp_pool(w["x"], w["ef"], w["weight"], w["bias"], w["factor"] if with_factor else None, index, act, "sum")
        want.backward(t["g"].double())
        R.exact_premise(want, *(w[k].grad for k in w if w[k].grad is not None))
        with ops.f32_exact(True), ops.lrp_fused():
            (out, grads), tags = _tags(lambda: _run_op(t, graph, L, act, "sum", with_factor))
        _assert_path(tags, True)
        assert torch.equal(out.double().cpu(), want.detach()), (name, act, "out")
        for k in w:
            if w[k].grad is None:
                assert grads[k] is None, k
            else:
                assert torch.equal(grads[k].double().cpu(), w[k].grad), (name, act, k)
        with ops.f32_exact(True), ops.lrp_composed():
            (out_c, grads_c), tags = _tags(lambda: _run_op(t, graph, L, act, "sum", with_factor))
        _assert_path(tags, False)
        assert torch.equal(out_c, out), (name, act, "composed out")
        for k in w:
            if grads[k] is not None:
                assert torch.equal(grads_c[k], grads[k]), (name, act, "composed", k)


def test_widths_the_kernel_does_not_take_run_composed():
    from dummynode4graphlearning_amd import ops
    d, L, H = R.batch(CASES["lrp_no_reversed_l3"], "g"), 3, 24
    rng = np.random.default_rng(8)
    t = R.exact_inputs(rng, int(np.sum(d["sizes"])), len(d["u"]), H, L)
    w = {k: t[k].double().requires_grad_(True) for k in ("x", "ef", "weight", "bias", "factor")}
    want, _ = R.lrp_pool(w["x"], w["ef"], w["weight"], w["bias"], w["factor"], R.perm_index(d, L), "relu", "sum")
    want.backward(t["g"].double())
    with ops.f32_exact(True), ops.lrp_fused():
        (out, grads), tags = _tags(lambda: _run_op(t, _bare_graph(d), L, "relu", "sum"))
    _assert_path(tags, False)
    assert torch.equal(out.double().cpu(), want.detach())
    assert all(torch.equal(grads[k].double().cpu(), w[k].grad) for k in w)


# ------------------------------------------------------------------------------------------------ goldens
@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("name", LAYERS)
def test_layer_matches_the_reference_goldens(name, fused):
    from dummynode4graphlearning_amd.subgraph_isomorphism import LRPLayer
    case = CASES[name]
    a = case["arrays"]
    torch.manual_seed(case["seed"])
    layer = LRPLayer(16, 16, **case["kw"])
    layer.load_state_dict({k: torch.from_numpy(np.array(a["param/" + k])) for k in case["keys"]}, strict=True)
    layer = layer.to(DEV).train()
    graph = R.make_graph(R.batch(case, "g"), DEV)
    x = torch.from_numpy(a["in/x"]).to(DEV).requires_grad_(True)
    ef = torch.from_numpy(a["in/ef"]).to(DEV).requires_grad_(True)

    def step():
        with _path(fused):
            out, eo = layer(graph, x, ef)
            assert eo is ef
            (out * torch.from_numpy(a["in/coef"]).to(DEV)).sum().backward()
        return out

    out, tags = _tags(step)
    _assert_path(tags, fused)
    checks = [("out", out, a["out/node_out"]), ("d x", x.grad, a["grad_in/x"]), ("d ef", ef.grad, a["grad_in/ef"])]
    checks += [("d " + k, p.grad, a["grad/" + k]) for k, p in layer.named_parameters()]
    sd = layer.state_dict()
    checks += [("buffer " + k, sd[k], a["after/" + k]) for k in case["buffers"] if not k.endswith("num_batches_tracked")]
    bad = []
    for tag, got, want in checks:
        e = R.rel_max(got, want)
        print("%s fused=%s %s rel_max %.3e" % (name, fused, tag, e))
        if not e < RTOL:
            bad.append((tag, e))
    assert not bad, bad


def _run_model(case, eight_args=False):
    from dummynode4graphlearning_amd.subgraph_isomorphism import LRP
    torch.manual_seed(case["seed"])
    model = LRP(**case["cfg"])
    model.load_state_dict(R.state_dict(case, "param"), strict=True)
    model = model.to(DEV).train()
    p, g = R.make_graph(R.batch(case, "p"), DEV), R.make_graph(R.batch(case, "g"), DEV)
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
    return model, res


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("name", MODELS)
def test_model_matches_the_reference_goldens(name, fused):
    case = CASES[name]
    a = case["arrays"]
    with _path(fused):
        (model, res), tags = _tags(lambda: _run_model(case))
    _assert_path(tags, fused)
    assert list(res.keys()) == list(OUT_KEYS)
    assert [k for k in OUT_KEYS if res[k] is None] == case["none_out"]
    bad = []

    def check(tag, got, want):
        e = R.rel_max(got, want)
        print("%s fused=%s %s rel_max %.3e" % (name, fused, tag, e))
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
    for k, p in model.named_parameters():
        if p.grad is not None:
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


def test_the_eight_argument_call_and_a_repeated_forward():
    case = CASES["lrp_l3_leaky"]
    with contextlib.nullcontext():
        _, res = _run_model(case)
        _, res8 = _run_model(case, eight_args=True)
    for k in OUT_KEYS:
        if res[k] is not None:
            assert torch.equal(res[k], res8[k]), k                               # the forward has no atomics: bit-identical
