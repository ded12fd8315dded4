"""The SI count model LRP on the CPU: the NumPy restatement of the ego-net permutation index (tests/lrp_ref.py) against the
reference's own index lists, the exact-test premise of tests/test_gpu_lrp.py, and construction, state_dict and initial values
against the goldens of the reference's own model (tests/golden/si_lrp.npz, make_golden_si_lrp.py)."""
import hashlib

import numpy as np
import pytest
import torch

import lrp_ref as R

CASES = R.load_golden()
MODELS = sorted(n for n in CASES if CASES[n]["kind"] == "model")
LAYERS = sorted(n for n in CASES if CASES[n]["kind"] == "layer")
TOL = 1e-5


def _sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()[:24]


def _seq_len(case):
    return case["cfg"]["lrp_seq_len"] if case["kind"] == "model" else case["kw"]["lrp_seq_len"]


def test_the_import_and_the_exports_exist():
    from dummynode4graphlearning_amd import ops
    from dummynode4graphlearning_amd import subgraph_isomorphism as si
    assert issubclass(si.LRP, si.GraphAdjModelV2) and si.LRPLayer.__module__.endswith("subgraph_isomorphism.lrp")
    for name in ("lrp_pool", "lrp_perm_index", "lrp_composed", "LrpIndex", "LRP_STAGE_BYTES", "lrp_stage_nodes"):
        assert hasattr(ops, name), name


def test_goldens_cover_the_cases_they_should():
    seen = {"L": set(), "act": set(), "bn": set(), "share": set(), "dummy": set(), "rev": set(), "kinds": set()}
    for name in MODELS:
        case = CASES[name]
        cfg, g = case["cfg"], R.batch(case, "g")
        assert 4 <= len(g["sizes"]) <= 6 and 3 <= g["sizes"].min() and g["sizes"].max() <= 13
        seen["L"].add(cfg["lrp_seq_len"]), seen["act"].add(cfg["rep_act_func"]), seen["bn"].add(cfg["rep_lrp_batch_norm"])
        seen["share"].add(cfg["share_rep_net"]), seen["dummy"].add(g["dummy"] is not None), seen["rev"].add(g["rev"] is not None)
        keep = np.ones(len(g["u"]), bool) if g["rev"] is None else ~g["rev"]
        pairs = set(zip(g["u"][keep].tolist(), g["v"][keep].tolist()))
        if len(pairs) < int(keep.sum()):
            seen["kinds"].add("parallel")
        real = np.ones(int(g["sizes"].sum()), bool) if g["dummy"] is None else ~g["dummy"]
        deg = np.bincount([a for a, b in pairs if g["dummy"] is None or not g["dummy"][b]], minlength=len(real))[real]
        seen["kinds"].update("deg%d" % d for d in set(deg.tolist()) if d <= 5)
        if g["dummy"] is not None and any(g["dummy"][b] and not g["dummy"][a] for a, b in pairs):
            seen["kinds"].add("dummy_neighbour")
    assert seen["L"] == {3, 4} and seen["act"] == {"relu", "leaky_relu"} and seen["bn"] == {True, False}
    assert seen["share"] == {True, False} and seen["dummy"] == {True, False} and seen["rev"] == {True, False}
    assert {"parallel", "dummy_neighbour"} | {"deg%d" % d for d in range(6)} <= seen["kinds"], seen["kinds"]


@pytest.mark.parametrize("name", MODELS + LAYERS)
def test_restated_enumeration_reproduces_the_reference_index_lists(name):
    case = CASES[name]
    for side in (("p", "g") if case["kind"] == "model" else ("g",)):
        ptr, nodes, edges = R.perm_index(R.batch(case, side), _seq_len(case))
        node_row, node_col, edge_row, edge_col, split = R.golden_lists(case, side)
        got = R.index_lists(nodes, edges)
        for g, w, tag in zip(got, (node_row, node_col, edge_row, edge_col), ("node_row", "node_col", "edge_row", "edge_col")):
            assert np.array_equal(g, w), (side, tag)
        assert np.array_equal(np.diff(ptr), split) and (split >= 1).all()


def test_enumeration_rules_on_a_hand_made_graph():
    """Graph of 5 nodes, node 4 the dummy: 0 -> {1, 2, 4}, 1 -> {}, 2 -> {0}, 4 -> {0, 1, 2, 3}; a parallel edge 0 -> 1."""
    d = dict(sizes=[5], esizes=[9], u=np.array([0, 0, 0, 0, 2, 4, 4, 4, 4]), v=np.array([1, 2, 4, 1, 0, 0, 1, 2, 3]),
             dummy=np.array([0, 0, 0, 0, 1], bool), rev=None)
    ptr, nodes, edges = R.perm_index(d, 4)
    per = [nodes[ptr[i]:ptr[i + 1]].tolist() for i in range(5)]
    assert per[0] == [[0, 1, 2, 4], [0, 2, 1, 4]]                      # permutations of the non-dummy neighbours, the dummy last
    assert per[1] == [[1, -1, -1, -1]] and per[3] == [[3, -1, -1, -1]]  # isolated: the node alone
    assert per[2] == [[2, 0, -1, -1]]
    assert per[4] == [[4, 0, 1, 2], [4, 0, 1, 3], [4, 0, 2, 3], [4, 1, 2, 3]]   # combinations only (the second half is empty)
    assert edges[0].tolist() == [-1, 3, 1, 2, -1, -1, -1, -1, 4, -1, -1, -1, 5, 6, 7, -1]   # eid(0, 1) = the LAST parallel edge
    d["dummy"] = None
    assert R.perm_index(d, 3)[1][:6].tolist() == [[0, 1, 2], [0, 1, 4], [0, 2, 1], [0, 2, 4], [0, 4, 1], [0, 4, 2]]
    d["u"] = np.array([0, 0, 0, 0, 2, 4, 4, 4, 3])
    d["v"] = np.array([1, 2, 4, 1, 0, 0, 1, 2, 3])
    with pytest.raises(ValueError, match="self-loop on node 3 of graph 0"):
        R.perm_index(d, 4)


@pytest.mark.parametrize("name", LAYERS)
def test_restated_op_reproduces_the_golden_layers(name):
    """lrp_ref.lrp_pool in float64 inside the layer's torch glue gives the reference layer's output and gradients."""
    case = CASES[name]
    a, kw = case["arrays"], case["kw"]
    d = R.batch(case, "g")
    index = R.perm_index(d, kw["lrp_seq_len"])
    P = {k: torch.from_numpy(np.array(a["param/" + k])).double().requires_grad_(True) for k in case["params"]}
    x = torch.from_numpy(a["in/x"]).double().requires_grad_(True)
    ef = torch.from_numpy(a["in/ef"]).double().requires_grad_(True)
    act = R.act_fn(kw["act_func"])
    in_deg = torch.bincount(torch.from_numpy(d["v"]), minlength=x.shape[0]).double().view(-1, 1)
    factor = act(in_deg @ P["degnet_0.weight"].t() + P["degnet_0.bias"]) @ P["degnet_1.weight"].t() + P["degnet_1.bias"]
    out, _ = R.lrp_pool(x, ef, P["weight"], P.get("bias"), factor, index, kw["act_func"], "mean")
    if kw.get("batch_norm"):
        out = (out - out.mean(0)) / torch.sqrt(out.var(0, unbiased=False) + 1e-5) * P["bn.weight"] + P["bn.bias"]
    if kw.get("mlp"):
        out = act(out @ P["mlp.weight"].t() + P["mlp.bias"])
    (out * torch.from_numpy(a["in/coef"]).double()).sum().backward()
    checks = [("out", out, a["out/node_out"]), ("d x", x.grad, a["grad_in/x"]), ("d ef", ef.grad, a["grad_in/ef"])]
    checks += [("d " + k, P[k].grad, a["grad/" + k]) for k in case["params"]]
    bad = [(t, R.rel_max(g, w)) for t, g, w in checks if not R.rel_max(g, w) < TOL]
    assert not bad, bad


@pytest.mark.parametrize("case", R.exact_graphs(), ids=lambda c: c[0])
def test_exact_premise_of_the_gpu_tests(case):
    """On the integer inputs of the exact GPU tests every intermediate of the float64 reference is an integer below 2^24: the
    table rows, the pre-activation of every sequence, the pooled sums, the outputs and the four gradients."""
    name, d, L, H = case
    rng = np.random.default_rng(5)
    N, E = int(np.sum(d["sizes"])), len(d["u"])
    t = {k: v.double() for k, v in R.exact_inputs(rng, N, E, H, L).items()}
    for k in ("x", "ef", "weight", "bias", "factor"):
        t[k].requires_grad_(True)
    index = R.perm_index(d, L)
    wt = t["weight"].permute(2, 1, 0)
    R.exact_premise(t["x"] @ wt.reshape(-1, wt.shape[2]).t(), t["ef"] @ wt.reshape(-1, wt.shape[2]).t())
    out, z = R.lrp_pool(t["x"], t["ef"], t["weight"], t["bias"], t["factor"], index, "relu", "sum")
    pooled, _ = R.lrp_pool(t["x"], t["ef"], t["weight"], t["bias"], None, index, "relu", "sum")
    z.retain_grad()
    out.backward(t["g"])
    R.exact_premise(z, pooled, out, z.grad, t["x"].grad, t["ef"].grad, t["weight"].grad, t["bias"].grad, t["factor"].grad)
    # the row-factorised gradients the kernel accumulates: d T_node / d T_edge are sums of z.grad rows, bounded by P per row
    assert int(index[0][-1]) * float(z.grad.abs().max()) < 2 ** 24
    assert bool(out.any()) and bool(t["x"].grad.any()) and bool(t["ef"].grad.any())


@pytest.mark.parametrize("name", MODELS)
def test_state_dict_keys_shapes_and_initial_values_are_the_references(name):
    from dummynode4graphlearning_amd.subgraph_isomorphism import LRP
    case = CASES[name]
    torch.manual_seed(case["seed"])
    model = LRP(**case["cfg"])
    sd = model.state_dict()
    assert list(sd.keys()) == case["keys"]
    for k, t in sd.items():
        assert list(t.shape) == case["shapes"][k], k
        src = "init/" + case["alias"].get(k, k)
        if src in case["arrays"]:
            want = torch.from_numpy(np.array(case["arrays"][src]))
            assert torch.equal(t, want), "%s: initial values differ, max |diff| %.3e" % (k, float((t.double() - want.double()).abs().max()))
        assert _sha(t) == case["init_sha"][k], "%s: initial values differ" % k
    assert [k for k, _ in model.named_parameters()] == case["params"]
    assert (model.p_rep_net is model.g_rep_net) == case["cfg"]["share_rep_net"]
    model.load_state_dict(R.state_dict(case, "param"), strict=True)
    assert "g_rep_net.lrp.graph_lrp_(0).weight" in sd and "g_rep_net.lrp.graph_lrp_(0).degnet_1.bias" in sd


@pytest.mark.parametrize("name", LAYERS)
def test_layer_constructor_matches_the_reference(name):
    from dummynode4graphlearning_amd.subgraph_isomorphism import LRPLayer
    case = CASES[name]
    torch.manual_seed(case["seed"])
    layer = LRPLayer(16, 16, **case["kw"])
    sd = layer.state_dict()
    assert list(sd.keys()) == case["keys"] and [k for k, _ in layer.named_parameters()] == case["params"]
    for k, t in sd.items():
        assert _sha(t) == case["init_sha"][k], k
    assert layer.get_output_dim() == 16 and "lrp_seq_len=%d" % case["kw"]["lrp_seq_len"] in repr(layer)


def test_unsupported_sequence_lengths_raise():
    from dummynode4graphlearning_amd.subgraph_isomorphism import LRP, LRPLayer
    for L in (1, 5):
        with pytest.raises(ValueError, match="lrp_seq_len"):
            LRPLayer(16, 16, lrp_seq_len=L)
        with pytest.raises(ValueError, match="lrp_seq_len"):
            LRP(**dict(CASES["lrp_l4_relu"]["cfg"], lrp_seq_len=L))


def test_sparse_matrices_are_refused_and_forward_has_no_cpu_path():
    from dummynode4graphlearning_amd._lib import DnHipError
    from dummynode4graphlearning_amd.subgraph_isomorphism import LRP
    case = CASES["lrp_l3_leaky"]
    torch.manual_seed(0)
    model = LRP(**case["cfg"])
    p, g = R.make_graph(R.batch(case, "p"), "cpu"), R.make_graph(R.batch(case, "g"), "cpu")
    sp = torch.sparse_coo_tensor(torch.zeros((2, 1), dtype=torch.long), torch.ones(1), (4, 4))
    with pytest.raises(TypeError, match="built from the graph"):
        model(p, sp, None, None, g, None, None, None)
    with pytest.raises(TypeError):
        model(p, g, None)
    with pytest.raises(DnHipError):
        model(p, g)
    with pytest.raises(DnHipError):
        model(p, None, None, None, g, None, None, None)
