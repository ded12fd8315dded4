"""The SI count model DMPLRP on the CPU: construction, state_dict and initial values against the goldens of the reference's own
model (tests/golden/si_dmplrp.npz, make_golden_si_dmplrp.py), the closed forms of the collapsed pooling index (tests/dmplrp_ref.py,
the restatement of what dn_lrp_collapse_*_i32 evaluate) against the histogram of the enumerated sequences, and the exact-test
premise of tests/test_gpu_dmplrp.py."""
import hashlib

import numpy as np
import pytest
import torch

import dmplrp_ref as DR
import lrp_ref as R

CASES = DR.load_golden()
MODELS = sorted(n for n in CASES if CASES[n]["kind"] == "model")
LAYERS = sorted(n for n in CASES if CASES[n]["kind"] == "layer")


def _sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()[:24]


def test_the_exports_exist():
    from dummynode4graphlearning_amd import _lib, ops
    from dummynode4graphlearning_amd import subgraph_isomorphism as si
    assert issubclass(si.DMPLRP, si.GraphAdjModelV2) and issubclass(si.DMPLRPPoolLayer, si.DMPLayer)
    assert si.DMPLRPPoolLayer.__module__.endswith("subgraph_isomorphism.dmplrp")
    for name in ("lrp_pool_linear", "lrp_collapsed", "lrp_collapsed_enabled", "LrpCollapsed", "LRP_COLLAPSED_DEFAULT"):
        assert hasattr(ops, name), name
    assert hasattr(ops.LrpIndex, "collapsed")
    for name in ("dn_lrp_collapse_count_i32", "dn_lrp_collapse_fill_i32"):
        assert name in _lib._SIGS, name


def test_goldens_cover_the_cases_they_should():
    m = {n: CASES[n] for n in MODELS}
    cfg = lambda n: m[n]["cfg"]                                                                       # noqa: E731
    assert any(cfg(n)["lrp_seq_len"] == 4 and cfg(n)["rep_act_func"] == "relu" and cfg(n)["rep_num_graph_layers"] == 2
               and cfg(n)["share_rep_net"] for n in m)
    assert any(cfg(n)["lrp_seq_len"] == 3 and cfg(n)["rep_act_func"] == "leaky_relu" and cfg(n)["rep_dmpnn_batch_norm"] for n in m)
    assert any(not cfg(n)["share_rep_net"] and cfg(n)["emb_net"] == "Equivariant" for n in m)
    assert any(R.batch(m[n], "g")["dummy"] is None for n in m)
    assert any(R.batch(m[n], "g")["rev"] is None for n in m)
    assert any(cfg(n)["filter_net"] == "None" and not cfg(n)["rep_residual"] for n in m)
    kws = [CASES[n]["kw"] for n in LAYERS]
    assert any(k["lrp_seq_len"] == 4 and "num_mlp_layers" not in k and "batch_norm" not in k for k in kws)
    assert any(k["lrp_seq_len"] == 3 and k.get("num_mlp_layers") == 0 and k.get("act_func") == "leaky_relu" for k in kws)
    assert any(k["lrp_seq_len"] == 2 and k.get("bias") is False for k in kws)
    both = False
    for n in LAYERS:
        g = R.batch(CASES[n], "g")
        if CASES[n]["kw"].get("batch_norm") and g["edummy"] is not None:
            de = g["edummy"] & ~(g["rev"] if g["rev"] is not None else np.zeros(len(g["u"]), bool))
            both = both or (bool(g["dummy"][g["u"][de]].any()) and bool(g["dummy"][g["v"][de]].any()))
    assert both, "no batch-normalised layer case with counted dummy edges in both directions"


@pytest.mark.parametrize("name", MODELS)
def test_state_dict_keys_shapes_and_initial_values_are_the_references(name):
    from dummynode4graphlearning_amd.subgraph_isomorphism import DMPLRP
    case = CASES[name]
    torch.manual_seed(case["seed"])
    model = DMPLRP(**case["cfg"])
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
    L = case["cfg"]["lrp_seq_len"]
    assert list(sd["g_rep_net.DMPLRP.graph_DMPLRP_(0).lrp_weight"].shape) == [16, 16, L * L]
    assert "g_rep_net.DMPLRP.graph_DMPLRP_(0).lrp_bias" in sd


@pytest.mark.parametrize("name", LAYERS)
def test_layer_constructor_matches_the_reference(name):
    from dummynode4graphlearning_amd.subgraph_isomorphism import DMPLRPPoolLayer
    case = CASES[name]
    torch.manual_seed(case["seed"])
    layer = DMPLRPPoolLayer(16, 16, **case["kw"])
    sd = layer.state_dict()
    assert list(sd.keys()) == case["keys"] and [k for k, _ in layer.named_parameters()] == case["params"]
    assert case["keys"][:7] == ["in_weight", "out_weight", "src_weight", "dst_weight", "nloop_weight", "eloop_weight", "lrp_weight"]
    for k, t in sd.items():
        assert _sha(t) == case["init_sha"][k], k
    assert layer.get_output_dim() == 16 and "lrp_seq_len=%d" % case["kw"]["lrp_seq_len"] in repr(layer)


def test_the_hand_made_graph_holds_what_it_should():
    d = DR.hand_made_graph()
    keep = ~d["rev"]
    pairs = list(zip(d["u"][keep].tolist(), d["v"][keep].tolist()))
    adj = {x: sorted(set(b for a, b in pairs if a == x)) for x in range(14)}
    dm = d["dummy"]
    nd = {x: sum(dm[w] for w in adj[x]) for x in adj}
    assert adj[0] == [] and not any(b == 0 for a, b in pairs)                                       # an isolated node
    assert not dm[1] and nd[1] == 0 and len(adj[1]) == 1                                             # kind 0, d < L - 1
    assert dm[9] and len(adj[9]) == 2 and dm[13] and len(adj[13]) == 1                               # dummies with d < L - 1 (L = 4)
    assert not dm[4] and nd[4] == 1 and len(adj[4]) == 1                                             # kind 2, n' = 0
    assert not dm[5] and nd[5] == 1 and len(adj[5]) == 2                                             # kind 2, n' = 1
    assert nd[6] == 2 and nd[7] == 2                                                                 # two dummy neighbours
    assert len(pairs) > len(set(pairs)) and bool(d["rev"].any())                                     # parallel and reversed edges


@pytest.mark.parametrize("case", DR.index_graphs(), ids=lambda c: c[0])
def test_closed_forms_equal_the_histogram_of_the_enumerated_rows(case):
    name, d, L = case
    for seq in ((2, 3, 4) if name.startswith("hand_made") else (L,)):
        want = DR.collapsed_by_enumeration(d, seq)
        got = DR.collapsed_closed_form(d, seq)
        for g, w, tag in zip(got, want, ("col_ptr", "col_rows", "col_cnt")):
            assert np.array_equal(g, w), (name, seq, tag)
        ptr = R.perm_index(d, seq)[0]
        assert want[0][-1] <= (seq + seq * (seq - 1)) * ptr[-1]


def test_the_collapsed_list_of_a_hub_is_sized_by_its_edges_not_its_sequences():
    d = DR.dummy_star(40)
    ptr, rows, cnt = DR.collapsed_by_enumeration(d, 4)
    assert R.perm_index(d, 4)[0][1] == 9880                                                          # C(40, 3) sequences of the hub
    assert ptr[1] <= 41 * 3 + 6 * len(d["u"]) and int(cnt[:ptr[1]].max()) == 9880


@pytest.mark.parametrize("case", DR.exact_cases(), ids=lambda c: "%s_L%d_H%d" % (c[0], c[2], c[3]))
def test_exact_premise_of_the_gpu_tests(case):
    """On the integer inputs of the exact GPU tests every intermediate is an integer below 2^24, whatever the order of the sums:
    the table rows, the pooled sums over the materialised sequences (the composed path) and over the collapsed rows (bounded by
    the sum of the magnitudes of the weighted rows), the outputs and the four gradients with the magnitudes of their terms."""
    name, d, L, H, in_dim = case
    rng = np.random.default_rng(5)
    N, E = int(np.sum(d["sizes"])), len(d["u"])
    t = {k: v.double() for k, v in R.exact_inputs(rng, N, E, H, L, in_dim).items()}
    for k in ("x", "ef", "weight", "bias"):
        t[k].requires_grad_(True)
    index = R.perm_index(d, L)
    wt = t["weight"].permute(2, 1, 0).reshape(-1, in_dim)
    diag = [k * (L + 1) for k in range(L)]
    w4 = t["weight"].permute(2, 1, 0)                                                                # [L^2, H, in]
    t_node = (t["x"] @ w4[diag].reshape(L * H, in_dim).t()).reshape(-1, H)
    off = [s for s in range(L * L) if s % (L + 1) != 0]
    t_edge = (t["ef"] @ w4[off].reshape(L * (L - 1) * H, in_dim).t()).reshape(-1, H)
    table = torch.cat([t_node, t_edge], 0).detach()
    R.exact_premise(table, t["x"].detach().abs() @ wt.detach().abs().t(), t["ef"].detach().abs() @ wt.detach().abs().t())
    out = DR.pool_linear(t["x"], t["ef"], t["weight"], t["bias"], index, "sum")
    out.backward(t["g"])
    R.exact_premise(out, t["x"].grad, t["ef"].grad, t["weight"].grad, t["bias"].grad)
    # the collapsed path: out[v] = sum_rows cnt T[row] + P_v bias, d T[row] = sum_v cnt g[v], d bias = sum_v P_v g[v]
    col_ptr, col_rows, col_cnt = (torch.from_numpy(a) for a in DR.collapsed_closed_form(d, L))
    node = torch.repeat_interleave(torch.arange(N), col_ptr[1:] - col_ptr[:-1])
    P = torch.from_numpy(np.diff(index[0])).double()
    mag = torch.zeros(N, H, dtype=torch.float64).index_add(0, node, col_cnt.double().unsqueeze(1) * table[col_rows].abs())
    got = torch.zeros(N, H, dtype=torch.float64).index_add(0, node, col_cnt.double().unsqueeze(1) * table[col_rows])
    assert torch.equal(got + P.unsqueeze(1) * t["bias"].detach(), out.detach())
    R.exact_premise(mag + P.unsqueeze(1) * t["bias"].detach().abs())
    d_mag = torch.zeros_like(table).index_add(0, col_rows, col_cnt.double().unsqueeze(1) * t["g"].abs()[node])
    R.exact_premise(d_mag, (P.unsqueeze(1) * t["g"].abs()).sum(0, keepdim=True))
    # the Linear kernels' backward: d W = rows^T d T, d rows = d T W, with the magnitudes of their terms
    dn, de = d_mag[:N * L].reshape(N, L * H), d_mag[N * L:].reshape(E, L * (L - 1) * H)
    R.exact_premise(t["x"].detach().abs().t() @ dn, t["ef"].detach().abs().t() @ de)
    R.exact_premise(dn @ w4[diag].reshape(L * H, in_dim).detach().abs(), de @ w4[off].reshape(L * (L - 1) * H, in_dim).detach().abs())
    # the composed path sums the d z rows of the sequences: bounded by the sequences of the batch
    assert int(index[0][-1]) * float(t["g"].abs().max()) < 2 ** 24
    assert bool(out.any()) and bool(t["x"].grad.any()) and (E == 0 or bool(t["ef"].grad.any()))


def test_bad_arguments_raise():
    from dummynode4graphlearning_amd.subgraph_isomorphism import DMPLRP, DMPLRPPoolLayer
    for L in (1, 5):
        with pytest.raises(ValueError, match="lrp_seq_len"):
            DMPLRPPoolLayer(16, 16, lrp_seq_len=L)
        with pytest.raises(ValueError, match="lrp_seq_len"):
            DMPLRP(**dict(CASES["dmplrp_l4_relu"]["cfg"], lrp_seq_len=L))
    with pytest.raises(ValueError, match="input_dim == hidden_dim"):
        DMPLRPPoolLayer(16, 32)


def test_sparse_matrices_are_refused_and_forward_has_no_cpu_path():
    from dummynode4graphlearning_amd._lib import DnHipError
    from dummynode4graphlearning_amd.subgraph_isomorphism import DMPLRP, DMPLRPPoolLayer
    case = CASES["dmplrp_no_share"]
    torch.manual_seed(0)
    model = DMPLRP(**case["cfg"])
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
    layer = DMPLRPPoolLayer(16, 16, lrp_seq_len=3)
    with pytest.raises(TypeError, match="built from the graph"):
        layer(g, torch.zeros(g.number_of_nodes(), 16), torch.zeros(g.number_of_edges(), 16), None, sp, None)
