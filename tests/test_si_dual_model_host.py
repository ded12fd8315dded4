"""SI count models CompGCN / DMPNN on the CPU: construction, state_dict, initial values, expand and option errors against the
goldens of the reference's own models (tests/golden/si_dual_models*.npz, make_golden_si_dual_models.py), and the float64
restatement of the whole forward (tests/si_dual_model_ref.py) against the same goldens at 1e-5 of each tensor's largest magnitude
(the level test_si_model_host.py and the oracle tests use; the reference's own fp32 rounding on these cases is ~5e-7)."""
import numpy as np
import pytest
import torch

import si_dual_model_ref as R

CASES = R.load_golden()
NAMES = sorted(CASES)
FORWARD = [n for n in NAMES if CASES[n]["forward"]]
TOL = 1e-5


@pytest.mark.parametrize("name", NAMES)
def test_state_dict_keys_shapes_and_initial_values_are_the_references(name):
    case = CASES[name]
    model = R.build_model(case, load=False)
    sd = model.state_dict()
    assert list(sd.keys()) == case["keys"]
    for k, t in sd.items():
        assert list(t.shape) == case["shapes"][k], k
        src = "init/" + case["alias"].get(k, k)
        if src in case["arrays"]:                                  # the values are stored for a few cases: say where and by how much
            want = torch.from_numpy(np.array(case["arrays"][src]))
            assert torch.equal(t, want), "%s: initial values differ, max |diff| %.3e" % (k, float((t.double() - want.double()).abs().max()))
        assert R.sha(t) == case["init_sha"][k], "%s: initial values differ" % k
    assert [k for k, _ in model.named_parameters()] == case["params"]
    cfg = case["cfg"]
    assert (model.p_enc_net is model.g_enc_net) == cfg["share_enc_net"]
    assert model.p_emb_net is not model.g_emb_net                 # (sic) only expand() shares the emb net
    assert (model.p_rep_net is model.g_rep_net) == cfg["share_rep_net"]
    assert all(k.startswith("p_") for k in case["alias"])
    assert all(not p.requires_grad for k, p in model.named_parameters() if "_enc_net." in k)
    assert (model.pred_net["v"] is None) == (not cfg["node_pred"]) and (model.pred_net["e"] is None) == (not cfg["edge_pred"])
    model.load_state_dict(R.state_dict(case, "param"), strict=True)


def test_key_names_and_dims_match_the_issue_examples():
    model = R.build_model(CASES["compgcn_mult"], load=False)
    sd = model.state_dict()
    for k in ("g_enc_net.el.weight", "g_emb_net.el.weight", "g_rep_net.compgcn.graph_compgcn_(1).rel_weight",
              "pred_net.v.p_fc.weight", "pred_net.e.pred_fc2.bias"):
        assert k in sd, k
    assert model.get_graph_enc_dims() == {"v": 8, "vl": 6, "el": 4}
    assert model.get_graph_enc_dim() == (14, 32)
    assert model.get_rep_dim() == (16 + 14 + 2, 16 + 32 + 2)
    sd = R.build_model(CASES["dmpnn"], load=False).state_dict()
    assert "g_rep_net.dmpnn.graph_dmpnn_(0).eloop_weight" in sd and "g_rep_net.dmpnn.graph_dmpnn_(1).emlp.2.bias" in sd
    # create_emb_net divides each weight by enc_dim // base (basemodel.py:1086-1090): an orthogonal [8, 16] has unit rows
    w = R.build_model(CASES["compgcn_mult"], load=False).g_emb_net["v"].weight
    assert torch.allclose(w.norm(dim=1), torch.full((8,), 1.0 / 4), atol=1e-6)


def test_expand_matches_the_reference():
    case = CASES["dmpnn_expand"]
    model = R.build_model(case)
    kw = dict(case["cfg"])
    kw.update(case["expand_kw"])
    torch.manual_seed(case["expand_seed"])
    model.expand(**kw)
    got = model.state_dict()
    want = {k[len("expand/"):]: v for k, v in case["arrays"].items() if k.startswith("expand/")}
    assert list(got.keys()) == list(want.keys())
    for k, t in got.items():
        assert torch.equal(t, torch.from_numpy(np.array(want[k]))), k
    for k, v in case["expand_kw"].items():
        assert getattr(model, k) == max(v, case["cfg"][k])
    assert model.get_graph_enc_dims()["el"] == 8


@pytest.mark.parametrize("option,exc", [
    (dict(pred_net="DIAMNet"), NotImplementedError),
    (dict(pred_net="MeanAttnPredictNet"), NotImplementedError),
    (dict(pred_net="NoSuchNet"), ValueError),
    (dict(emb_net="NoSuchEmbedding"), ValueError),
    (dict(enc_net="NoSuchEncoder"), NotImplementedError),
    (dict(filter_net="NoSuchFilter"), ValueError),
])
def test_unsupported_options_raise(option, exc):
    from dummynode4graphlearning_amd.subgraph_isomorphism import DMPNN
    with pytest.raises(exc):
        DMPNN(**dict(CASES["dmpnn"]["cfg"], **option))


def test_forward_has_no_cpu_path():
    from dummynode4graphlearning_amd._lib import DnHipError
    case = CASES["dmpnn"]
    model = R.build_model(case)
    with pytest.raises(DnHipError):
        model(R.make_graph(R.batch(case, "p"), "cpu"), R.make_graph(R.batch(case, "g"), "cpu"))


def test_v1_models_are_untouched_by_the_new_exports():
    from dummynode4graphlearning_amd import subgraph_isomorphism as si
    assert issubclass(si.CompGCN, si.GraphAdjModelV2) and issubclass(si.GraphAdjModelV2, si.GraphAdjModel)
    assert not issubclass(si.RGIN, si.GraphAdjModelV2)


def _check(tag, got, want, bad):
    e = R.rel_max(got, want)
    if not e < TOL:
        bad.append((tag, e))


@pytest.mark.parametrize("name", FORWARD)
def test_restatement_reproduces_the_golden_outputs_and_gradients(name):
    """The float64 restatement of the whole forward + backward gives every golden output, every parameter gradient (None pattern
    included), the gradients of the four rep tensors and the BatchNorm statistics the buffers were updated with."""
    case = CASES[name]
    a, cfg = case["arrays"], case["cfg"]
    sd = R.state_dict(case, "param")
    res = R.forward(sd, cfg, R.batch(case, "p"), R.batch(case, "g"), R.case_coefs(case))
    bad = []
    assert [k for k in R.OUT_KEYS if res[k] is None] == case["none_out"]
    for k in R.OUT_KEYS:
        if res[k] is None:
            continue
        if k.endswith("_mask"):
            assert torch.equal(res[k], torch.from_numpy(a["out/" + k])), k
        else:
            _check("out/" + k, res[k], a["out/" + k], bad)
    assert [k for k in case["params"] if res["grad"].get(k) is None] == case["none_grad"]
    for k in case["params"]:
        if res["grad"].get(k) is None:
            continue
        want = a["grad/" + k]
        if R.bn_shift(cfg, k):                                   # true gradient 0: see si_dual_model_ref.bn_shift
            scale = R.layer_weight_grad_scale(case, k)
            if not float(res["grad"][k].abs().max()) < 1e-4 * scale:
                bad.append((k, float(res["grad"][k].abs().max())))
            continue
        _check("grad/" + k, res["grad"][k], want, bad)
    assert [k for k in R.REPS if res["grad_rep"][k] is None] == case["none_rep"]
    for k in R.REPS:
        if res["grad_rep"][k] is not None:
            _check("grad_rep/" + k, res["grad_rep"][k], a["grad_rep/" + k], bad)
    running = {}                                                 # running = 0.9 * running + 0.1 * batch (unbiased var), in call order
    for mod, mean, var, rows in res["bn"]:
        m0, v0 = running.get(mod, (0.0, 1.0))
        running[mod] = (0.9 * m0 + 0.1 * mean, 0.9 * v0 + 0.1 * var * rows / (rows - 1))
    assert bool(running) == bool(cfg.get("rep_compgcn_batch_norm" if cfg["rep_net"] == "CompGCN" else "rep_dmpnn_batch_norm", False))
    for mod, (mean, var) in running.items():
        _check("after/" + mod + ".running_mean", mean, a["after/" + mod + ".running_mean"], bad)
        _check("after/" + mod + ".running_var", var, a["after/" + mod + ".running_var"], bad)
    assert not bad, bad


@pytest.mark.parametrize("name", FORWARD)
def test_restatement_outside_the_rep_nets(name):
    """Fed the goldens' four rep tensors, the glue alone (embeddings, masks, heads, mix) gives the goldens' predictions and the
    gradients into the rep tensors."""
    case = CASES[name]
    a = case["arrays"]
    reps = [a["out/" + k] for k in R.REPS]
    res = R.forward(R.state_dict(case, "param"), case["cfg"], R.batch(case, "p"), R.batch(case, "g"), R.case_coefs(case), reps=reps)
    bad = []
    for k in ("pred_c", "pred_v", "pred_e"):
        if res[k] is not None:
            _check(k, res[k], a["out/" + k], bad)
    for k in R.REPS:
        if k not in case["none_rep"]:
            _check("grad_rep/" + k, res["grad_rep"][k], a["grad_rep/" + k], bad)
    assert not bad, bad
