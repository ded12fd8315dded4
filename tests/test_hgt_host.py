"""Host tests of the SI count model HGT (subgraph_isomorphism/hgt.py): no GPU.

* the float64 restatement tests/hgt_ref.py reproduces every layer golden of the reference (tests/golden/si_hgt.npz) to
  RTOL = 1e-4 of each tensor's largest magnitude (the bound of test_gpu_si_model.py / test_gpu_lrp.py), the None pattern of the
  parameter gradients included (the bias in front of a BatchNorm, whose true gradient is zero: hgt_ref.bn_shift);
* HGT(**cfg) / HeteroGraphTransLayer have the goldens' state_dict keys in the goldens' order and bit-equal initial values under
  the recorded seed;
* the five regularisers densify to the weights the reference's DecompMultiTransform.forward applies."""
import hashlib

import numpy as np
import pytest
import torch

import hgt_ref as R

RTOL = 1e-4
CASES = R.load_golden()
MODELS = sorted(k for k, c in CASES.items() if c["kind"] == "model")
LAYERS = sorted(k for k, c in CASES.items() if c["kind"] == "layer")


def _sha(t):
    return hashlib.sha256(t.detach().contiguous().numpy().tobytes()).hexdigest()[:24]


def test_the_golden_file_holds_the_cases_the_model_is_checked_on():
    assert len(MODELS) == 15 and len(LAYERS) == 5
    regs = {(c["cfg"].get("rep_hgt_regularizer"), c["cfg"].get("rep_hgt_num_bases", -1) > 0) for c in (CASES[k] for k in MODELS)}
    assert {(r, True) for r in ("none", "basis", "bdd", "diag", "scalar")} <= regs and (None, False) in regs
    assert {CASES[k]["cfg"].get("rep_hgt_num_heads", 4) for k in MODELS} == {1, 2, 4}
    a = CASES[LAYERS[0]]["arrays"]
    u, v, et = a["g/u"], a["g/v"], a["g/elabel"]
    indeg = np.bincount(v, minlength=int(a["g/sizes"].sum()))
    assert (indeg == 0).any() and (indeg == 1).any() and (u == v).any()                        # no in-edge, one in-edge, a self-loop
    assert len({(x, y, t) for x, y, t in zip(u, v, et)}) < len(u)                                 # a multi-edge


@pytest.mark.parametrize("name", LAYERS)
def test_restatement_reproduces_the_layer_goldens(name):
    case = CASES[name]
    a = case["arrays"]
    y, gx, grads = R.run_layer_case(case)
    assert [k for k in case["params"] if grads[k] is None] == case["none_grad"]
    assert all(k.startswith("a_transform.") for k in case["none_grad"]) and case["none_grad"]
    errs = [("out", R.rel_max(y, a["out/node_out"])), ("grad x", R.rel_max(gx, a["grad_in/x"]))]
    errs += [("grad " + k, R.grad_error(case, k, g)) for k, g in grads.items() if g is not None]
    bad = []
    for k, e in errs:
        print("%s %s rel_max %.3e" % (name, k, e))
        if not e < RTOL:
            bad.append((k, e))
    assert not bad, bad


@pytest.mark.parametrize("name", MODELS)
def test_model_state_dict_keys_and_initial_values(name):
    from dummynode4graphlearning_amd.subgraph_isomorphism import HGT
    case = CASES[name]
    torch.manual_seed(case["seed"])
    model = HGT(**case["cfg"])
    sd = model.state_dict()
    assert list(sd.keys()) == case["keys"]
    assert [k for k, _ in model.named_parameters()] == case["params"]
    assert {k: list(t.shape) for k, t in sd.items()} == case["shapes"]
    assert {k: _sha(t) for k, t in sd.items()} == case["init_sha"]
    if "init/" + case["keys"][0] in case["arrays"]:
        for k, t in R.state_dict(case, "init").items():
            assert torch.equal(sd[k], t), k
    model.load_state_dict(R.state_dict(case, "param"))


def test_default_config_has_dense_per_type_weights():
    """rep_hgt_regularizer defaults to "diag" but num_bases -1 turns every transform into "none" (hgt.py:22-25)."""
    from dummynode4graphlearning_amd.subgraph_isomorphism import HGT
    case = CASES["default"]
    cfg = case["cfg"]
    assert "rep_hgt_regularizer" not in cfg and "rep_hgt_num_bases" not in cfg
    layer = list(HGT(**cfg).g_rep_net["hgt"])[0]
    assert layer.regularizer == "diag" and layer.num_heads == 4 and layer.q_transform.regularizer == "none"
    assert tuple(layer.q_transform.weights["weight"].shape) == (cfg["max_ngvl"], cfg["hid_dim"] ** 2)


@pytest.mark.parametrize("name", LAYERS)
def test_layer_state_dict_keys_and_initial_values(name):
    from dummynode4graphlearning_amd.subgraph_isomorphism import HeteroGraphTransLayer
    case = CASES[name]
    d = case["dims"]
    torch.manual_seed(case["seed"])
    layer = HeteroGraphTransLayer(d["H"], d["H"], num_node_types=d["T"], num_edge_types=d["R"], **case["kw"])
    assert list(layer.state_dict().keys()) == case["keys"]
    assert [k for k, _ in layer.named_parameters()] == case["params"]
    assert {k: _sha(t) for k, t in layer.state_dict().items()} == case["init_sha"]


@pytest.mark.parametrize("regularizer,num_bases", [("none", 2), ("basis", 2), ("bdd", 4), ("diag", 3), ("scalar", 2), ("diag", -1), ("bdd", 0)])
def test_regularisers_densify_to_the_weights_the_reference_applies(regularizer, num_bases):
    from dummynode4graphlearning_amd.subgraph_isomorphism import DecompMultiTransform
    T, D, n = 5, 16, 40
    torch.manual_seed(3)
    tr = DecompMultiTransform(D, D, T, regularizer, num_bases).double()
    assert tr.regularizer == R.effective_regularizer(regularizer, num_bases)
    rng = np.random.default_rng(4)
    x = torch.from_numpy(rng.standard_normal((n, D)))
    xtype = torch.from_numpy(rng.integers(0, T, size=n))
    want = R.decomp_apply(regularizer, num_bases, {k: v.detach() for k, v in tr.weights.items()}, x, xtype, D, D)
    dense = tr.dense_weights()
    assert tuple(dense.shape) == (T, D, D)
    got = torch.bmm(x.unsqueeze(1), dense[xtype]).squeeze(1)
    assert R.rel_max(got, want) < 1e-12
    assert R.rel_max(tr(x, xtype), want) < 1e-12                                                  # the module's own CPU path
    # the gradient reaches every parameter of the decomposition through the dense form
    (got * torch.from_numpy(rng.standard_normal((n, D)))).sum().backward()
    assert all(p.grad is not None and p.grad.abs().sum() > 0 for p in tr.parameters())


def test_fused_switch_is_thread_local():
    from dummynode4graphlearning_amd import ops
    assert ops.hgt_fused_enabled() == ops.HGT_FUSED_DEFAULT
    with ops.hgt_fused():
        assert ops.hgt_fused_enabled()
        with ops.hgt_fused(False):
            assert not ops.hgt_fused_enabled()
        assert ops.hgt_fused_enabled()
    assert ops.hgt_fused_enabled() == ops.HGT_FUSED_DEFAULT
    x = torch.zeros(3, 24)
    assert not ops.hgt_fused_supported(x, 2)                                                      # not on the GPU
