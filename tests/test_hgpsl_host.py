"""HGP-SL on the host (no GPU): the composed path on CPU tensors against the goldens of the reference's own hgpsl.py
(tests/golden/gc_hgpsl.npz: the same perm and edge list; outputs within 1e-4 of their maximum, gradients within 5e-4 of their
range, a gradient expected below 1e-5 stays below 1e-5), the float32 rule of k, the parameters' initial bits and names, the refusals,
and the GCN conv of the same file."""
import numpy as np
import pytest
import torch

import hgpsl_cases as C
import hgpsl_ref as R


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("tag", C.layer_tags())
def test_composed_layer_against_the_reference_golden(tag, dtype):
    errs = C.run_layer(tag, torch.device("cpu"), dtype)
    print(tag, {k: "%.1e" % v for k, v in errs.items()})


def test_composed_stack_against_the_reference_golden():
    errs = C.run_stack(torch.device("cpu"))
    print({k: "%.1e" % v for k, v in errs.items()})


def test_k_is_the_float32_ceiling():
    from dummynode4graphlearning_amd import ops
    assert ops.hgpsl_k(0.3, [50, 90, 100, 170]) == [16, 28, 31, 52]                  # the exact ceilings are 15, 27, 30, 51
    assert ops.hgpsl_k(0.3, [10, 20, 1, 0]) == [3, 6, 1, 0]
    assert ops.hgpsl_k(0.8, [1, 78, 80, 81, 1280, 1281]) == [1, 63, 64, 65, 1024, 1025]
    assert ops.hgpsl_k(1.0, [7, 64]) == [7, 64] and ops.hgpsl_k(0.5, []) == []
    for ratio in (0.3, 0.5, 0.8):
        sizes = list(range(0, 300))
        assert ops.hgpsl_k(ratio, sizes) == [R.k_of(ratio, n) for n in sizes]
    ptr = torch.tensor([0, 50, 140])
    index = ops.HgpslIndex(torch.tensor([0, 60]), torch.tensor([1, 61]), ptr, 140)
    pooled = index.pooled(0.3)
    assert pooled.ks == [16, 28] and pooled.ptr_host == [0, 16, 44] and pooled.blk_host == [0, 256, 256 + 784]


def test_init_bits_and_state_dict_keys():
    from dummynode4graphlearning_amd.graph_classification import HGPSLPool, hgpsl
    torch.manual_seed(11)
    layer = HGPSLPool(7, ratio=0.5, sparse=True)
    torch.manual_seed(11)
    att = torch.Tensor(1, 14)
    torch.nn.init.xavier_uniform_(att)
    assert torch.equal(layer.att.data, att) and list(layer.state_dict().keys()) == ["att"]
    torch.manual_seed(5)
    conv = hgpsl.GCN(4, 6)
    torch.manual_seed(5)
    wt = torch.Tensor(4, 6)
    torch.nn.init.xavier_uniform_(wt)
    assert torch.equal(conv.weight.data, wt) and torch.equal(conv.bias.data, torch.zeros(6))
    assert list(conv.state_dict().keys()) == ["weight", "bias"] and list(hgpsl.GCN(4, 6, bias=False).state_dict().keys()) == ["weight"]


def test_refusals():
    from dummynode4graphlearning_amd import _lib, ops
    from dummynode4graphlearning_amd.graph_classification import HGPSLPool
    with pytest.raises(NotImplementedError, match="sample"):
        HGPSLPool(4, sample=True)
    for ratio in (0, 1, 0.0, 1.5, -0.2, "0.5", None, True):
        with pytest.raises(ValueError, match="ratio"):
            HGPSLPool(4, ratio=ratio)
    HGPSLPool(4, ratio=1.0)
    ptr = torch.tensor([0, 3, 6])
    with pytest.raises(_lib.DnHipError, match="repeated"):
        ops.HgpslIndex(torch.tensor([0, 1, 0]), torch.tensor([1, 2, 1]), ptr, 6)
    with pytest.raises(_lib.DnHipError, match="joins two graphs"):
        ops.HgpslIndex(torch.tensor([0, 2]), torch.tensor([1, 3]), ptr, 6)
    with pytest.raises(_lib.DnHipError, match="outside the batch"):
        ops.HgpslIndex(torch.tensor([0, 2]), torch.tensor([1, 6]), ptr, 6)
    ops.HgpslIndex(torch.tensor([0, 1, 4]), torch.tensor([1, 0, 4]), ptr, 6)


def test_sl_false_returns_the_filtered_edges():
    from dummynode4graphlearning_amd.graph_classification import HGPSLPool
    z, metas = C.golden()
    t = lambda k: torch.from_numpy(z["soft_w/" + k])                                # noqa: E731
    layer = HGPSLPool(metas["soft_w"]["H"], ratio=0.8, sl=False)
    xo, ei, ea, b = layer(t("x"), t("edge_index"), t("edge_attr"), t("batch"))
    want = R.pool(t("x").double(), t("edge_index"), t("edge_attr").double(), t("ptr").tolist(), layer.att.detach().double(), 0.8, sl=False)
    assert torch.equal(ei, want["edge_index"]) and torch.equal(ea.double(), want["edge_attr"]) and torch.equal(b, want["batch"])
    assert torch.equal(xo, t("x")[want["perm"]])


def test_sparsemax_module_matches_the_restatement():
    from dummynode4graphlearning_amd.graph_classification import Sparsemax
    x = torch.tensor([1.7301, 0.6792, -1.0565, 1.6614, -0.3196, -0.7790, -0.3877, -0.4943, 0.1831, -0.0061], dtype=torch.float64,
                     requires_grad=True)
    batch = torch.tensor([0, 0, 0, 0, 1, 1, 1, 1, 1, 1])
    out = Sparsemax()(x, batch)
    want = torch.cat([R.sparsemax_rows(x.detach()[:4].view(1, -1))[0].view(-1), R.sparsemax_rows(x.detach()[4:].view(1, -1))[0].view(-1)])
    assert torch.allclose(out, want, atol=1e-12) and torch.allclose(out[:4].sum(), torch.tensor(1.0, dtype=torch.float64))
    g = torch.arange(10, dtype=torch.float64)
    out.backward(g)
    supp = out.detach() > 0
    exp = torch.zeros(10, dtype=torch.float64)
    for sl in (slice(0, 4), slice(4, 10)):
        s = supp[sl]
        exp[sl] = torch.where(s, g[sl] - g[sl][s].mean(), torch.zeros(1, dtype=torch.float64))
    assert torch.allclose(x.grad, exp, atol=1e-12)


def test_gcn_conv_against_its_golden():
    from dummynode4graphlearning_amd.graph_classification import hgpsl
    z, metas = C.golden()
    m = metas["stack"]
    t = lambda k: torch.from_numpy(z["stack/" + k])                                 # noqa: E731
    conv = hgpsl.GCN(m["H"], m["H"], cached=True)
    with torch.no_grad():
        conv.weight.copy_(t("init/conv2.weight"))
        conv.bias.copy_(t("init/conv2.bias") + 0.25)
    x = torch.from_numpy(np.random.default_rng(3).standard_normal((int(t("mid/edge_index").max()) + 1, m["H"])).astype(np.float32))
    got = conv(x, t("mid/edge_index"), t("mid/edge_attr"))
    want = R.gcn(x.double(), t("mid/edge_index"), t("mid/edge_attr").double(), conv.weight.detach().double(), conv.bias.detach().double())
    assert C.rel_max(got, want) < C.RTOL
    with pytest.raises(RuntimeError, match="Cached"):
        conv(x, t("mid/edge_index")[:, :-1], t("mid/edge_attr")[:-1])
