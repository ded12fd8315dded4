"""GPU tests of the SI count model HGT (subgraph_isomorphism/hgt.py) and its attention kernels (dn_hgt.hip).

* goldens: the reference's own HGT models and layers (tests/golden/si_hgt.npz), fp32, on the fused kernels and on the composed
  path: every OutputDict tensor, every parameter gradient (None for a_transform and the frozen tables), the rep gradients to
  RTOL = 1e-4 of the tensor's largest magnitude, masks exact (the bias in front of a BatchNorm: hgt_ref.bn_shift);
* op level (ops.hgt_message_pass) against the float64 restatement tests/hgt_ref.py at the smallest shapes that can still go wrong:
  in-degrees 0, 1, 63, 64, 65 and a hub of 300 in a 320-node graph, R in {1, 4}, (H, heads) in {(16, 4), (64, 4), (64, 1), (256, 8)},
  a duplicated edge and a self-loop edge, E = 0, N = 1, logits of about +-80, two graphs inside 64 edges;
* the fused forward and all its gradients are bitwise equal across two runs, fused and composed agree, and an unsupported dtype or
  width takes the composed path and matches.

The bound: the reference is float64 on the same fp32 inputs; the kernels sum at most 300 products per softmax and 256 per dot
product in fp32 (relative error ~ sqrt(n) 2^-24 < 2e-6 of the largest term), so 1e-4 of a tensor's largest magnitude -- the
project's bound against the fp32 goldens -- holds with room."""
import functools
import zlib

import numpy as np
import pytest
import torch

import hgt_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RTOL = 1e-4
CASES = R.load_golden()
MODELS = sorted(k for k, c in CASES.items() if c["kind"] == "model")
LAYERS = sorted(k for k, c in CASES.items() if c["kind"] == "layer")
PATHS = ["fused", "composed"]


def _path(name):
    from dummynode4graphlearning_amd import ops
    return ops.hgt_fused(name == "fused")


def _graph(d, dev=DEV):
    from dummynode4graphlearning_amd import BatchedGraph
    nd = {"id": torch.as_tensor(np.asarray(d["id"])).to(dev), "label": torch.as_tensor(np.asarray(d["label"])).to(dev)}
    if d.get("dummy") is not None:
        nd["is_dummy"] = torch.as_tensor(np.asarray(d["dummy"])).to(dev)
    return BatchedGraph(torch.as_tensor(np.asarray(d["u"])).to(dev), torch.as_tensor(np.asarray(d["v"])).to(dev),
                        int(np.sum(d["sizes"])), batch_num_nodes=torch.as_tensor(np.asarray(d["sizes"])),
                        ndata=nd, edata={"label": torch.as_tensor(np.asarray(d["elabel"])).to(dev)})


def _tags(fn):
    from dummynode4graphlearning_amd import ops
    with ops.KernelTimer() as timer:
        fn()
        return set(timer.summary())


# ------------------------------------------------------------------------------------------------ goldens
def _run_model(case, path):
    from dummynode4graphlearning_amd.subgraph_isomorphism import HGT
    torch.manual_seed(case["seed"])
    model = HGT(**case["cfg"])
    model.load_state_dict(R.state_dict(case, "param"))
    model = model.to(DEV).train()
    with _path(path):
        res = model(_graph(R.batch(case, "p")), _graph(R.batch(case, "g")))
        res["p_v_rep"].retain_grad()
        res["g_v_rep"].retain_grad()
        loss = (res["pred_c"] * R.loss_coef(case["B"], torch.float32, DEV)).sum()
        if res["pred_v"] is not None:
            loss = loss + (res["pred_v"] * torch.from_numpy(case["arrays"]["coef_v"]).to(DEV)).sum()
        loss.backward()
    return model, res


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", MODELS)
def test_model_matches_the_reference_goldens(name, path):
    case = CASES[name]
    a = case["arrays"]
    model, res = _run_model(case, path)
    assert list(res.keys()) == list(R.OUT_KEYS)
    assert [k for k in R.OUT_KEYS if res[k] is None] == case["none_out"]
    bad = []
    for k in R.OUT_KEYS:
        if res[k] is None:
            continue
        want = a["out/" + k]
        assert tuple(res[k].shape) == tuple(want.shape), k
        if res[k].dtype == torch.bool:
            assert torch.equal(res[k].cpu(), torch.from_numpy(want)), k
            continue
        e = R.rel_max(res[k], want)
        print("%s %s out %s rel_max %.3e" % (name, path, k, e))
        if not e < RTOL:
            bad.append((k, e))
    for k, got in (("p", res["p_v_rep"].grad), ("g", res["g_v_rep"].grad)):
        e = R.rel_max(got, a["grad_rep/" + k])
        print("%s %s grad_rep %s rel_max %.3e" % (name, path, k, e))
        if not e < RTOL:
            bad.append(("grad_rep/" + k, e))
    none_grad = [k for k, p in model.named_parameters() if p.grad is None]
    assert none_grad == case["none_grad"]
    assert any("a_transform" in k for k in none_grad) and any("enc_net" in k for k in none_grad)
    for k, p in model.named_parameters():
        if p.grad is None:
            continue
        e = R.grad_error(case, k, p.grad)
        print("%s %s grad %s rel_max %.3e" % (name, path, k, e))
        if not e < RTOL:
            bad.append((k, e))
    for k in case["buffers"]:
        if k in case["alias"]:
            continue
        got, want = model.state_dict()[k], a["after/" + k]
        if got.dtype.is_floating_point:
            e = R.rel_max(got, want)
            if not e < RTOL:
                bad.append(("after " + k, e))
        else:
            assert torch.equal(got.cpu(), torch.from_numpy(np.asarray(want)).to(got.dtype).reshape(got.shape)), k
    assert not bad, bad


def _run_layer(case, path, dtype=torch.float32):
    from dummynode4graphlearning_amd import BatchedGraph
    from dummynode4graphlearning_amd.subgraph_isomorphism import HeteroGraphTransLayer
    a, d = case["arrays"], case["dims"]
    layer = HeteroGraphTransLayer(d["H"], d["H"], num_node_types=d["T"], num_edge_types=d["R"], **case["kw"])
    layer.load_state_dict({k: torch.from_numpy(np.array(a["param/" + k])) for k in case["keys"]})
    layer = layer.to(DEV).to(dtype).train()
    t = lambda k: torch.from_numpy(np.asarray(a[k])).to(DEV)                                   # noqa: E731
    g = BatchedGraph(t("g/u"), t("g/v"), int(a["g/sizes"].sum()), batch_num_nodes=torch.from_numpy(a["g/sizes"]),
                     ndata={"label": t("g/label")}, edata={"label": t("g/elabel")})
    x = t("in/x").to(dtype).requires_grad_(True)
    with _path(path):
        y = layer(g, x)
        (y * t("in/coef").to(dtype)).sum().backward()
    return layer, x, y


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", LAYERS)
def test_layer_matches_the_reference_goldens(name, path):
    case = CASES[name]
    a = case["arrays"]
    layer, x, y = _run_layer(case, path)
    errs = [("out", R.rel_max(y, a["out/node_out"])), ("grad x", R.rel_max(x.grad, a["grad_in/x"]))]
    assert [k for k, p in layer.named_parameters() if p.grad is None] == case["none_grad"]
    errs += [("grad " + k, R.grad_error(case, k, p.grad)) for k, p in layer.named_parameters() if p.grad is not None]
    errs += [("after " + k, R.rel_max(layer.state_dict()[k], a["after/" + k])) for k in case["buffers"] if "num_batches" not in k]
    for k, e in errs:
        print("%s %s %s rel_max %.3e" % (name, path, k, e))
    assert not [(k, e) for k, e in errs if not e < RTOL], errs


def test_path_tags_show_which_attention_ran():
    case = CASES["bdd_b4_h2"]
    fused = {"hgt_attn_fwd", "hgt_attn_bwd_dst", "hgt_attn_bwd_src"}
    assert fused <= _tags(lambda: _run_model(case, "fused"))
    assert not fused & _tags(lambda: _run_model(case, "composed"))
    assert "rows_gemm" in _tags(lambda: _run_model(case, "composed"))                          # the typed products are HIP on both paths


def test_unsupported_dtype_takes_the_composed_path_and_matches():
    """float64 rows: nothing of dn_hgt.hip (fp32 only) or of the fp32 / bf16 product kernels runs, the result is the restatement's."""
    case = CASES["layer_bdd_h2_leaky"]
    a = case["arrays"]
    box = {}
    tags = _tags(lambda: box.update(r=_run_layer(case, "fused", torch.float64)))
    assert not {"hgt_attn_fwd", "hgt_attn_bwd_dst", "hgt_attn_bwd_src"} & tags
    layer, x, y = box["r"]
    want_y, want_gx, want_g = R.run_layer_case(case)
    assert y.dtype == torch.float64 and R.rel_max(y, want_y) < 1e-10 and R.rel_max(x.grad, want_gx) < 1e-10
    for k, p in layer.named_parameters():
        assert (p.grad is None) == (want_g[k] is None), k
        if p.grad is not None:
            assert R.rel_max(p.grad, want_g[k]) < 1e-10, k
    assert R.rel_max(y, a["out/node_out"]) < RTOL


# ------------------------------------------------------------------------------------------------ op level
def _zoo(R_):
    """One 320-node graph: in-degrees 0 (node 0), 1, 63, 64, 65 (nodes 1-4), a hub of 300 (node 5), 0-6 elsewhere; the edge 7 -> 8 of
    type 0 twice, the self-loop 9 -> 9."""
    rng = np.random.default_rng(50 + R_)
    N = 320
    deg = rng.integers(0, 7, size=N)
    deg[:6] = [0, 1, 63, 64, 65, 300]
    dst = np.repeat(np.arange(N), deg)
    src = rng.integers(0, N, size=len(dst))
    et = rng.integers(0, R_, size=len(dst))
    src = np.concatenate([src, [7, 7, 9]])
    dst = np.concatenate([dst, [8, 8, 9]])
    et = np.concatenate([et, [0, 0, R_ - 1]])
    order = rng.permutation(len(src))                                                          # edge ids in no particular order
    return N, src[order], dst[order], et[order]


def _two_graphs(R_):
    """Two graphs (3 and 4 nodes) whose 5 + 7 edges all lie inside one wavefront's worth (64) of edges."""
    src = np.array([0, 1, 2, 2, 0, 3, 4, 5, 6, 3, 5, 4])
    dst = np.array([1, 2, 0, 1, 0, 4, 5, 6, 3, 5, 3, 4])
    return 7, src, dst, np.arange(12) % R_


GRAPHS = {"zoo": _zoo, "two_graphs": _two_graphs,
          "no_edges": lambda R_: (5, np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.int64)),
          "one_node_loop": lambda R_: (1, np.array([0, 0]), np.array([0, 0]), np.array([0, R_ - 1])),
          "one_node_alone": lambda R_: (1, np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.int64))}
OP_CASES = [("zoo", R_, H, heads, 1.0) for R_ in (1, 4) for H, heads in ((16, 4), (64, 4), (64, 1), (256, 8))]
OP_CASES += [(g, 4, 64, 4, 1.0) for g in ("two_graphs", "no_edges", "one_node_loop", "one_node_alone")]
OP_CASES += [("zoo", 4, 64, 4, 80.0), ("two_graphs", 1, 16, 4, 80.0)]                           # logits of about +-80
NAMES = ("agg", "dq", "dk", "dv", "datt", "dmsg", "dpri")


@functools.lru_cache(maxsize=None)
def _op_case(graph, R_, H, heads, logit_scale):
    """Inputs (fp32, CPU) and the float64 restatement's outputs and gradients, computed once per case."""
    N, src, dst, et = GRAPHS[graph](R_)
    rng = np.random.default_rng(zlib.crc32(repr((graph, R_, H, heads)).encode()))
    dk = H // heads
    f = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(np.float32))                 # noqa: E731
    q, k, v, coef = f(N, H), f(N, H), f(N, H), f(N, H)
    att, msg = f(R_, heads, dk, dk) / dk ** 0.5, f(R_, heads, dk, dk) / dk ** 0.5
    pri = 1.0 + 0.3 * f(R_, heads)
    scale = float(dk) ** -0.5
    src, dst, et = (torch.from_numpy(np.asarray(t, np.int64)) for t in (src, dst, et))
    if logit_scale != 1.0 and len(src):                                                        # q scaled so that max |logit| is logit_scale
        with torch.no_grad():
            e = (q.view(N, heads, dk)[dst].double() * torch.einsum("bij,bijk->bik", k.view(N, heads, dk)[src].double(), att[et].double()))
            q = (q * (logit_scale / float((e.sum(-1) * pri[et] * scale).abs().max()))).float()
    ins = (q, k, v, att, msg, pri)
    leaves = [t.double().requires_grad_(True) for t in ins]
    agg, a = R.attention(*leaves, scale, src, dst, et)
    (agg * coef.double()).sum().backward()
    if logit_scale != 1.0 and graph == "zoo":
        lg = torch.log(a.detach().clamp(min=1e-300))
        assert float((lg.max() - lg.min())) > 40                                               # the softmax really spans e^40: max subtraction matters
    return dict(N=N, src=src, dst=dst, et=et, ins=ins, coef=coef, scale=scale, want=[agg.detach()] + [t.grad for t in leaves])


def _run_op(c, R_, path):
    from dummynode4graphlearning_amd import ops
    ix = ops.HgtIndex(c["src"].to(DEV), c["dst"].to(DEV), c["et"].to(DEV), c["N"], R_)
    leaves = [t.to(DEV).requires_grad_(True) for t in c["ins"]]
    with _path(path):
        agg = ops.hgt_message_pass(*leaves, ix, c["scale"])
        (agg * c["coef"].to(DEV)).sum().backward()
    return [agg.detach()] + [t.grad if t.grad is not None else torch.zeros_like(t) for t in leaves]


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("graph,R_,H,heads,logit_scale", OP_CASES)
def test_op_matches_the_float64_restatement(graph, R_, H, heads, logit_scale, path):
    c = _op_case(graph, R_, H, heads, logit_scale)
    box = {}
    tags = _tags(lambda: box.update(got=_run_op(c, R_, path)))
    assert ("hgt_attn_fwd" in tags) == (path == "fused")                                        # no fall-back at any of these shapes
    got = box["got"]
    errs = {}
    for name, g, w in zip(NAMES, got, c["want"]):
        assert torch.isfinite(g).all(), name
        if float(w.abs().max()) == 0.0:                                                         # (no edges: every result is exactly zero)
            assert float(g.abs().max()) == 0.0, name
            continue
        errs[name] = R.rel_max(g, w)
    print(graph, R_, H, heads, logit_scale, path, {k: "%.2e" % e for k, e in errs.items()})
    assert all(e < RTOL for e in errs.values()), errs


def test_fused_and_composed_agree():
    c = _op_case("zoo", 4, 64, 4, 1.0)
    for name, a, b, w in zip(NAMES, _run_op(c, 4, "fused"), _run_op(c, 4, "composed"), c["want"]):
        assert float((a - b).abs().max()) < RTOL * float(w.abs().max()), name


@pytest.mark.parametrize("graph,R_,H,heads", [("zoo", 4, 64, 4), ("zoo", 1, 256, 8), ("two_graphs", 4, 16, 4)])
def test_fused_runs_are_bitwise_equal(graph, R_, H, heads):
    c = _op_case(graph, R_, H, heads, 1.0)
    one, two = _run_op(c, R_, "fused"), _run_op(c, R_, "fused")
    for name, a, b in zip(NAMES, one, two):
        assert torch.equal(a, b), name


def test_model_runs_are_bitwise_equal_on_the_fused_path():
    outs = []
    for _ in range(2):
        model, res = _run_model(CASES["bdd_b4_h2"], "fused")
        outs.append([res["pred_c"].detach().clone(), res["p_v_rep"].grad.clone(), res["g_v_rep"].grad.clone()] +
                    [p.grad.clone() for _, p in model.named_parameters() if p.grad is not None])
    assert all(torch.equal(x, y) for x, y in zip(*outs))


def test_unsupported_width_takes_the_composed_path_and_matches():
    """d_k = 6 is no multiple of 4: the fused predicate declines, the composed path serves the shape."""
    from dummynode4graphlearning_amd import ops
    assert not ops.hgt_fused_supported(torch.zeros(1, 24, device=DEV), 4) and ops.hgt_fused_supported(torch.zeros(1, 24, device=DEV), 2)
    c = _op_case("two_graphs", 4, 24, 4, 1.0)
    box = {}
    tags = _tags(lambda: box.update(got=_run_op(c, 4, "fused")))
    assert "hgt_attn_fwd" not in tags
    for name, g, w in zip(NAMES, box["got"], c["want"]):
        assert R.rel_max(g, w) < RTOL, name


def test_bad_edge_types_raise():
    from dummynode4graphlearning_amd import ops
    from dummynode4graphlearning_amd._lib import DnHipError
    t = lambda *v: torch.tensor(v, device=DEV)                                                  # noqa: E731
    with pytest.raises(DnHipError, match="edge type"):
        ops.HgtIndex(t(0, 1), t(1, 0), t(0, 4), 2, 4)
    with pytest.raises(DnHipError, match="node type"):
        ops.TypeIndex(t(0, 5), 5)
