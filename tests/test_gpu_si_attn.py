"""GPU tests of the attention count heads and DIAMNet on the ragged path (graph_adj.attn_head_ragged on ops.seg_attention /
ops.seg_window_pool) against the goldens of the reference's own pred.py and models (tests/golden/si_attn.npz), on both paths:
the fused kernels and `ops.attn_fused(False)`.  Every tensor to 1e-4 of its largest magnitude, masks exact, None lists identical."""
import numpy as np
import pytest
import torch

import seg_attn_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RTOL = 1e-4
CASES = R.load_golden()
RAGGED_HEADS = sorted(n for n, c in CASES.items() if c["kind"] == "head" and not c["has_w"])
WEIGHT_HEADS = sorted(n for n, c in CASES.items() if c["kind"] == "head" and c["has_w"])
MODELS = sorted(n for n, c in CASES.items() if c["kind"] == "model")
FUSED_TAGS = {"seg_attn_fwd", "seg_attn_bwd_q", "seg_attn_bwd_kv"}


def _tags(fn):
    from dummynode4graphlearning_amd import ops
    with ops.KernelTimer() as timer:
        res = fn()
        return res, set(timer.summary())


def _head(case):
    from dummynode4graphlearning_amd.subgraph_isomorphism import attn_pred
    net = getattr(attn_pred, case["cls"])(case["input_dim"], **case["kw"])
    net.load_state_dict({k: torch.from_numpy(np.array(case["arrays"]["param/" + k])) for k in case["keys"]})
    return net.to(DEV).train()


def _ragged_side(x, mask):
    """The pre-padded golden rows [B, L, D] / mask as ragged rows: every pair keeps its rows from the first unmasked position on (a
    masked row behind it is a dummy row).  Returns (rows, ptr, skip, L, count, index of the kept padded slots)."""
    B, L = mask.shape
    keep = torch.zeros_like(mask)
    for b in range(B):
        keep[b, int(torch.nonzero(mask[b])[0]):] = True
    flat = torch.nonzero(keep.reshape(-1)).view(-1)
    lens = keep.sum(1)
    ptr = torch.tensor([0] + list(np.cumsum(lens.numpy())), dtype=torch.int32)
    return x.reshape(B * L, -1)[flat], ptr, ~mask.reshape(-1)[flat], L, mask.sum(1), flat


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("name", RAGGED_HEADS)
def test_ragged_head_matches_the_reference(name, fused):
    from dummynode4graphlearning_amd import ops
    from dummynode4graphlearning_amd.subgraph_isomorphism.graph_adj import attn_head_ragged
    case = CASES[name]
    a = case["arrays"]
    net = _head(case)
    sides = []
    for s in ("p", "g"):
        rows, ptr, skip, L, cnt, flat = _ragged_side(torch.from_numpy(np.array(a["in/" + s])), torch.from_numpy(a["in/%s_mask" % s]))
        sides.append((rows.to(DEV).requires_grad_(True), ptr.to(DEV), skip.to(DEV), L, cnt.to(DEV), flat))
    (pr, pp, ps, Lp, pc, pf), (gr, gp, gs, Lg, gc, gf) = sides

    def run():
        with ops.attn_fused(fused):
            y = attn_head_ragged(net, pr, pp, ps, Lp, pc, gr, gp, gs, Lg, gc)
            (y * torch.from_numpy(np.array(a["in/coef"])).to(DEV)).sum().backward()
        return y
    y, tags = _tags(run)
    assert (FUSED_TAGS <= tags) == fused and bool(tags & FUSED_TAGS) == fused, tags
    if case["cls"] == "DIAMNet":
        assert ("seg_window_pool" in tags) == fused and ("seg_window_pool_bwd" in tags) == fused
    # (the gradient of a masked row is compared nowhere: the models clear those rows in front of the head, which drops it)
    pl, gl = (~ps).cpu().numpy(), (~gs).cpu().numpy()
    checks = [("y", y, a["out/y"]), ("grad p", pr.grad[~ps], a["grad_in/p"].reshape(-1, case["input_dim"])[pf.numpy()][pl]),
              ("grad g", gr.grad[~gs], a["grad_in/g"].reshape(-1, case["input_dim"])[gf.numpy()][gl])]
    assert [k for k, q in net.named_parameters() if q.grad is None] == case["none_grad"]
    checks += [("grad " + k, q.grad, a["grad/" + k]) for k, q in net.named_parameters() if q.grad is not None]
    bad = []
    for tag, got, want in checks:
        e = R.rel_max(got, want)
        print("%s %s %s rel_max %.3e" % (name, fused, tag, e))
        if not e < RTOL:
            bad.append((tag, e))
    assert not bad, bad


@pytest.mark.parametrize("name", WEIGHT_HEADS)
def test_padded_head_with_weights_on_the_device(name):
    case = CASES[name]
    a = case["arrays"]
    net = _head(case)
    t = lambda k: torch.from_numpy(np.array(a[k])).to(DEV)   # noqa: E731
    y, w = net(t("in/p"), t("in/p_mask"), t("in/g"), t("in/g_mask"))
    assert R.rel_max(y, a["out/y"]) < RTOL and R.rel_max(w, a["out/w"]) < RTOL


def _model(case):
    from dummynode4graphlearning_amd import subgraph_isomorphism as SI
    cfg = dict(case["cfg"])
    pred_net = cfg.pop("pred_net")
    model = getattr(SI, case["cls"])(**cfg)
    model.set_pred_net(pred_net, **cfg)
    sd = {k: torch.from_numpy(np.array(case["arrays"]["param/" + case["alias"].get(k, k)])) for k in case["keys"]}
    model.load_state_dict(sd, strict=True)
    return model.to(DEV).train()


def _graphs(case):
    a = case["arrays"]
    if case["cls"] == "DMPNN":
        import si_dual_model_ref as D
        return [D.make_graph(D.batch(case, s), DEV) for s in ("p", "g")]
    from dummynode4graphlearning_amd import BatchedGraph
    t = lambda x: torch.as_tensor(np.asarray(x)).to(DEV)     # noqa: E731
    out = []
    for s in ("p", "g"):
        d = {k: a["%s/%s" % (s, k)] for k in ("sizes", "u", "v", "id", "label", "elabel")}
        nd = {"id": t(d["id"]), "label": t(d["label"])}
        if a.get("%s/dummy" % s) is not None:
            nd["is_dummy"] = t(a["%s/dummy" % s])
        out.append(BatchedGraph(t(d["u"]), t(d["v"]), int(np.sum(d["sizes"])), batch_num_nodes=torch.as_tensor(np.asarray(d["sizes"])),
                                ndata=nd, edata={"label": t(d["elabel"])}))
    return out


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("name", MODELS)
def test_whole_model_matches_the_reference(name, fused):
    from dummynode4graphlearning_amd import ops
    case = CASES[name]
    a = case["arrays"]
    model = _model(case)
    pg, gg = _graphs(case)

    def run():
        with ops.attn_fused(fused), ops.f32_exact(True):
            res = model(pg, gg)
            c = torch.arange(1, case["B"] + 1, dtype=torch.float32, device=DEV).view(-1, 1) / case["B"]
            (res["pred_c"] * c).sum().backward()
        return res
    res, tags = _tags(run)
    assert bool(tags & FUSED_TAGS) == fused and "si_head_padded" not in tags, tags
    assert [k for k in res.keys() if res[k] is None] == case["none_out"]
    bad = []
    for k in res.keys():
        if res[k] is None:
            continue
        want = a["out/" + k]
        assert tuple(res[k].shape) == tuple(want.shape), k
        if res[k].dtype == torch.bool:
            assert torch.equal(res[k].cpu(), torch.from_numpy(want)), k
            continue
        e = R.rel_max(res[k], want)
        print("%s %s out %s rel_max %.3e" % (name, fused, k, e))
        if not e < RTOL:
            bad.append((k, e))
    assert [k for k, p in model.named_parameters() if p.grad is None] == case["none_grad"]
    for k, p in model.named_parameters():
        if p.grad is None:
            continue
        e = R.rel_max(p.grad, a["grad/" + k])
        print("%s %s grad %s rel_max %.3e" % (name, fused, k, e))
        if not e < RTOL:
            bad.append((k, e))
    assert not bad, bad


def test_fused_head_runs_are_bitwise_equal():
    case = CASES["rgin_diamnet"]
    pg, gg = _graphs(case)
    outs = []
    for _ in range(2):
        model = _model(case)
        res = model(pg, gg)
        res["pred_c"].sum().backward()
        outs.append([res["pred_c"].detach().clone()] + [p.grad.clone() for p in model.parameters() if p.grad is not None])
    assert all(torch.equal(x, y) for x, y in zip(*outs))
