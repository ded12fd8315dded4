"""GPU parity of the SI nn.Module surface (RGINLayer / RGCNLayer / rep nets / dual layers / predict nets) against the golden
vectors captured from the reference's own layers and against the oracle restatement (GC models: test_gpu_gc_models.py).

Tolerance (north_star): fp32 layer outputs within 1e-4 relative of the reference.  Relative error is measured
against the tensor's max magnitude (rel_max = max|a-b| / max|b|), gradients included."""
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import layers as OL

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RTOL = 1e-4


def _rel_max(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp(min=1e-12))


def _rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp(min=1e-12))


def _cases(golden_dir):
    z = np.load(os.path.join(golden_dir, "si_layers.npz"))
    return z, json.loads(bytes(z["meta"]).decode())


def _build(m):
    from dummynode4graphlearning_amd.subgraph_isomorphism import RGCNLayer, RGINLayer
    kw = dict(num_rels=m["num_rels"], regularizer=m["regularizer"], num_bases=m["num_bases"],
              self_loop=m["self_loop"], act_func=m["act_func"])
    if m["kind"] == "rgin":
        return RGINLayer(m["input_dim"], m["hidden_dim"], num_mlp_layers=m["num_mlp_layers"], batch_norm=bool(m.get("batch_norm", False)), **kw)
    return RGCNLayer(m["input_dim"], m["hidden_dim"], edge_norm=m["edge_norm"], batch_norm=bool(m.get("batch_norm", False)), **kw)


@pytest.mark.parametrize("exact", [False, True])
def test_si_layers_match_reference_goldens(golden_dir, exact):
    """48 + 2 reference-run cases (outputs + every gradient) at 1e-4, in both fp32 arithmetic modes of the matrix kernels:
    the default 3-term bf16 split (fast MFMA path) and the exact-f32 MFMA checker.  Includes the benchmark width H = 256."""
    from dummynode4graphlearning_amd import BatchedGraph, ops
    z, meta = _cases(golden_dir)
    assert any(m["hidden_dim"] == 256 for m in meta)
    worst = 0.0
    old_mode = ops.F32_EXACT
    ops.F32_EXACT = exact
    try:
        worst = _run_si_goldens(z, meta, BatchedGraph)
    finally:
        ops.F32_EXACT = old_mode
    print("fp32 mode %s: worst rel_max over %d golden cases: %.3e" % ("exact" if exact else "bf16x3 split", len(meta), worst))
    assert worst < (5e-6 if exact else RTOL)


def test_si_layers_with_batch_norm_and_other_activations_match_reference_goldens(golden_dir):
    """si_layers_bn.npz (round 6, reference-run): RGINLayer / RGCNLayer with batch_norm=True (--rep_rgin_batch_norm, rgin.py:50-57;
    --rep_rgcn_batch_norm, rgcn.py:52-53) in training mode and the activations gelu / selu / elu at a matrix-core width, at 1e-4: outputs, every gradient, the BatchNorm buffers after the step.
    Path: the BatchNorm (and a ReLU behind it) runs on the HIP BatchNorm kernels, the Linears on the MFMA Linear kernels."""
    from dummynode4graphlearning_amd import BatchedGraph, ops
    z = np.load(os.path.join(golden_dir, "si_layers_bn.npz"))
    meta = json.loads(bytes(z["meta"]).decode())
    calls = {"bn": 0, "lin": 0}
    orig_bn, orig_lin = ops.batch_norm_rows, ops.linear_act
    ops.batch_norm_rows = lambda *a, **k: (calls.__setitem__("bn", calls["bn"] + 1), orig_bn(*a, **k))[1]
    ops.linear_act = lambda *a, **k: (calls.__setitem__("lin", calls["lin"] + 1), orig_lin(*a, **k))[1]
    worst = 0.0
    try:
        for m in meta:
            tag = m["tag"]
            before = dict(calls)
            layer = _build(m)
            sd = {k[len(tag) + 7:]: torch.from_numpy(z[k]) for k in z.files if k.startswith(tag + "/param/")}
            missing = layer.load_state_dict(sd, strict=False)            # (the buffers start from torch's defaults, as the reference's did)
            assert not missing.unexpected_keys and all("running_" in k or "num_batches" in k for k in missing.missing_keys), missing
            layer = layer.to(DEV).train()
            u, v, t = (torch.from_numpy(z[tag + "/" + k]).to(DEV) for k in ("u", "v", "t"))
            g = BatchedGraph(u, v, m["N"])
            x = torch.from_numpy(z[tag + "/x"]).to(DEV).requires_grad_(True)
            out, _ = layer(g, x, t)
            if m["batch_norm"]:
                assert calls["bn"] == before["bn"] + 1, (tag, "BatchNorm did not take the HIP kernels")
                if m["hidden_dim"] in (64, 128) and m["kind"] == "rgin":
                    assert calls["lin"] == before["lin"] + 2, (tag, "the Linears did not take the MFMA kernels")
            (out * torch.from_numpy(z[tag + "/coef"]).to(DEV)).sum().backward()
            errs = {"out": _rel_max(out, torch.from_numpy(z[tag + "/out"])), "grad_x": _rel_max(x.grad, torch.from_numpy(z[tag + "/grad_x"]))}
            scale = max(float(np.abs(z[tag + "/grad/" + k]).max()) for k, _ in layer.named_parameters() if z[tag + "/grad/" + k].size)
            for k, p in layer.named_parameters():
                ref = z[tag + "/grad/" + k]
                if ref.size and np.abs(ref).max() > 1e-5 * scale:
                    errs["grad " + k] = _rel_max(p.grad, torch.from_numpy(ref))
                elif ref.size:                                           # a shift in front of a BatchNorm (the conv's bias, mlp.0.bias): the
                    assert float(p.grad.abs().max()) < 1e-4 * scale, (tag, k)   # gradient is zero up to rounding noise on either side
            for k, b in layer.named_buffers():
                errs["buffer " + k] = _rel_max(b.float(), torch.from_numpy(z[tag + "/buffer/" + k]).float())
            for k, e in errs.items():
                assert e < RTOL, "%s %s rel_max %.3e" % (tag, k, e)
                worst = max(worst, e)
    finally:
        ops.batch_norm_rows, ops.linear_act = orig_bn, orig_lin
    assert calls["bn"] >= 9
    print("worst rel_max over %d BatchNorm / activation golden cases: %.3e" % (len(meta), worst))


def _run_si_goldens(z, meta, BatchedGraph):
    """... and WHICH path ran: every rgin case with relu / leaky_relu (the reference CLI's default, config.py:329-335) and a
    matrix-core width must take the fused Linear + activation kernels (ops.relu_mlp), every bdd case (the CLI's default
    regulariser, config.py:145-158) the one-launch block-diagonal composition (ops.bdd_dense)."""
    from dummynode4graphlearning_amd import ops
    worst = 0.0
    calls = {"mlp": 0, "bdd": 0}
    orig_mlp, orig_bdd, orig_layer = ops.relu_mlp, ops.bdd_dense, ops.rgin_layer_f32
    ops.relu_mlp = lambda *a, **k: (calls.__setitem__("mlp", calls["mlp"] + 1), orig_mlp(*a, **k))[1]
    ops.bdd_dense = lambda *a, **k: (calls.__setitem__("bdd", calls["bdd"] + 1), orig_bdd(*a, **k))[1]
    # (H = 64 / 128 with a self loop and a two-layer MLP: the whole layer as ONE function on the same kernels -- ops.rgin_layer_f32)
    ops.rgin_layer_f32 = lambda *a, **k: (calls.__setitem__("mlp", calls["mlp"] + 1), calls.__setitem__("layer", calls.get("layer", 0) + 1),
                                          orig_layer(*a, **k))[2]
    try:
        worst = _run_si_goldens_inner(z, meta, BatchedGraph, calls)
    finally:
        ops.relu_mlp, ops.bdd_dense, ops.rgin_layer_f32 = orig_mlp, orig_bdd, orig_layer
    assert ops.f32_mode() or calls.get("layer", 0) > 0, "no golden case took the one-function fp32 layer"
    return worst


def _run_si_goldens_inner(z, meta, BatchedGraph, calls):
    worst = 0.0
    seen = {"leaky_fused": 0, "bdd": 0}
    for m in meta:
        tag = m["tag"]
        before = dict(calls)
        layer = _build(m)
        sd = {k[len(tag) + 7:]: torch.from_numpy(z[k]) for k in z.files if k.startswith(tag + "/param/")}
        layer.load_state_dict(sd, strict=True)                       # same names and shapes as the reference
        layer = layer.to(DEV).train()
        u, v, t = (torch.from_numpy(z[tag + "/" + k]).to(DEV) for k in ("u", "v", "t"))
        g = BatchedGraph(u, v, m["N"])
        x = torch.from_numpy(z[tag + "/x"]).to(DEV).requires_grad_(True)
        out, et = layer(g, x, t)
        assert et is t
        if (m["kind"] == "rgin" and m["act_func"] in ("relu", "leaky_relu") and m["num_mlp_layers"] > 0
                and m["hidden_dim"] in (64, 128, 256)):
            assert calls["mlp"] == before["mlp"] + 1, (tag, "the MLP did not take the fused Linear + activation kernels")
            seen["leaky_fused"] += m["act_func"] == "leaky_relu"
        if m["regularizer"] == "bdd":
            assert calls["bdd"] == before["bdd"] + 1, (tag, "bdd weights were not composed by dn_bdd_compose")
            seen["bdd"] += 1
        (out * torch.from_numpy(z[tag + "/coef"]).to(DEV)).sum().backward()
        errs = {"out": _rel_max(out, torch.from_numpy(z[tag + "/out"])),
                "grad_x": _rel_max(x.grad, torch.from_numpy(z[tag + "/grad_x"]))}
        for k, p in layer.named_parameters():
            ref = z[tag + "/grad/" + k]
            if ref.size and np.abs(ref).max() > 0:
                errs["grad " + k] = _rel_max(p.grad, torch.from_numpy(ref))
        for k, e in errs.items():
            assert e < RTOL, "%s %s rel_max %.3e" % (tag, k, e)
            worst = max(worst, e)
    assert seen["leaky_fused"] > 0 and seen["bdd"] > 0, seen
    return worst


def test_rgin_layer_bf16_close_to_fp32_reference(golden_dir):
    """bf16 storage / fp32 accumulate is a build extension (the reference is fp32 only): checked against the
    fp32 golden at bf16 resolution (2^-8 relative per stored tensor).  Outputs: 3e-2 of the range.  Gradients: relative
    L2 error 0.15 -- the fp32 golden and the bf16 run round ~0.2-1 % of the ReLU pre-activations to opposite signs, and each
    such flip switches a whole gradient path (a bias gradient summed over 500 rows then differs by several percent);
    the tight checks of the bf16 kernels are the matched-operand tests (test_relu_mlp_matches_torch_autograd,
    test_fused_row_factorisation_forward_backward, test_rows_*)."""
    from dummynode4graphlearning_amd import BatchedGraph
    z, meta = _cases(golden_dir)
    m = [m for m in meta if m["kind"] == "rgin" and m["hidden_dim"] == 64 and m["regularizer"] == "basis"][0]
    tag = m["tag"]
    layer = _build(m)
    layer.load_state_dict({k[len(tag) + 7:]: torch.from_numpy(z[k]) for k in z.files if k.startswith(tag + "/param/")})
    layer = layer.to(DEV).to(torch.bfloat16)
    u, v, t = (torch.from_numpy(z[tag + "/" + k]).to(DEV) for k in ("u", "v", "t"))
    x = torch.from_numpy(z[tag + "/x"]).to(DEV).to(torch.bfloat16).requires_grad_(True)
    out, _ = layer(BatchedGraph(u, v, m["N"]), x, t)
    (out.float() * torch.from_numpy(z[tag + "/coef"]).to(DEV)).sum().backward()
    assert out.dtype == torch.bfloat16 and x.grad.dtype == torch.bfloat16
    assert _rel_max(out.float(), torch.from_numpy(z[tag + "/out"])) < 3e-2
    errs = {"grad_x": _rel_l2(x.grad.float(), torch.from_numpy(z[tag + "/grad_x"]))}
    for k, p in layer.named_parameters():
        assert p.grad is not None and p.grad.dtype == torch.bfloat16, k
        errs[k] = _rel_l2(p.grad.float(), torch.from_numpy(z[tag + "/grad/" + k]))
    print(errs)
    assert max(errs.values()) < 0.15, errs


def test_rep_nets_match_reference_goldens(golden_dir):
    """a-11: RGINRepNet / RGCNRepNet (get_pattern_rep with the zero mask, get_graph_rep with residual / mask / gate) against
    the reference's own create_rep_net + get_*_rep run (si_rep_nets.npz): outputs and every gradient to 1e-4."""
    from dummynode4graphlearning_amd import BatchedGraph
    from dummynode4graphlearning_amd.subgraph_isomorphism import RGCNRepNet, RGINRepNet
    z = np.load(os.path.join(golden_dir, "si_rep_nets.npz"))
    meta = json.loads(bytes(z["meta"]).decode())
    for m in meta:
        tag = m["tag"]
        if m["kind"] == "rgin":
            net = RGINRepNet(m["H"], m["R"], num_layers=m["num_layers"], rep_residual=m["rep_residual"], act_func=m["act_func"],
                             name=m["name"])
        else:
            net = RGCNRepNet(m["H"], m["R"], num_layers=m["num_layers"], rep_residual=m["rep_residual"], act_func=m["act_func"],
                             edge_norm=m["edge_norm"], name=m["name"])
        net.load_state_dict({k[len(tag) + 7:]: torch.from_numpy(z[k]) for k in z.files if k.startswith(tag + "/param/")}, strict=True)
        net = net.to(DEV).train()
        t = lambda k: torch.from_numpy(z[tag + "/" + k]).to(DEV)  # noqa: E731
        g = BatchedGraph(t("u"), t("v"), m["N"], edata={"label": t("t")})
        x = t("x").requires_grad_(True)
        mode = m["mode"]
        if mode == "pattern_mask":
            out = net.get_pattern_rep(g, x, mask=t("mask"))
        elif mode == "pattern":
            out = net.get_pattern_rep(g, x)
        else:
            out = net.get_graph_rep(g, x, mask=t("mask") if "mask" in mode else None, gate=t("gate") if "gate" in mode else None)
        (out * t("coef")).sum().backward()
        errs = {"out": _rel_max(out, t("out")), "grad_x": _rel_max(x.grad, t("grad_x"))}
        for k, p in net.named_parameters():
            ref = z[tag + "/grad/" + k]
            if ref.size and np.abs(ref).max() > 0:
                errs["grad " + k] = _rel_max(p.grad, torch.from_numpy(ref))
        for k, e in errs.items():
            assert e < RTOL, "%s %s %s %s rel_max %.3e" % (tag, m["kind"], mode, k, e)


def test_rep_net_residual_and_gate(golden_dir):
    from dummynode4graphlearning_amd import BatchedGraph
    from dummynode4graphlearning_amd.subgraph_isomorphism import RGINRepNet
    rng = np.random.default_rng(9)
    N, E, R, H = 120, 500, 4, 32
    torch.manual_seed(1)
    net = RGINRepNet(H, R, num_layers=3, act_func="leaky_relu").to(DEV)
    u, v, t = (torch.from_numpy(rng.integers(0, n, size=E)) for n in (N, N, R))
    g = BatchedGraph(u.to(DEV), v.to(DEV), N, edata={"label": t.to(DEV)})
    x = torch.from_numpy(rng.standard_normal((N, H)).astype(np.float32))
    gate = torch.from_numpy((rng.random((N, 1)) > 0.2).astype(np.float32))
    got = net.get_graph_rep(g, x.to(DEV), gate=gate.to(DEV))
    cur = x * gate
    for layer in net.rgin:
        p = {k: w.detach().cpu() for k, w in layer.named_parameters()}
        o = OL.rgin_layer(cur, u, v, t, p, regularizer="basis", num_rels=R, num_bases=-1, act="leaky_relu") * gate
        cur = cur + o
    assert _rel_max(got, cur) < RTOL


@pytest.mark.parametrize("H", [64, 128])
@pytest.mark.parametrize("slope", [0.0, 1 / 5.5])
def test_two_layer_fp32_mlp_takes_the_chain_launches(H, slope):
    """ops.relu_mlp, two Linears, fp32 on the bf16 split at H = 64 / 128: ONE launch each way for the Linears (dn_rows_chain2_f32) and
    two weight-gradient launches; the same numbers as one launch per Linear (forward: up to the split's rounding of the stored hidden
    rows -- here bit-equal inputs give results within 2e-5; gradients likewise)."""
    from dummynode4graphlearning_amd import ops
    rng = np.random.default_rng(7 + H)
    N = 2500
    x0 = torch.from_numpy(rng.standard_normal((N, H)).astype(np.float32)).to(DEV)
    gout = torch.from_numpy(rng.standard_normal((N, H)).astype(np.float32)).to(DEV)
    lins = [torch.nn.Linear(H, H).to(DEV) for _ in range(2)]

    def run():
        for l in lins:
            l.zero_grad()
        x = x0.clone().requires_grad_(True)
        with ops.KernelTimer() as timer:
            y = ops.relu_mlp(x, lins, slope)
            y.backward(gout)
        return [r[0] for r in timer.records], [y.detach().clone(), x.grad.clone()] + [p.grad.clone() for l in lins for p in l.parameters()]

    tags, got = run()
    assert tags == ["rows_chain2", "rows_wgrad", "rows_chain2", "rows_wgrad"], tags
    old = ops.CHAIN2_F32_ENABLED
    try:
        ops.CHAIN2_F32_ENABLED = False
        tags1, sep = run()
    finally:
        ops.CHAIN2_F32_ENABLED = old
    assert "rows_chain2" not in tags1 and len(tags1) == 6
    for a, b in zip(got, sep):
        assert _rel_l2(a, b) < 2e-5
    with ops.f32_exact(True):                                           # the exact-f32 checker mode keeps one launch per Linear
        tags2, exact = run()
    assert "rows_chain2" not in tags2
    assert _rel_l2(got[0], exact[0]) < 2e-5


@pytest.mark.parametrize("slope", [0.0, 1 / 5.5])
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32])
def test_relu_mlp_matches_torch_autograd(dt, slope):
    """Fused Linear + ReLU / leaky-ReLU chain (forward epilogues, masked input-gradient epilogue, fused bias sums) vs torch in
    fp64 on the same (bf16-rounded) operands; fp32 runs on the exact-f32 MFMA.  slope 1 / 5.5 = the reference's `leaky_relu`
    (utils/act.py:466, constants.py:10)."""
    from dummynode4graphlearning_amd import ops
    rng = np.random.default_rng(4)
    N, H = 3000, 128
    bf = lambda a: torch.from_numpy(a.astype(np.float32)).to(dt)  # noqa: E731
    x = bf(rng.standard_normal((N, H)))
    lins = []
    for _ in range(3):
        lin = torch.nn.Linear(H, H)
        lin.weight.data = bf(rng.standard_normal((H, H)) / np.sqrt(H)).float()
        lin.bias.data = bf(rng.standard_normal(H) * 0.5).float()
        lins.append(lin)
    gout = bf(rng.standard_normal((N, H)))
    dl = [torch.nn.Linear(H, H).to(DEV).to(dt) for _ in lins]
    for d, l in zip(dl, lins):
        d.weight.data.copy_(l.weight.data)
        d.bias.data.copy_(l.bias.data)
    xd = x.to(DEV).requires_grad_(True)
    # fp32: the exact-f32 MFMA for the tight comparison.  (Under the default 3-term bf16 split ONE pre-activation within its 1e-5
    # of 0 decides differently from the fp64 chain -- measured with slope 1/5.5: every quantity behind that element 2.5e-4 off,
    # everything in front of it 7e-6; the exact arithmetic agrees to 4e-7 throughout.  The split is pinned by the goldens.)
    with ops.f32_exact(True):
        y = ops.relu_mlp(xd, dl, slope)
        y.backward(gout.to(DEV))
    # reference: same chain in fp64 with the kernel's storage points (every activation / gradient tensor kept in bf16),
    # so both sides see the same ReLU masks; backward written out by hand (rounding treated as identity)
    rb = lambda t: t.to(dt).double()  # noqa: E731
    acts = [x.double()]
    for l in lins:
        acts.append(rb(torch.nn.functional.leaky_relu(acts[-1] @ l.weight.double().t() + l.bias.double(), slope)))
    dact = lambda a: torch.where(a > 0, torch.ones_like(a), torch.full_like(a, slope))  # noqa: E731
    g = rb(gout.double() * dact(acts[-1]))
    ref_gw, ref_gb = [None] * 3, [None] * 3
    for i in (2, 1, 0):
        ref_gw[i] = g.t() @ acts[i]
        ref_gb[i] = g.sum(0)
        g = g @ lins[i].weight.double()
        if i > 0:
            g = g * dact(acts[i])
        g = rb(g)
    lim = 5e-3 if dt == torch.bfloat16 else 5e-6          # fp32: exact-f32 MFMA (measured 4e-7)
    assert _rel_l2(y, acts[-1]) < lim

    def rows_but_worst(a, b, drop=4):
        """relative L2 over all rows but the `drop` worst: a pre-activation within the arithmetic's 1e-5 of 0 decides differently
        in the two runs (1-2 elements in 1.2 M here) and moves ONE row's gradient by O(1) -- not what this test is about."""
        a, b = a.detach().cpu().double(), b.detach().cpu().double()
        err = (a - b).square().sum(1)
        keep = torch.argsort(err)[: a.shape[0] - drop]
        return float(err[keep].sum().sqrt() / b[keep].norm())

    assert rows_but_worst(xd.grad, g) < lim and _rel_l2(xd.grad, g) < 40 * lim
    for i, d in enumerate(dl):          # (such an element also moves ONE row of that layer's weight gradient and one bias element)
        assert rows_but_worst(d.weight.grad, ref_gw[i], drop=2) < lim and _rel_l2(d.weight.grad, ref_gw[i]) < 40 * lim
        assert rows_but_worst(d.bias.grad.view(-1, 1), ref_gb[i].view(-1, 1), drop=2) < lim


@pytest.mark.parametrize("pre_pad", [False, True])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_split_and_batchify_graph_feats(pre_pad, dtype):
    from dummynode4graphlearning_amd.subgraph_isomorphism.dl import split_and_batchify_graph_feats
    rng = np.random.default_rng(3)
    sizes = torch.tensor([5, 1, 9, 3, 9, 2])
    N, H = int(sizes.sum()), 64
    x = torch.from_numpy(rng.standard_normal((N, H)).astype(np.float32)).to(dtype)
    coef = torch.from_numpy(rng.standard_normal((6, 9, H)).astype(np.float32)).to(dtype)
    xd = x.to(DEV).requires_grad_(True)
    feats, mask = split_and_batchify_graph_feats(xd, sizes.to(DEV), pre_pad=pre_pad)
    (feats.float() * coef.to(DEV).float()).sum().backward()
    xr = x.float().requires_grad_(True)
    rf, rm = OL.split_and_batchify_graph_feats(xr, sizes, pre_pad=pre_pad)
    (rf * coef.float()).sum().backward()
    assert torch.equal(mask.cpu(), rm)
    torch.testing.assert_close(feats.detach().cpu().float(), rf.detach(), rtol=0, atol=0)
    torch.testing.assert_close(xd.grad.cpu().float(), xr.grad, rtol=1e-2 if dtype == torch.bfloat16 else 0, atol=1e-2 if dtype == torch.bfloat16 else 0)
    same = split_and_batchify_graph_feats(torch.ones(8, 4, device=DEV), torch.tensor([4, 4], device=DEV))
    assert same[0].shape == (2, 4, 4) and bool(same[1].all())


@pytest.mark.parametrize("kind,kw", [
    ("rgin", dict(act_func="leaky_relu", num_mlp_layers=2, self_loop=True)),     # fused conv, generic (non-ReLU) MLP path
    ("rgin", dict(act_func="relu", num_mlp_layers=0, self_loop=False)),           # no self loop: bias added outside the kernel
    ("rgin", dict(act_func="relu", num_mlp_layers=2, self_loop=True, regularizer="bdd", num_bases=4)),
    ("rgcn", dict(act_func="relu", edge_norm="in", self_loop=True)),              # per-destination norm around the fused pipeline
    ("rgcn", dict(act_func="relu", edge_norm="both", self_loop=True)),            # separable sqrt(out_norm[src]) sqrt(in_norm[dst])
    ("rgcn", dict(act_func="relu", edge_norm="both", self_loop=False)),           # zero-degree nodes masked to 0
    ("rgcn", dict(act_func="tanh", edge_norm="none", self_loop=False)),
])
def test_bf16_layer_variants_match_fp64_on_same_operands(kind, kw):
    """Every bf16 code path of the SI layers (fused row factorisation with / without self loop, generic MLP, block-diagonal
    weights, RGCN with its separable edge norms around the same pipeline) against the oracle in fp64 on the same bf16-rounded parameters."""
    from dummynode4graphlearning_amd import BatchedGraph, synthetic
    from dummynode4graphlearning_amd.subgraph_isomorphism import RGCNLayer, RGINLayer
    raw = synthetic.config3(seed=21, graphs=16)
    aug = __import__("oracle.transforms", fromlist=["x"]).dummy_augment_si(
        *(raw[k] for k in ("node_ptr", "edge_ptr", "src", "dst", "node_id", "node_label", "edge_id", "edge_label")),
        raw["max_nv"], raw["max_nvl"], raw["max_ne"], raw["max_nel"])
    src, dst, et = (torch.from_numpy(aug[k]) for k in ("src", "dst", "edge_label"))
    N, R, H = len(aug["node_label"]), raw["num_rels"], 64
    torch.manual_seed(7)
    kw = dict(kw)
    cls = RGINLayer if kind == "rgin" else RGCNLayer
    layer = cls(H, H, num_rels=R, **kw).to(torch.bfloat16)
    rng = np.random.default_rng(2)
    x = torch.from_numpy(rng.standard_normal((N, H)).astype(np.float32)).to(torch.bfloat16)
    coef = torch.from_numpy(rng.standard_normal((N, H)).astype(np.float32)).to(torch.bfloat16)
    p64 = {k: v.detach().double().requires_grad_(True) for k, v in layer.named_parameters()}
    dl = layer.to(DEV)
    xd = x.to(DEV).requires_grad_(True)
    out, _ = dl(BatchedGraph(src.to(DEV), dst.to(DEV), N), xd, et.to(DEV))
    out.backward(coef.to(DEV))
    xr = x.double().requires_grad_(True)
    reg, nb = kw.get("regularizer", "basis"), kw.get("num_bases", -1)
    if kind == "rgin":
        ref = OL.rgin_layer(xr, src, dst, et, p64, regularizer=reg, num_rels=R, num_bases=nb,
                            num_mlp_layers=kw["num_mlp_layers"], act=kw["act_func"])
    else:
        ref = OL.rgcn_layer(xr, src, dst, et, p64, regularizer=reg, num_rels=R, num_bases=nb, edge_norm=kw["edge_norm"],
                            act=kw["act_func"])
    ref.backward(coef.double())
    # unmatched storage points (every intermediate of the GPU run is rounded to bf16): 3e-2 relative L2 on the output;
    # gradients 0.1 (a pre-activation rounded across a ReLU / leaky-ReLU kink switches that element's whole gradient path,
    # and a bias gradient sums only 800 such rows here) -- the tight bf16 checks are the matched-storage kernel tests
    assert _rel_l2(out, ref) < 3e-2
    assert _rel_l2(xd.grad, xr.grad) < 0.1
    for k, p in dl.named_parameters():
        if p64[k].grad is not None and p64[k].grad.abs().max() > 0:
            assert _rel_l2(p.grad, p64[k].grad) < 0.1, k


def test_empty_and_degenerate_batches():
    """No edges at all, and a batch whose every graph is a single node: the layers must still run (self loop + bias only)."""
    from dummynode4graphlearning_amd import BatchedGraph
    from dummynode4graphlearning_amd.subgraph_isomorphism import RGINLayer
    z = torch.zeros(0, dtype=torch.long, device=DEV)
    for dtype in (torch.float32, torch.bfloat16):
        torch.manual_seed(0)
        layer = RGINLayer(64, 64, num_rels=3).to(DEV).to(dtype)
        x = torch.randn(7, 64, device=DEV).to(dtype).requires_grad_(True)
        out, _ = layer(BatchedGraph(z, z, 7), x, z)
        out.float().sum().backward()
        p = {k: v.detach().cpu().double() for k, v in layer.named_parameters()}
        ref = OL.rgin_layer(x.detach().cpu().double(), z.cpu(), z.cpu(), z.cpu(), p, num_rels=3, act="relu")
        assert _rel_l2(out, ref) < (5e-5 if dtype == torch.float32 else 2e-2)
        assert x.grad is not None and torch.isfinite(x.grad.float()).all()


def test_dual_layers_match_reference_goldens(golden_dir):
    """f-4: CompGCNLayer / DMPLayer (node AND edge outputs, every gradient) against the reference's own runs, fp32 1e-4."""
    from dummynode4graphlearning_amd import BatchedGraph
    from dummynode4graphlearning_amd.subgraph_isomorphism import CompGCNLayer, DMPLayer
    z = np.load(os.path.join(golden_dir, "si_dual_layers.npz"))
    meta = json.loads(bytes(z["meta"]).decode())
    worst = 0.0
    for m in meta:
        tag, H = m["tag"], m["H"]
        if m["kind"] == "compgcn":
            layer = CompGCNLayer(H, H, self_loop=m["self_loop"], comp_opt=m["comp_opt"], edge_norm=m["edge_norm"],
                                 act_func=m["act_func"])
        else:
            layer = DMPLayer(H, H, num_mlp_layers=m["num_mlp_layers"], batch_norm=False, act_func=m["act_func"])
        sd = {k[len(tag) + 7:]: torch.from_numpy(z[k]) for k in z.files if k.startswith(tag + "/param/")}
        layer.load_state_dict(sd, strict=True)
        layer = layer.to(DEV).train()
        g = BatchedGraph(torch.from_numpy(z[tag + "/u"]).to(DEV), torch.from_numpy(z[tag + "/v"]).to(DEV), m["N"])
        if m["rev"]:
            g.edata["is_reversed"] = torch.from_numpy(z[tag + "/rev"]).to(DEV)
        x = torch.from_numpy(z[tag + "/x"]).to(DEV).requires_grad_(True)
        ef = torch.from_numpy(z[tag + "/ef"]).to(DEV).requires_grad_(True)
        no, eo = layer(g, x, ef)
        ((no * torch.from_numpy(z[tag + "/c1"]).to(DEV)).sum() + (eo * torch.from_numpy(z[tag + "/c2"]).to(DEV)).sum()).backward()
        errs = {"node_out": _rel_max(no, torch.from_numpy(z[tag + "/node_out"])),
                "edge_out": _rel_max(eo, torch.from_numpy(z[tag + "/edge_out"])),
                "grad_x": _rel_max(x.grad, torch.from_numpy(z[tag + "/grad_x"])),
                "grad_ef": _rel_max(ef.grad, torch.from_numpy(z[tag + "/grad_ef"]))}
        for k, p in layer.named_parameters():
            ref = z[tag + "/grad/" + k]
            if ref.size and np.abs(ref).max() > 0:
                errs["grad " + k] = _rel_max(p.grad, torch.from_numpy(ref))
        for k, e in errs.items():
            assert e < RTOL, "%s %s rel_max %.3e" % (tag, k, e)
            worst = max(worst, e)
    print("worst rel_max over %d dual-layer golden cases: %.3e" % (len(meta), worst))


@pytest.mark.parametrize("kind", ["compgcn", "dmp"])
def test_dual_layers_bf16_run_on_the_matrix_cores(kind):
    """bf16 storage (H = 64: the dense products take the MFMA Linear kernels) against the oracle in fp64 on the same
    bf16-rounded parameters and inputs."""
    from dummynode4graphlearning_amd import BatchedGraph
    from dummynode4graphlearning_amd.subgraph_isomorphism import CompGCNLayer, DMPLayer
    rng = np.random.default_rng(3)
    N, E, H = 400, 1600, 64
    u, v = torch.from_numpy(rng.integers(0, N, size=E)), torch.from_numpy(rng.integers(0, N, size=E))
    rev = torch.from_numpy(rng.random(E) < 0.5)
    torch.manual_seed(1)
    layer = (CompGCNLayer(H, H, comp_opt="mult", edge_norm="both", act_func="relu") if kind == "compgcn"
             else DMPLayer(H, H, num_mlp_layers=2, batch_norm=False, act_func="relu")).to(torch.bfloat16)
    x = torch.from_numpy(rng.standard_normal((N, H)).astype(np.float32)).to(torch.bfloat16)
    ef = torch.from_numpy(rng.standard_normal((E, H)).astype(np.float32)).to(torch.bfloat16)
    p64 = {k: t.detach().double() for k, t in layer.named_parameters()}
    dl = layer.to(DEV)
    g = BatchedGraph(u.to(DEV), v.to(DEV), N)
    g.edata["is_reversed"] = rev.to(DEV)
    xd, efd = x.to(DEV).requires_grad_(True), ef.to(DEV).requires_grad_(True)
    no, eo = dl(g, xd, efd)
    (no.float().sum() + eo.float().sum()).backward()
    assert no.dtype == torch.bfloat16 and eo.dtype == torch.bfloat16 and xd.grad is not None and efd.grad is not None
    if kind == "compgcn":
        rn, re = OL.compgcn_layer(x.double(), ef.double(), u, v, rev, p64, comp_opt="mult", edge_norm="both", act="relu")
    else:
        rn, re = OL.dmp_layer(x.double(), ef.double(), u, v, rev, p64, num_mlp_layers=2, act="relu")
    assert _rel_l2(no, rn) < 3e-2 and _rel_l2(eo, re) < 3e-2


def test_predict_nets_match_reference_goldens(golden_dir):
    """f-4: ragged -> padded (HIP gather) -> dummy masking -> Sum/MeanPredictNet against the reference's run: masks exact,
    outputs and every gradient (through the padding op) to 1e-4."""
    from dummynode4graphlearning_amd import subgraph_isomorphism as SI
    z = np.load(os.path.join(golden_dir, "si_pred.npz"))
    meta = json.loads(bytes(z["meta"]).decode())
    for m in meta:
        tag = m["tag"]
        net = getattr(SI, m["cls"])(12, 16, act_func=m["act_func"], return_weights=m["return_weights"])
        net.load_state_dict({k[len(tag) + 7:]: torch.from_numpy(z[k]) for k in z.files if k.startswith(tag + "/param/")}, strict=True)
        net = net.to(DEV)
        t = lambda k: torch.from_numpy(z[tag + "/" + k]).to(DEV)  # noqa: E731
        p_flat, g_flat = t("p_flat").requires_grad_(True), t("g_flat").requires_grad_(True)
        p_rep, p_mask = SI.split_and_batchify_graph_feats(p_flat, t("p_len"), pre_pad=True)
        g_rep, g_mask = SI.split_and_batchify_graph_feats(g_flat, t("g_len"), pre_pad=True)
        g_mask = SI.mask_dummy_nodes(g_mask, t("g_dummy"), t("g_len"))
        assert np.array_equal(g_mask.cpu().numpy(), z[tag + "/g_mask"])
        y, w = net(p_rep, p_mask, g_rep, g_mask)
        B = y.shape[0]
        loss = (y * torch.arange(1, B + 1, device=DEV).view(-1, 1).float()).sum() + (w.sum() if w is not None else 0.0)
        loss.backward()
        assert _rel_max(y, torch.from_numpy(z[tag + "/y"])) < RTOL
        if w is not None:
            assert _rel_max(w, torch.from_numpy(z[tag + "/w"])) < RTOL
        assert _rel_max(p_flat.grad, torch.from_numpy(z[tag + "/grad_p"])) < RTOL
        assert _rel_max(g_flat.grad, torch.from_numpy(z[tag + "/grad_g"])) < RTOL
        for k, p in net.named_parameters():
            assert _rel_max(p.grad, torch.from_numpy(z[tag + "/grad/" + k])) < RTOL, (tag, k)


def test_full_size_config5_layer_through_batch_properties():
    """BASELINE config 5 at FULL size (N = 1,015,808, E = 3,997,696, R = 16, H = 256, bf16) through properties that do not
    need a full-size oracle: (1) a batch is a disjoint union, so the first graphs' rows of the big run must equal a run on
    those graphs alone -- which is itself checked against the fp64 oracle; (2) data-parallel consistency: the parameter
    gradients of the whole batch equal the sum over two half batches (what the RCCL all-reduce relies on); (3) everything
    finite, dummy rows included."""
    from dummynode4graphlearning_amd import BatchedGraph, synthetic, transforms
    from dummynode4graphlearning_amd.subgraph_isomorphism import RGINLayer
    raw = synthetic.config5()
    keys = ("node_ptr", "edge_ptr", "src", "dst", "node_id", "node_label", "edge_id", "edge_label")
    vocab = (raw["max_nv"], raw["max_nvl"], raw["max_ne"], raw["max_nel"])
    H, R, G = 256, raw["num_rels"], len(raw["node_ptr"]) - 1

    def augment(g0, g1):
        n0, n1, e0, e1 = raw["node_ptr"][g0], raw["node_ptr"][g1], raw["edge_ptr"][g0], raw["edge_ptr"][g1]
        sub = dict(node_ptr=raw["node_ptr"][g0:g1 + 1] - n0, edge_ptr=raw["edge_ptr"][g0:g1 + 1] - e0,
                   src=raw["src"][e0:e1] - n0, dst=raw["dst"][e0:e1] - n0, node_id=raw["node_id"][n0:n1],
                   node_label=raw["node_label"][n0:n1], edge_id=raw["edge_id"][e0:e1], edge_label=raw["edge_label"][e0:e1])
        return transforms.dummy_augment_si(*(torch.from_numpy(np.ascontiguousarray(sub[k])).to(DEV) for k in keys), *vocab)

    torch.manual_seed(11)
    layer = RGINLayer(H, H, num_rels=R, regularizer="basis", num_bases=-1, num_mlp_layers=2, act_func="relu").to(DEV).to(torch.bfloat16)
    full = augment(0, G)
    N = int(full["node_label"].numel())
    assert N == 1015808 and int(full["src"].numel()) == 3997696
    gen = torch.Generator(device=DEV).manual_seed(3)
    x = torch.randn(N, H, device=DEV, generator=gen).to(torch.bfloat16)
    coef = torch.randn(N, H, device=DEV, generator=gen).to(torch.bfloat16)

    graphs = {}

    def run(aug, rows, tag=None):
        for p in layer.parameters():
            p.grad = None
        xs = x[rows].clone().requires_grad_(True)
        # the batch WITH its graph boundaries, as bench.py builds it (bench.py:79-80): the graph-local index builder,
        # the absorbed fold and the sweep tile order are what this test must exercise
        bnn = (aug["node_ptr"][1:] - aug["node_ptr"][:-1]).long()
        bne = (aug["edge_ptr"][1:] - aug["edge_ptr"][:-1]).long()
        g = BatchedGraph(aug["src"], aug["dst"], int(aug["node_label"].numel()), bnn, bne, node_ptr=aug["node_ptr"],
                         edge_ptr=aug["edge_ptr"])
        et_ = aug["edge_label"].long()
        out, _ = layer(g, xs, et_)
        out.backward(coef[rows])
        if tag:
            graphs[tag] = (g, et_)
        return out.detach(), xs.grad.detach(), {k: p.grad.detach().float().clone() for k, p in layer.named_parameters()}

    out_f, gx_f, gw_f = run(full, slice(0, N), "full")
    assert bool(torch.isfinite(out_f.float()).all()) and bool(torch.isfinite(gx_f.float()).all())
    # which path ran at full size: graph-local builder, both folds absorbed by the unit stream (AGG units), sweep tile order
    from dummynode4graphlearning_amd import ops
    ix = graphs["full"][0].row_index(graphs["full"][1], R, True).parts[0][2]             # (the cached index the run used)
    assert ix.built_by == "local"
    for d in "fb":
        fold = ops._row_index_fold(ix, d, "units")
        assert fold is not None and fold.graph_tiles is not None and fold.sweep_tiles is not None
        cu = ix.close_units(d)
        assert cu.agg and cu.num_tiles == G
    # (1) first 64 graphs alone (31 nodes each after augmentation)
    g_small = 64
    n_small = g_small * 31
    out_s, gx_s, _ = run(augment(0, g_small), slice(0, n_small))
    assert _rel_l2(out_f[:n_small], out_s) < 2e-3 and _rel_l2(gx_f[:n_small], gx_s) < 2e-3
    #     ... and that small run against the oracle in fp64 on the same bf16 operands
    sm = augment(0, g_small)
    p64 = {k: v.detach().double().cpu() for k, v in layer.named_parameters()}
    ref = OL.rgin_layer(x[:n_small].double().cpu(), sm["src"].long().cpu(), sm["dst"].long().cpu(), sm["edge_label"].long().cpu(),
                        p64, regularizer="basis", num_rels=R, num_bases=-1, num_mlp_layers=2, act="relu")
    assert _rel_l2(out_s, ref) < 3e-2
    # (2) two halves
    half = G // 2
    nh = half * 31
    _, _, gw_a = run(augment(0, half), slice(0, nh))
    _, _, gw_b = run(augment(half, G), slice(nh, N))
    for k in gw_f:
        if float(gw_f[k].abs().max()) > 0:
            assert _rel_l2(gw_a[k] + gw_b[k], gw_f[k]) < 2e-2, k


def test_default_bf16_pipeline_on_2048_config5_graphs_matches_fp64_with_the_same_storage_points():
    """The pipeline bench.py times -- graph-local index builder, folded pre-aggregation, ring transform, fused closing launch,
    two-layer chain with bit masks, LDS-DMA weight gradients -- on 2,048 config-5 graphs (N = 63,488, E = 249,856, R = 16,
    H = 256, bf16) against the reference formulation (rgin.py:102-160: per-edge x[src] W[etype], sum by destination, self loop,
    bias, Linear-ReLU-Linear, ReLU) evaluated in fp64 on the same bf16 parameters and inputs and rounded to bf16 at the points
    where the GPU path stores a bf16 tensor (per-edge product rows, the collapsed relation's per-graph sum, the layer's
    pre-MLP rows, both MLP activations); the rounding is transparent to autograd, so the fp64 gradients are those of the reference
    at the forward values the GPU saw.  The two ReLUs use the GPU run's own sign patterns (its h1 / h2 > 0, recomputed with the
    same deterministic launches): an element whose pre-activation lies within fp32 summation noise of 0 would otherwise switch
    a whole row's gradient path in one of the two runs (measured without this: 0.13 of the maximum on a handful of rows).
    Outputs and EVERY gradient: 2e-2 of the tensor's max, 5e-3 relative L2."""
    from dummynode4graphlearning_amd import BatchedGraph, ops, synthetic, transforms
    from dummynode4graphlearning_amd.subgraph_isomorphism import RGINLayer
    G, H = 2048, 256
    raw = synthetic.config5(seed=5, graphs=G)
    keys = ("node_ptr", "edge_ptr", "src", "dst", "node_id", "node_label", "edge_id", "edge_label")
    aug = transforms.dummy_augment_si(*(torch.from_numpy(raw[k]).to(DEV) for k in keys), raw["max_nv"], raw["max_nvl"],
                                      raw["max_ne"], raw["max_nel"])
    R = raw["num_rels"]
    N, E = int(aug["node_label"].numel()), int(aug["src"].numel())
    assert (N, E) == (G * 31, G * 122)
    bnn = (aug["node_ptr"][1:] - aug["node_ptr"][:-1]).long()
    bne = (aug["edge_ptr"][1:] - aug["edge_ptr"][:-1]).long()
    g = BatchedGraph(aug["src"], aug["dst"], N, bnn, bne, node_ptr=aug["node_ptr"], edge_ptr=aug["edge_ptr"])
    et = aug["edge_label"].long()
    torch.manual_seed(23)
    layer = RGINLayer(H, H, num_rels=R, regularizer="basis", num_bases=-1, num_mlp_layers=2, act_func="relu").to(DEV).to(torch.bfloat16)
    gen = torch.Generator(device=DEV).manual_seed(5)
    x = torch.randn(N, H, device=DEV, generator=gen).to(torch.bfloat16).requires_grad_(True)
    coef = torch.randn(N, H, device=DEV, generator=gen).to(torch.bfloat16)
    out, _ = layer(g, x, et)
    out.backward(coef)
    ix = g.row_index(et, R, True).parts[0][2]
    assert ix.built_by == "local" and ops._row_index_fold(ix, "f") is not None and ops._row_index_fold(ix, "b") is not None
    agg_rel = ops._row_index_fold(ix, "f").rel                     # the collapsed relation of the forward pass (u -> dummy)

    def r(t):                                                       # bf16 storage point, transparent to autograd
        return t + (t.detach().to(torch.bfloat16).double() - t.detach())

    p = {k: v.detach().double().cpu().requires_grad_(True) for k, v in layer.named_parameters()}
    xr = x.detach().double().cpu().requires_grad_(True)
    src, dst, etc = aug["src"].long().cpu(), aug["dst"].long().cpu(), et.cpu()
    acc = xr @ p["loop_weight"] + p["bias"]                         # the unit-stream closing launch keeps the self-loop tile and the
    fold_rows = None                                                # row sums in its fp32 accumulators: one rounding, below
    for rel in range(R):
        e = (etc == rel).nonzero().reshape(-1)
        if e.numel() == 0:
            continue
        if rel == agg_rel:                                          # one row per destination: its input is the SUM of the sources,
            d_u, inv = torch.unique(dst[e], return_inverse=True)    # rounded once; the product joins the output row afterwards
            aux = r(torch.zeros(d_u.numel(), H, dtype=torch.float64).index_add(0, inv, xr[src[e]]))
            fold_rows = (d_u, aux @ p["weight"][rel])
        else:
            acc = acc.index_add(0, dst[e], r(xr[src[e]] @ p["weight"][rel]))
    pre = r(acc)
    pre = pre.index_add(0, fold_rows[0], r(pre[fold_rows[0]] + fold_rows[1]) - pre[fold_rows[0]])
    # the GPU run's pre-MLP rows and activations (bitwise what the layer computed: same launches, no atomics)
    with torch.no_grad():
        W_all = torch.cat([layer.weight, layer.loop_weight.unsqueeze(0)], 0)
        pre_gpu = ops.rel_transform_fused(x.detach(), W_all, layer.bias, g.row_index(et, R, True))
        h1_gpu, h2_gpu = ops.rows_chain2(pre_gpu, layer.mlp[0].weight, layer.mlp[0].bias, True, layer.mlp[2].weight,
                                         layer.mlp[2].bias, True)
        assert torch.equal(h2_gpu, out.detach())
    close_pre = _rel_l2(pre_gpu, pre)
    assert close_pre < 5e-3, close_pre
    m1, m2 = (h1_gpu > 0).double().cpu(), (h2_gpu > 0).double().cpu()
    h1 = r((pre @ p["mlp.0.weight"].t() + p["mlp.0.bias"]) * m1)
    ref = r((h1 @ p["mlp.2.weight"].t() + p["mlp.2.bias"]) * m2)
    ref.backward(coef.double().cpu())

    def close(a, b, what):
        assert _rel_max(a, b) < 2e-2 and _rel_l2(a, b) < 5e-3, (what, _rel_max(a, b), _rel_l2(a, b))

    close(out, ref, "output")
    close(x.grad, xr.grad, "input gradient")
    for k, v in layer.named_parameters():
        close(v.grad, p[k].grad, k)
    # The same reference with its OWN ReLU decisions (no mask taken from the GPU run): the two runs may only disagree where a
    # pre-activation lies within the bf16 storage noise of 0, and on every row where they agree the outputs agree as above.
    with torch.no_grad():
        a1 = pre @ p["mlp.0.weight"].t() + p["mlp.0.bias"]
        own1 = (r(a1) > 0).double()
        a2 = r(a1 * own1) @ p["mlp.2.weight"].t() + p["mlp.2.bias"]
        own2 = (r(a2) > 0).double()
        for name, a, own, gpu_mask in (("hidden", a1, own1, m1), ("output", a2, own2, m2)):
            flip = own != gpu_mask
            frac = float(flip.double().mean())
            rows = float(flip.any(1).double().mean())
            noise = 2.0 ** -7 * float(a.abs().max())                # a bf16 rounding of the largest pre-activation of the tensor
            print("own-mask run, %s ReLU: %.2e of the elements (%.2e of the rows) decide differently" % (name, frac, rows))
            assert frac < 2e-3, (name, frac)
            assert float(a[flip].abs().max()) < noise if bool(flip.any()) else True, (name, float(a[flip].abs().max()), noise)
        ref_own = r(a2 * own2)
        same = ~((own1 != m1).any(1) | (own2 != m2).any(1))
        assert float(same.double().mean()) > 0.5
        assert _rel_l2(out.detach().cpu().double()[same], ref_own[same]) < 5e-3


def test_bf16_step_is_bitwise_reproducible():
    """No atomics anywhere on the path and fixed summation orders: two runs of the same forward + backward (fused closing
    launch, two-layer chains with bit masks, LDS-DMA weight gradients) must agree bit for bit -- which also screens the
    hand-synchronised kernels (counted vmcnt rings, single-barrier pipelines) for races."""
    from dummynode4graphlearning_amd import BatchedGraph, synthetic, transforms
    from dummynode4graphlearning_amd.subgraph_isomorphism import RGINLayer
    raw = synthetic.config5(graphs=4096)
    keys = ("node_ptr", "edge_ptr", "src", "dst", "node_id", "node_label", "edge_id", "edge_label")
    aug = transforms.dummy_augment_si(*(torch.from_numpy(raw[k]).to(DEV) for k in keys), raw["max_nv"], raw["max_nvl"],
                                      raw["max_ne"], raw["max_nel"])
    N, H, R = int(aug["node_label"].numel()), 256, raw["num_rels"]
    torch.manual_seed(5)
    layer = RGINLayer(H, H, num_rels=R, regularizer="basis", num_bases=-1, num_mlp_layers=2, act_func="relu").to(DEV).to(torch.bfloat16)
    gen = torch.Generator(device=DEV).manual_seed(9)
    x0 = torch.randn(N, H, device=DEV, generator=gen).to(torch.bfloat16)
    coef = torch.randn(N, H, device=DEV, generator=gen).to(torch.bfloat16)
    # the batch WITH its graph boundaries, as bench.py builds it: graph-local index, absorbed fold (AGG units), sweep tile order
    bnn = (aug["node_ptr"][1:] - aug["node_ptr"][:-1]).long()
    bne = (aug["edge_ptr"][1:] - aug["edge_ptr"][:-1]).long()
    g = BatchedGraph(aug["src"], aug["dst"], N, bnn, bne, node_ptr=aug["node_ptr"], edge_ptr=aug["edge_ptr"])
    et = aug["edge_label"].long()
    runs = []
    for _ in range(4):
        for p in layer.parameters():
            p.grad = None
        x = x0.clone().requires_grad_(True)
        out, _ = layer(g, x, et)
        out.backward(coef)
        runs.append([out.detach().clone(), x.grad.clone()] + [p.grad.clone() for p in layer.parameters()])
    from dummynode4graphlearning_amd import ops
    ix = g.row_index(et, R, True).parts[0][2]
    assert ix.built_by == "local"
    for d in "fb":
        fold = ops._row_index_fold(ix, d, "units")
        assert fold is not None and fold.graph_tiles is not None and fold.sweep_tiles is not None and ix.close_units(d).agg
    for r in runs[1:]:
        for a, b in zip(runs[0], r):
            assert torch.equal(a, b)


def test_one_row_index_serves_both_closing_kinds():
    """An H = 256 bf16 layer (unit-stream closing launch, fold absorbed into its AGG units) and an H = 128 bf16 layer (slot kernel +
    partial rows + fold tail) on ONE BatchedGraph, i.e. one cached RowIndex: the second kind builds the tables it misses and
    passes the fold verdict on as the slot builder's drop switch -- both layers match the oracle, in either order."""
    from dummynode4graphlearning_amd import BatchedGraph, ops, synthetic, transforms
    from dummynode4graphlearning_amd.subgraph_isomorphism import RGINLayer
    raw = synthetic.config5(seed=21, graphs=300)
    keys = ("node_ptr", "edge_ptr", "src", "dst", "node_id", "node_label", "edge_id", "edge_label")
    aug = transforms.dummy_augment_si(*(torch.from_numpy(raw[k]).to(DEV) for k in keys), raw["max_nv"], raw["max_nvl"], raw["max_ne"],
                                      raw["max_nel"])
    N, R = int(aug["node_label"].numel()), raw["num_rels"]
    et = aug["edge_label"].long()
    bnn = (aug["node_ptr"][1:] - aug["node_ptr"][:-1]).long()
    bne = (aug["edge_ptr"][1:] - aug["edge_ptr"][:-1]).long()
    for order in ((256, 128), (128, 256)):
        g = BatchedGraph(aug["src"], aug["dst"], N, bnn, bne, node_ptr=aug["node_ptr"], edge_ptr=aug["edge_ptr"])
        for H in order:
            torch.manual_seed(H)
            layer = RGINLayer(H, H, num_rels=R, regularizer="basis", num_bases=-1, num_mlp_layers=2, act_func="relu").to(DEV).to(torch.bfloat16)
            gen = torch.Generator(device=DEV).manual_seed(H + 1)
            x = torch.randn(N, H, device=DEV, generator=gen).to(torch.bfloat16).requires_grad_(True)
            out, _ = layer(g, x, et)
            out.backward(torch.ones_like(out))
            p64 = {k: v.detach().double().cpu() for k, v in layer.named_parameters()}
            ref = OL.rgin_layer_rel_grouped(x.detach().double().cpu(), aug["src"].long().cpu(), aug["dst"].long().cpu(), et.cpu(), p64, R,
                                            act="relu", num_mlp_layers=2)
            assert _rel_l2(out, ref) < 3e-2, (order, H, _rel_l2(out, ref))
            assert bool(torch.isfinite(x.grad.float()).all())
        ix = g.row_index(et, R, True).parts[0][2]
        assert ix._units and ix._slots and all(ix._units[d].agg for d in "fb")          # one index, both kinds of tables


def _dummy_layout_batch(rng, G, n, m, R, layout):
    """G graphs of n real nodes + one dummy node, m random real edges (types 0 .. R-3), u -> dummy (R-2), dummy -> u (R-1).
    layout "last": [u_1 .. u_n, d] per graph (train.py:416-426); "first": [d, u_1 .. u_n]; "end": every dummy node behind all
    real nodes of the batch (no contiguous graph ranges)."""
    src, dst, et, node_ptr, edge_ptr = [], [], [], [0], [0]
    for j in range(G):
        if layout == "end":
            base, d = j * n, G * n + j
            real = np.arange(base, base + n)
        else:
            base = j * (n + 1)
            d = base + n if layout == "last" else base
            real = np.arange(base, base + n) + (0 if layout == "last" else 1)
        s, t = rng.integers(0, n, size=m), rng.integers(0, n, size=m)
        src += [real[s], real, np.full(n, d)]
        dst += [real[t], np.full(n, d), real]
        et += [rng.integers(0, R - 2, size=m), np.full(n, R - 2), np.full(n, R - 1)]
        node_ptr.append((j + 1) * (n + 1))
        edge_ptr.append((j + 1) * (m + 2 * n))
    cat = lambda a: torch.from_numpy(np.concatenate(a).astype(np.int64)).to(DEV)  # noqa: E731
    return cat(src), cat(dst), cat(et), G * (n + 1), np.array(node_ptr), np.array(edge_ptr)


@pytest.mark.parametrize("layout,G", [("first", 200), ("end", 2), ("end", 150), ("last", 200)])
def test_absorbed_fold_only_where_the_dummy_row_belongs_to_its_own_tile(layout, G):
    """The AGG units of the unit-stream closing launch add a graph's folded product to the dummy node's row as a plain
    read-modify-write, which is only ordered when the SAME workgroup stored that row (its own tile).  Layouts that put the dummy
    node elsewhere -- in front of its graph (the row then belongs to the previous tile), or all dummy nodes at the end of the
    batch -- must get the verdict "no" from dn_fold_graph_tiles_build_i32 and take partial rows + dn_fold_tail_bf16: results
    bit-identical to a run with the absorbed fold switched off (DN_CLOSE_AGG=0) and close to fp64; the reference's own layout
    (dummy last, train.py:416-426) keeps the absorbed fold."""
    from dummynode4graphlearning_amd import BatchedGraph, ops
    from dummynode4graphlearning_amd.subgraph_isomorphism import RGINLayer
    rng = np.random.default_rng(G)
    H, R, n, m = 256, 8, 20, 44
    src, dst, et, N, node_ptr, edge_ptr = _dummy_layout_batch(rng, G, n, m, R, layout)
    torch.manual_seed(4)
    layer = RGINLayer(H, H, num_rels=R, regularizer="basis", num_bases=-1, num_mlp_layers=2, act_func="relu").to(DEV).to(torch.bfloat16)
    gen = torch.Generator(device=DEV).manual_seed(2)
    x0 = torch.randn(N, H, device=DEV, generator=gen).to(torch.bfloat16)
    coef = torch.randn(N, H, device=DEV, generator=gen).to(torch.bfloat16)

    def run(agg_enabled):
        old = ops.CLOSE_AGG_ENABLED
        ops.CLOSE_AGG_ENABLED = agg_enabled
        try:
            kw = {}
            if layout != "end":
                t = lambda a: torch.from_numpy(a).to(DEV).int()  # noqa: E731
                kw = dict(node_ptr=t(node_ptr), edge_ptr=t(edge_ptr))
                g = BatchedGraph(src, dst, N, torch.full((G,), n + 1), torch.full((G,), m + 2 * n), **kw)
            else:
                g = BatchedGraph(src, dst, N)
            for p in layer.parameters():
                p.grad = None
            x = x0.clone().requires_grad_(True)
            out, _ = layer(g, x, et)
            out.backward(coef)
            ix = g.row_index(et, R, True).parts[0][2]
            absorbed = [ix.close_units(d).agg for d in "fb"]
            return absorbed, [out.detach().clone(), x.grad.clone()] + [p.grad.clone() for p in layer.parameters()]
        finally:
            ops.CLOSE_AGG_ENABLED = old

    absorbed, got = run(True)
    assert absorbed == ([True, True] if layout == "last" else [False, False]), absorbed
    _, want = run(False)
    if layout != "last":
        for a, b in zip(got, want):
            assert torch.equal(a, b)
    else:                                                                # same sums up to the bf16 rounding of the collapsed rows
        for a, b in zip(got, want):
            assert _rel_l2(a, b) < 1e-2
    p64 = {k: v.detach().double().cpu() for k, v in layer.named_parameters()}
    ref = OL.rgin_layer(x0.double().cpu(), src.cpu(), dst.cpu(), et.cpu(), p64, regularizer="basis", num_rels=R, num_bases=-1,
                        num_mlp_layers=2, act="relu")
    assert _rel_l2(got[0], ref) < 3e-2


@pytest.mark.parametrize("seed", [0, 1])
def test_absorbed_fold_on_tu_shaped_batches_with_graphs_of_1_to_700_nodes(seed):
    """north_star quotes the roofline on TU-shaped batches, and TU graphs are not all within 32 nodes (tu_data_processing.py:179-218;
    PROTEINS reaches 620).  RGINLayer H = 256 bf16 on graphs of 1 .. 700 real nodes + the SI dummy node (train.py:404-474): both
    directions take the ABSORBED fold over multi-tile graphs (unit order 2: four conv launches per step, no partial rows, no tail
    launch), the graph-local index builder serves the batch -- its graphs of more than 1024 edges one by one --, and the step equals
    the partial-row path of rounds 4-5 (DN_CLOSE_MULTI=0) up to the bf16 rounding of the collapsed rows, fp64 math within bf16
    noise, and itself bit for bit."""
    from dummynode4graphlearning_amd import BatchedGraph, ops
    from dummynode4graphlearning_amd.subgraph_isomorphism import RGINLayer
    rng = np.random.default_rng(40 + seed)
    H, R = 256, 8
    sizes = [int(np.clip(rng.lognormal(3.4, 0.7), 1, 700)) for _ in range(90)] + [700, 1, 2, 31, 32, 33, 64, 65, 300]
    src, dst, et, node_ptr, edge_ptr = [], [], [], [0], [0]
    for n in sizes:
        base, m = node_ptr[-1], int(1.9 * n)
        s_, t_ = rng.integers(0, n, size=m), rng.integers(0, n, size=m)
        src += [base + s_, base + np.arange(n), np.full(n, base + n)]
        dst += [base + t_, np.full(n, base + n), base + np.arange(n)]
        et += [rng.integers(0, R - 2, size=m), np.full(n, R - 2), np.full(n, R - 1)]
        node_ptr.append(base + n + 1)
        edge_ptr.append(edge_ptr[-1] + m + 2 * n)
    cat = lambda a: torch.from_numpy(np.concatenate(a).astype(np.int64)).to(DEV)  # noqa: E731
    src, dst, et, N, G = cat(src), cat(dst), cat(et), node_ptr[-1], len(sizes)
    assert max(np.diff(edge_ptr)) > 1024
    torch.manual_seed(4)
    layer = RGINLayer(H, H, num_rels=R, regularizer="basis", num_bases=-1, num_mlp_layers=2, act_func="relu").to(DEV).to(torch.bfloat16)
    gen = torch.Generator(device=DEV).manual_seed(2)
    x0 = torch.randn(N, H, device=DEV, generator=gen).to(torch.bfloat16)
    coef = torch.randn(N, H, device=DEV, generator=gen).to(torch.bfloat16)
    t = lambda a: torch.tensor(a, device=DEV, dtype=torch.int32)  # noqa: E731

    def run(multi):
        old = ops.CLOSE_MULTI_ENABLED
        ops.CLOSE_MULTI_ENABLED = multi
        try:
            g = BatchedGraph(src, dst, N, torch.tensor(np.diff(node_ptr)), torch.tensor(np.diff(edge_ptr)), node_ptr=t(node_ptr),
                             edge_ptr=t(edge_ptr))
            for p in layer.parameters():
                p.grad = None
            x = x0.clone().requires_grad_(True)
            with ops.KernelTimer() as timer:
                out, _ = layer(g, x, et)
                out.backward(coef)
            ix = g.row_index(et, R, True).parts[0][2]
            tags = [r[0] for r in timer.records]
            return ix, tags, [out.detach().clone(), x.grad.clone()] + [p.grad.clone() for p in layer.parameters()]
        finally:
            ops.CLOSE_MULTI_ENABLED = old

    ix, tags, got = run(True)
    assert ix.built_by == "local"
    assert [ix.close_units(d).order for d in "fb"] == [3, 3] and all(ix.close_units(d).agg for d in "fb")
    assert tags.count("rows_close") == 2 and "fold_tail" not in tags and tags.count("rows_transform:conv") == 2, tags
    ix0, tags0, want = run(False)
    assert tags0.count("fold_tail") == 2 and not any(ix0.close_units(d).agg for d in "fb")
    for a, b in zip(got, want):
        assert _rel_l2(a, b) < 1e-2
    _, _, again = run(True)
    for a, b in zip(got, again):
        assert torch.equal(a, b)
    p64 = {k: v.detach().double().cpu() for k, v in layer.named_parameters()}
    ref = OL.rgin_layer(x0.double().cpu(), src.cpu(), dst.cpu(), et.cpu(), p64, regularizer="basis", num_rels=R, num_bases=-1,
                        num_mlp_layers=2, act="relu")
    assert _rel_l2(got[0], ref) < 3e-2
