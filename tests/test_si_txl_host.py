"""The TransformerXL count model on edge sequences, on the CPU (no GPU, no kernels), against the reference's goldens
(tests/golden/si_txl*.npz: make_golden_si_txl.py):

* construction: state_dict keys and shapes (the _module_dict / _param_dict prefixes, pos_emb last), shared modules, the initial values
  under the golden's seed (hashes; values for one case);
* the WHOLE model and every TXLLayer case on the composed path: every OutputDict tensor (masks exact), every parameter gradient and
  the gradients of p_e_rep / g_e_rep, of w, r_w_bias and r_r_bias; the multi-segment cases pin k_net.weight.grad, which carries the
  gradient that comes through the detached memory;
* ops.txl_attention on CPU tensors takes the composed op and agrees with the float64 restatement of txl_ref.py;
* the whole-sequence restatement (TransformerXL._rep_fused, on the composed op and on txl_ref.attention) equals the segment loop in
  float64, values and every gradient, within 1e-12 of the largest magnitude;
* the seg_len quirk, the ignored rep_txl_* keys, expand(**kw), the refusals inherited from EdgeSeqModel.

Bound: 1e-4 of a tensor's largest magnitude (the project's bound for fp32 against fp32 goldens), masks and integers exact."""
import hashlib
import os

import numpy as np
import pytest
import torch

import eseq_ref as R
import txl_ref as T
from test_si_cnn_host import build_seq

CASES = T.load_cases()
MODELS = [(m, a) for m, a in CASES if m["kind"] == "model"]
LAYERS = [(m, a) for m, a in CASES if m["kind"] == "layer"]


def _sha(t):
    return hashlib.sha256(t.detach().contiguous().numpy().tobytes()).hexdigest()[:24]


def build_model(m, arrs, device="cpu"):
    from dummynode4graphlearning_amd.subgraph_isomorphism import TransformerXL
    torch.manual_seed(m["seed"])
    model = TransformerXL(**m["cfg"])
    init = {k: t.clone() for k, t in model.state_dict().items()}
    sd = model.state_dict()
    with torch.no_grad():
        for k in sd:
            src = m["alias"].get(k, k)
            sd[k].copy_(torch.from_numpy(arrs["param/%s" % src]))
    return model.to(device), init


def run_model(m, arrs, device="cpu"):
    model, _ = build_model(m, arrs, device)
    model.train(m["mode"] == "train")
    res = model(build_seq(arrs, "p", device), build_seq(arrs, "g", device))
    res["p_e_rep"].retain_grad()
    res["g_e_rep"].retain_grad()
    B = m["B"]
    c = torch.arange(1, B + 1, dtype=torch.float32, device=device).view(-1, 1) / B
    loss = (res["pred_c"] * c).sum()
    if res["pred_e"] is not None:
        loss = loss + (res["pred_e"] * torch.from_numpy(arrs["coef_e"]).to(device)).sum()
    loss.backward()
    return model, res


def check_model(m, arrs, model, res):
    for k in res.keys():
        if k in m["none_out"]:
            assert res[k] is None, k
        else:
            R.close(res[k].detach().cpu().numpy(), arrs["out/%s" % k], "%s out/%s" % (m["name"], k))
    R.close(res["p_e_rep"].grad.cpu().numpy(), arrs["grad_rep/p"], "%s grad p_e_rep" % m["name"])
    R.close(res["g_e_rep"].grad.cpu().numpy(), arrs["grad_rep/g"], "%s grad g_e_rep" % m["name"])
    for k, p in model.named_parameters():
        if k in m["none_grad"]:
            assert p.grad is None, k
        else:
            R.close(p.grad.cpu().numpy(), arrs["grad/%s" % k], "%s grad/%s" % (m["name"], k))


def run_layer(m, arrs, device="cpu", fused=None):
    """The golden layer case through TXLLayer.forward (fused is None: one segment with its memory, composed) or through
    TXLLayer.forward_sequence over [pad | memory | segment] (the segment's window is then the last seg + mem rows; fused picks the
    path of ops.txl_attention): (layer, init hashes, y, {w, r_w_bias, r_r_bias: gradient})."""
    from dummynode4graphlearning_amd import ops
    from dummynode4graphlearning_amd.subgraph_isomorphism import TXLLayer
    torch.manual_seed(m["seed"])
    H, mem = m["H"], m["mem"]
    layer = TXLLayer(H, H, num_heads=m["heads"], pre_lnorm=m["pre_lnorm"])
    init = {k: _sha(t) for k, t in layer.state_dict().items()}
    with torch.no_grad():
        for k, t in layer.state_dict().items():
            t.copy_(torch.from_numpy(arrs["param/%s" % k]))
    layer = layer.to(device).train()
    w = torch.from_numpy(arrs["in/w"]).to(device).requires_grad_(True)
    rwb = torch.from_numpy(arrs["in/r_w_bias"]).to(device).requires_grad_(True)
    rrb = torch.from_numpy(arrs["in/r_r_bias"]).to(device).requires_grad_(True)
    mems = torch.from_numpy(arrs["in/mems"]).to(device)
    r = torch.from_numpy(arrs["in/r"]).to(device)
    Q = w.shape[1]
    if fused is None:
        mask = torch.ones((1, Q, Q + mem), dtype=torch.bool, device=device)
        y = layer(w, r, rwb, rrb, attn_mask=mask, mems=mems if mem > 0 else None)
    else:
        x = w if mem == 0 else torch.cat([w.new_zeros((w.shape[0], Q - mem, H)), mems, w], 1)
        with ops.eseq_fused(fused):
            y = layer.forward_sequence(x, r[0].flip(0), rwb, rrb, Q, mem)[:, -Q:]
    (y * torch.from_numpy(arrs["in/coef"]).to(device)).sum().backward()
    return layer, init, y, {"w": w.grad, "r_w_bias": rwb.grad, "r_r_bias": rrb.grad}


def check_layer(m, arrs, layer, y, grads):
    R.close(y.detach().cpu().numpy(), arrs["out/y"], m["name"] + " y")
    for k, g in grads.items():
        R.close(g.cpu().numpy(), arrs["grad_in/%s" % k], "%s d%s" % (m["name"], k))
    for k, p in layer.named_parameters():
        R.close(p.grad.cpu().numpy(), arrs["grad/%s" % k], "%s grad/%s" % (m["name"], k))


def test_the_golden_files_hold_every_case_the_issue_lists():
    by_name = {m["name"]: (m, a) for m, a in MODELS}
    assert {"defaults", "heads4", "pre_lnorm", "mem32", "seg16", "clamp20", "layers1", "layers3", "no_share", "position", "mean_head",
            "edge_weights", "equal_lengths", "all_filtered", "revflag", "dropout_eval"} <= set(by_name)
    lens = by_name["defaults"][1]["g/seq/lens"]
    L = by_name["defaults"][1]["g/seq/u"].shape[1]
    assert lens.min() >= 70 and L <= 150 and L % 64 != 0 and 2 <= -(-L // 64) <= 3
    for k in ("seg_len", "mem_len", "clamp_len", "num_heads", "pre_lnorm"):
        assert k not in by_name["defaults"][0]["cfg"]
    assert by_name["heads4"][0]["cfg"]["num_heads"] == 4 and by_name["pre_lnorm"][0]["cfg"]["pre_lnorm"]
    assert by_name["mem32"][0]["cfg"]["mem_len"] == 32 and by_name["seg16"][0]["cfg"]["seg_len"] == 16
    assert by_name["clamp20"][0]["cfg"]["clamp_len"] == 20
    assert by_name["layers1"][0]["cfg"]["rep_num_graph_layers"] == 1 and by_name["layers3"][0]["cfg"]["rep_num_graph_layers"] == 3
    assert by_name["dropout_eval"][0]["cfg"]["rep_dropout"] > 0 and by_name["dropout_eval"][0]["mode"] == "eval"
    assert not by_name["no_share"][0]["cfg"]["share_rep_net"] and not by_name["no_share"][0]["alias"]
    a = by_name["all_filtered"][1]
    assert not a["out/g_e_rep"][0].any() and a["out/g_e_rep"][1].any()              # every tuple of graph 0 is filtered out
    a = by_name["equal_lengths"][1]
    assert len(set(a["g/seq/lens"].tolist())) == 1 and len(set(a["p/seq/lens"].tolist())) == 1
    assert {(m["mem"], m["pre_lnorm"], m["heads"]) for m, _ in LAYERS} == {(a, b, c) for a in (0, 64, 32) for b in (False, True)
                                                                          for c in (1, 4)}
    for m, a in MODELS:                                                              # biases and LayerNorm weights are non-trivial
        for k in [k for k in m["keys"] if k.endswith(("o_net.bias", "layer_norm.weight", "layer_norm.bias")) and k not in m["alias"]]:
            v = a["param/%s" % k]
            assert np.unique(v).size == v.size, k
    for f in os.listdir(T.GOLDEN):
        if f.startswith("si_txl"):
            assert os.path.getsize(os.path.join(T.GOLDEN, f)) < 1 << 20, f


@pytest.mark.parametrize("case", MODELS, ids=[m["name"] for m, _ in MODELS])
def test_construction_matches_the_reference(case):
    m, arrs = case
    model, init = build_model(m, arrs)
    assert list(init.keys()) == m["keys"]
    assert {k: list(t.shape) for k, t in init.items()} == m["shapes"]
    assert {k: _sha(t) for k, t in init.items()} == m["init_sha"]
    sd = model.state_dict(keep_vars=True)
    for k, src in m["alias"].items():
        assert sd[k] is sd[src], (k, src)
    for k, t in init.items():
        if "init/%s" % k in arrs:
            assert np.array_equal(t.numpy(), arrs["init/%s" % k]), k
    assert [k for k, _ in model.named_parameters()] == m["params"]
    cfg = m["cfg"]
    n, H = cfg.get("num_heads", 1), cfg["hid_dim"]
    assert list(init.keys())[-1] == "pos_emb.weight" and not sd["pos_emb.weight"].requires_grad
    seg = cfg.get("seg_len", 64)
    assert init["pos_emb.weight"].shape[0] == max(cfg.get("clamp_len", -1), seg + cfg.get("seg_len", 0) + cfg.get("mem_len", 64))
    for side, key in (("g", "graph"), ("p", "pattern")):
        assert tuple(sd["%s_rep_net._param_dict.r_w_bias" % side].shape) == (n, H // n)
        assert tuple(sd["%s_rep_net._param_dict.r_r_bias" % side].shape) == (n, H // n)
        for i in range(cfg["rep_num_%s_layers" % key]):
            pre = "%s_rep_net._module_dict.txl.%s_txl_(%d)." % (side, "graph" if cfg["share_rep_net"] else key, i)
            for name in ("q", "k", "v", "r"):
                assert tuple(sd[pre + "attn.%s_net.weight" % name].shape) == (H, H) and pre + "attn.%s_net.bias" % name not in sd
            for name in ("attn.o_net.weight", "attn.o_net.bias", "attn.layer_norm.weight", "ff.layer1.weight", "ff.layer2.bias",
                         "ff.layer_norm.bias"):
                assert pre + name in sd
    assert (model.p_rep_net is model.g_rep_net) == cfg["share_rep_net"]


@pytest.mark.parametrize("case", MODELS, ids=[m["name"] for m, _ in MODELS])
def test_model_composed_on_the_cpu_matches_the_reference(case):
    from dummynode4graphlearning_amd import ops
    m, arrs = case
    with ops.eseq_fused(False):
        model, res = run_model(m, arrs)
    check_model(m, arrs, model, res)
    assert res["p_e_emb"].shape[:2] == arrs["p/seq/u"].shape            # rows layout [B, L, C] throughout, lengths kept
    assert res["g_e_rep"].shape[:2] == arrs["g/seq/u"].shape


@pytest.mark.parametrize("case", [c for c in MODELS if c[0]["name"] in ("defaults", "heads4", "pre_lnorm", "mem32", "seg16")],
                         ids=lambda c: c[0]["name"])
def test_model_whole_sequence_path_on_cpu_tensors_matches_the_reference(case):
    """`with ops.eseq_fused(True)` on CPU tensors: the layers refuse the kernels (fused_ok), the model stays on the segment loop."""
    from dummynode4graphlearning_amd import ops
    m, arrs = case
    with ops.eseq_fused(True):
        model, res = run_model(m, arrs)
    check_model(m, arrs, model, res)


@pytest.mark.parametrize("case", LAYERS, ids=[m["name"] for m, _ in LAYERS])
def test_layer_composed_on_the_cpu_matches_the_reference(case):
    m, arrs = case
    layer, init, y, grads = run_layer(m, arrs)
    assert init == m["init_sha"] and list(init.keys()) == m["keys"]
    check_layer(m, arrs, layer, y, grads)
    assert layer.get_output_dim() == m["H"]


@pytest.mark.parametrize("case", LAYERS, ids=[m["name"] for m, _ in LAYERS])
def test_layer_over_the_whole_sequence_on_cpu_tensors_takes_the_composed_op_and_matches(case):
    from dummynode4graphlearning_amd import ops
    m, arrs = case
    class Tags(ops.KernelTimer):                                          # the tags alone: no GPU events without a GPU
        def launch(self, tag, fn):
            self.records.append((tag, None, None))
            return fn()

    with Tags() as t:
        layer, _, y, grads = run_layer(m, arrs, fused=True)
    check_layer(m, arrs, layer, y, grads)
    tags = {r[0] for r in t.records}
    assert "txl_composed" in tags and "txl_attn_fwd" not in tags, tags


def _op_inputs(seed, B, Lp, n, d, seg, mem, dtype=torch.float64):
    g = torch.Generator().manual_seed(seed)
    mk = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64).to(dtype).requires_grad_(True)  # noqa: E731
    return dict(q=mk(B, Lp, n, d), k=mk(B, Lp, n, d), v=mk(B, Lp, n, d), k_mem=mk(B, Lp, n, d), v_mem=mk(B, Lp, n, d),
                rk=mk(seg + mem, n, d), r_w_bias=mk(n, d), r_r_bias=mk(n, d)), torch.randn(B, Lp, n * d, generator=g, dtype=torch.float64)


@pytest.mark.parametrize("geo", [(2, 192, 2, 8, 64, 64), (2, 128, 1, 16, 64, 32), (3, 48, 4, 4, 16, 0), (1, 144, 1, 8, 48, 64),
                                 (2, 72, 2, 4, 24, 24)], ids=str)
def test_op_on_cpu_tensors_takes_the_composed_op_and_agrees_with_the_restatement(geo):
    from dummynode4graphlearning_amd import ops
    B, Lp, n, d, seg, mem = geo
    scale = 1 / d ** 0.5
    ins, coef = _op_inputs(11 + Lp, *geo)
    assert not ops.txl_attention_supported(*ins.values(), seg, mem)
    got = ops.txl_attention(*ins.values(), seg, mem, scale)
    assert torch.equal(got, ops.txl_attention_composed(*ins.values(), seg, mem, scale))
    (got * coef).sum().backward()
    ref_ins = {k: t.detach().clone().requires_grad_(True) for k, t in ins.items()}
    want = T.attention(*ref_ins.values(), seg, mem, scale)
    (want * coef).sum().backward()
    R.close(got.detach().numpy(), want.detach().numpy(), "out", rel=1e-12)
    for k in ins:
        if mem == 0 and k in ("k_mem", "v_mem"):
            assert ins[k].grad is None and ref_ins[k].grad is None
            continue
        R.close(ins[k].grad.numpy(), ref_ins[k].grad.numpy(), "d" + k, rel=1e-12)
    if mem > 0:                                                          # the memory rows' gradient is a gradient of its own
        assert ins["k_mem"].grad[:, -seg:].abs().max() == 0 and ins["k_mem"].grad[:, :seg].abs().max() > 0
        assert ins["k"].grad.abs().min() > 0


def test_rel_shift_is_the_flat_reindexing_and_its_wrapped_entries_are_live():
    from dummynode4graphlearning_amd import ops
    for qlen, klen in ((4, 4), (4, 7), (16, 48), (64, 128)):
        x = torch.arange(1, 2 * qlen * klen * 3 + 1, dtype=torch.float64).view(2, qlen, klen, 3)
        got = ops.txl_rel_shift(x)
        row, col = T.shift_index(qlen, klen)
        want = x[:, row, (col - 1).clamp(min=0)] * (col > 0).double().view(1, qlen, klen, 1)
        assert torch.equal(got, want)
        assert int((col == 0).sum()) == qlen - 1 and set(torch.unique(row - torch.arange(qlen).view(-1, 1)).tolist()) <= {0, 1}
        hit = torch.zeros(qlen, klen)
        hit[row[col > 0], col[col > 0] - 1] += 1                          # a bijection onto every entry but BD[0, 0 .. qlen - 2]
        assert hit[0, :qlen - 1].sum() == 0 and hit.sum() == qlen * klen - (qlen - 1) and hit.max() == 1


WHOLE = [("defaults_L192", {}, 192), ("defaults_L150", {}, 150), ("mem32_heads4_L200", {"mem_len": 32, "num_heads": 4}, 200),
         ("seg16_pre_lnorm", {"seg_len": 16, "pre_lnorm": True}, 70), ("pre_lnorm_L130", {"pre_lnorm": True}, 130),
         ("L65", {}, 65)]


@pytest.mark.parametrize("name,over,L", WHOLE, ids=[w[0] for w in WHOLE])
def test_the_whole_sequence_restatement_equals_the_segment_loop_in_float64(name, over, L, monkeypatch):
    from dummynode4graphlearning_amd import ops
    from dummynode4graphlearning_amd.subgraph_isomorphism import TransformerXL
    m, _ = MODELS[0]
    torch.manual_seed(7)
    model = TransformerXL(**dict(m["cfg"], rep_num_graph_layers=2, **over)).double()
    with torch.no_grad():
        for p in model.g_rep_net.parameters():
            p.add_(0.2 * torch.randn_like(p))
    B, H = 3, m["cfg"]["hid_dim"]
    lens = torch.tensor([L, L // 2, 3])
    mask = (torch.arange(L).view(1, L) >= (L - lens).view(-1, 1)).view(B, L, 1)
    emb0 = torch.randn(B, L, H, dtype=torch.float64)
    coef = torch.randn(B, L, H, dtype=torch.float64)
    net = model.g_rep_net

    def run(fn):
        model.zero_grad()
        emb = emb0.clone().requires_grad_(True)
        out = fn(net, emb.masked_fill(~mask, 0.0), mask)
        (out * coef).sum().backward()
        return [out.detach(), emb.grad] + [p.grad.clone() for p in net.parameters()]

    want = run(model._rep_composed)
    got = run(model._rep_fused)                                           # (CPU tensors: ops.txl_attention's composed op)
    monkeypatch.setattr(ops, "txl_attention", T.attention)
    got_ref = run(model._rep_fused)
    for a, b, c in zip(want, got, got_ref):
        R.close(b.numpy(), a.numpy(), name, rel=1e-12)
        R.close(c.numpy(), a.numpy(), name + " (txl_ref)", rel=1e-12)
    k_grad = dict(net.named_parameters())["_module_dict.txl.graph_txl_(0).attn.k_net.weight"].grad
    assert k_grad.abs().max() > 0
    if name == "L65":
        # data padded right, mask padded left: the live outputs of a sequence shorter than 64 lie in the second segment, whose only
        # data row is row 64 (the first segment reaches it as detached memory); the full-length sequence keeps output row 63 too
        assert (want[1].abs().sum(-1) > 0).sum(1).tolist() == [65, 1, 1]


def test_the_memory_sends_gradient_into_the_weights_but_not_into_the_input():
    from dummynode4graphlearning_amd.subgraph_isomorphism import TransformerXL
    m, _ = MODELS[0]
    torch.manual_seed(3)
    model = TransformerXL(**dict(m["cfg"], rep_num_graph_layers=1)).double()
    B, L, H = 2, 128, m["cfg"]["hid_dim"]
    mask = torch.ones(B, L, 1, dtype=torch.bool)
    emb = torch.randn(B, L, H, dtype=torch.float64, requires_grad=True)
    k_net = next(iter(model.g_rep_net["txl"])).attn.k_net
    coef = torch.randn(B, 64, H, dtype=torch.float64)
    for fn in (model._rep_composed, model._rep_fused):
        model.zero_grad()
        emb.grad = None
        out = fn(model.g_rep_net, emb, mask)
        (out[:, 64:] * coef).sum().backward()                                      # the second segment only: it sees the first as memory
        assert emb.grad[:, :64].abs().max() == 0 and emb.grad[:, 64:].abs().max() > 0
        g_all = k_net.weight.grad.clone()
        model.zero_grad()
        model.mem_len = 0                                                 # the same segment without its memory
        out = fn(model.g_rep_net, emb, mask)
        (out[:, 64:] * coef).sum().backward()
        model.mem_len = 64
        assert (g_all - k_net.weight.grad).abs().max() > 1e-6


def test_the_seg_len_quirk_and_the_ignored_keys():
    from dummynode4graphlearning_amd.subgraph_isomorphism import TransformerXL
    m, arrs = MODELS[0]
    dflt = TransformerXL(**m["cfg"])
    assert (dflt.seg_len, dflt.ext_len, dflt.mem_len, dflt.clamp_len, dflt.num_heads) == (64, 0, 64, -1, 1)
    assert dflt.effective_mem_len() == 64 and dflt.pos_emb.weight.shape[0] == 128
    quirk = TransformerXL(**dict(m["cfg"], seg_len=64))                   # the same segment length, passed: the memory never fills
    assert quirk.ext_len == 64 and quirk.effective_mem_len() == 0 and quirk.pos_emb.weight.shape[0] == 192
    assert TransformerXL(**dict(m["cfg"], mem_len=0)).effective_mem_len() == 0
    assert TransformerXL(**dict(m["cfg"], clamp_len=300)).pos_emb.weight.shape[0] == 300
    x = torch.randn(2, 100, m["cfg"]["hid_dim"])
    mask = torch.ones(2, 100, 1, dtype=torch.bool)
    quirk.load_state_dict({k: v for k, v in dflt.state_dict().items() if k != "pos_emb.weight"}, strict=False)
    with torch.no_grad():
        a, b = quirk._rep_composed(quirk.g_rep_net, x, mask), dflt._rep_composed(dflt.g_rep_net, x, mask)
        assert torch.allclose(quirk._rep_composed(quirk.g_rep_net, x[:, :64], mask[:, :64]),      # one segment: no memory either way
                              dflt._rep_composed(dflt.g_rep_net, x[:, :64], mask[:, :64]))
        assert not torch.allclose(a, b)                                   # later segments differ: one has a memory, one has not
    torch.manual_seed(m["seed"])
    plain = TransformerXL(**m["cfg"])
    torch.manual_seed(m["seed"])
    keyed = TransformerXL(**dict(m["cfg"], rep_txl_seg_len=16, rep_txl_mem_len=8, rep_txl_num_heads=4, rep_txl_pre_lnorm=True))
    assert keyed.seg_len == 64 and keyed.num_heads == 1
    assert all(torch.equal(a, b) for a, b in zip(plain.state_dict().values(), keyed.state_dict().values()))
    assert not hasattr(TransformerXL, "decoder_forward")
    deep = TransformerXL(**dict(m["cfg"], rep_num_graph_layers=6))        # more layers than the reference's torch could run
    with torch.no_grad():
        assert deep._rep_composed(deep.g_rep_net, x, mask).shape == x.shape


def test_expand_keeps_the_old_weights_and_the_outputs():
    from dummynode4graphlearning_amd import ops
    m, arrs = next(c for c in MODELS if c[0]["name"] == "no_share")
    model, _ = build_model(m, arrs)
    model.eval()
    p, g = build_seq(arrs, "p"), build_seq(arrs, "g")
    with ops.eseq_fused(False), torch.no_grad():
        before = model(p, g)
        old = {k: t.clone() for k, t in model.state_dict().items()}
        model.expand(**dict(m["cfg"], max_ngv=100, max_ngvl=20, max_npv=100, max_npvl=20))
        after = model(p, g)
    assert model.max_ngv == 100 and model.max_npv == 100 and model.max_ngvl == 20
    sd = model.state_dict()
    for k in ("g_emb_net.u.weight", "g_emb_net.vl.weight", "p_emb_net.ul.weight", "pred_net.g_fc.weight"):
        o, n = old[k], sd[k]
        assert n.shape[0] >= o.shape[0] and n.shape[1] >= o.shape[1] and n.numel() > o.numel(), k
        assert torch.equal(n[n.shape[0] - o.shape[0]:, n.shape[1] - o.shape[1]:], o), k
    for k in ("g_rep_net._module_dict.txl.graph_txl_(0).attn.k_net.weight", "p_rep_net._param_dict.r_r_bias", "pos_emb.weight"):
        assert torch.equal(sd[k], old[k]), k
    assert torch.equal(before["p_e_mask"], after["p_e_mask"]) and after["pred_c"].shape == before["pred_c"].shape
    with pytest.raises(ValueError):
        model.expand(base=3)


def test_the_refusals_inherited_from_edge_seq_model():
    from dummynode4graphlearning_amd import ops
    from dummynode4graphlearning_amd.subgraph_isomorphism import TransformerXL
    m, arrs = MODELS[0]
    p, g = build_seq(arrs, "p"), build_seq(arrs, "g")
    model = TransformerXL(**dict(m["cfg"], filter_net="None"))            # constructs, as in the reference
    assert model.filter_net is None
    with ops.eseq_fused(False), pytest.raises(ValueError, match="ScalarFilter"):
        model(p, g)
    model, _ = build_model(m, arrs)
    g.tdata["is_dummy"] = torch.zeros_like(g.u, dtype=torch.bool)
    with ops.eseq_fused(False), pytest.raises(NotImplementedError, match="basemodel.py:534"):
        model(p, g)
