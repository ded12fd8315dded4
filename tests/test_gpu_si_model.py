"""GPU tests of the SI count models RGIN / RGCN (subgraph_isomorphism/graph_adj.py) and their HIP glue (dn_simodel.hip).

* goldens: the reference's own models (tests/golden/si_models.npz), fp32, in both fp32 arithmetic modes: every OutputDict
  tensor and every parameter gradient to RTOL = 1e-4 of the tensor's largest magnitude, masks exact, None pattern identical;
* path tags: the ragged head at the defaults, the padded fallback for pred_return_weights="node";
* exact-integer kernel tests in fp32 and bf16 (small integer operands: every result is exact whatever the summation order);
* a scale case at the SI defaults on config-3 graphs, checked piece by piece against the float64 restatement of
  tests/si_model_ref.py fed the model's own rep outputs, and end to end against a float64 run of the whole model;
* determinism and the errors a bad batch raises."""
import numpy as np
import pytest
import torch

import si_model_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RTOL = 1e-4
CASES = R.load_golden()


def _graph(d, dev=DEV):
    from dummynode4graphlearning_amd import BatchedGraph
    nd = {"id": torch.as_tensor(np.asarray(d["id"])).to(dev), "label": torch.as_tensor(np.asarray(d["label"])).to(dev)}
    if d.get("dummy") is not None:
        nd["is_dummy"] = torch.as_tensor(np.asarray(d["dummy"])).to(dev)
    return BatchedGraph(torch.as_tensor(np.asarray(d["u"])).to(dev), torch.as_tensor(np.asarray(d["v"])).to(dev),
                        int(np.sum(d["sizes"])), batch_num_nodes=torch.as_tensor(np.asarray(d["sizes"])),
                        ndata=nd, edata={"label": torch.as_tensor(np.asarray(d["elabel"])).to(dev)})


def _golden_model(case):
    from dummynode4graphlearning_amd.subgraph_isomorphism import RGCN, RGIN
    cfg = case["cfg"]
    torch.manual_seed(case["seed"])
    model = {"RGIN": RGIN, "RGCN": RGCN}[cfg["rep_net"]](**cfg)
    model.load_state_dict(R.state_dict(case, "param"))
    return model.to(DEV).train()


def _run_golden(case):
    model = _golden_model(case)
    res = model(_graph(R.batch(case, "p")), _graph(R.batch(case, "g")))
    B = case["B"]
    loss = (res["pred_c"] * R.loss_coef(B, torch.float32, DEV)).sum()
    if res["pred_v"] is not None:
        loss = loss + (res["pred_v"] * torch.from_numpy(case["arrays"]["coef_v"]).to(DEV)).sum()
    loss.backward()
    return model, res


@pytest.mark.parametrize("exact", [True, False])
@pytest.mark.parametrize("name", sorted(CASES))
def test_model_matches_the_reference_goldens(name, exact):
    from dummynode4graphlearning_amd import ops
    case = CASES[name]
    a = case["arrays"]
    with ops.f32_exact(exact):
        model, res = _run_golden(case)
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
        print("%s %s out %s rel_max %.3e" % (name, exact, k, e))
        if not e < RTOL:
            bad.append((k, e))
    assert [k for k, p in model.named_parameters() if p.grad is None] == case["none_grad"]
    for k, p in model.named_parameters():
        if p.grad is None:
            continue
        e = R.rel_max(p.grad, a["grad/" + k])
        print("%s %s grad %s rel_max %.3e" % (name, exact, k, e))
        if not e < RTOL:
            bad.append((k, e))
    assert not bad, bad


def _tags(fn):
    from dummynode4graphlearning_amd import ops
    with ops.KernelTimer() as timer:
        fn()
        return set(timer.summary())


def test_path_tags_show_the_ragged_head_and_the_fallback():
    tags = _tags(lambda: _run_golden(CASES["defaults"]))
    for t in ("si_filter", "si_embed", "si_embed_wgrad", "si_pool_sum", "si_pool_sum_bwd", "si_len_mask"):
        assert t in tags, (t, tags)
    assert "si_head_padded" not in tags
    tags = _tags(lambda: _run_golden(CASES["max_head"]))
    assert {"si_pool_max", "si_pool_max_bwd"} <= tags and "si_head_padded" not in tags
    tags = _tags(lambda: _run_golden(CASES["no_filter"]))
    assert "si_meta" in tags and "si_filter" not in tags
    tags = _tags(lambda: _run_golden(CASES["node_weights"]))
    assert "si_head_padded" in tags and "si_pool_sum" not in tags and "si_pool_max" not in tags


def test_two_runs_are_bit_identical():
    outs = []
    for _ in range(2):
        model, res = _run_golden(CASES["defaults"])
        outs.append([res[k].detach().clone() for k in R.OUT_KEYS if res[k] is not None] +
                    [p.grad.clone() for _, p in model.named_parameters() if p.grad is not None])
    assert all(torch.equal(x, y) for x, y in zip(*outs))


def test_bad_batches_raise():
    from dummynode4graphlearning_amd._lib import DnHipError
    case = CASES["defaults"]
    model = _golden_model(case)
    p, g = R.batch(case, "p"), R.batch(case, "g")
    for side, key, value in (("g", "label", case["cfg"]["max_ngvl"]), ("p", "label", -1), ("g", "id", case["cfg"]["max_ngv"])):
        d = dict(g if side == "g" else p)
        d[key] = np.array(d[key], copy=True)
        d[key][3] = value
        pg, gg = (_graph(p), _graph(d)) if side == "g" else (_graph(d), _graph(g))
        with pytest.raises(DnHipError, match="outside"):
            model(pg, gg)
    d = dict(g)
    d["sizes"] = np.array(d["sizes"], copy=True)
    d["sizes"][1] += d["sizes"][2]
    d["sizes"][2] = 0                                          # graph 2 has no nodes
    with pytest.raises(ValueError, match="no nodes"):
        model(_graph(p), _graph(d))


# ------------------------------------------------------------------------------------------------ exact-integer kernel tests
DTYPES = [torch.float32, torch.bfloat16]


def _ragged(rng, sizes, dummy_last=True, nlab=6, nid=16):
    """node_ptr, labels, ids, dummy flags of graphs of the given sizes; a size-1 entry given as -1 is a graph holding only a
    dummy; otherwise the last node of a graph of >= 2 nodes is its dummy (when dummy_last)."""
    ptr, lab, ids, dm = [0], [], [], []
    for s in sizes:
        n = abs(s)
        ptr.append(ptr[-1] + n)
        lab += list(rng.integers(0, nlab, size=n))
        ids += list(rng.integers(0, nid, size=n))
        if s < 0:
            dm += [True] * n
        else:
            dm += [False] * (n - 1) + [dummy_last and n >= 2]
    t = lambda x, dt: torch.tensor(x, dtype=dt, device=DEV)                     # noqa: E731
    return t(ptr, torch.int32), t(lab, torch.int32), t(ids, torch.int32), t(dm, torch.bool)


def _ints(rng, shape, lo, hi, dtype):
    return torch.from_numpy(rng.integers(lo, hi + 1, size=shape).astype(np.float32)).to(DEV).to(dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_exact_filter_gate_and_meta(dtype):
    from dummynode4graphlearning_amd import ops
    rng = np.random.default_rng(11)
    for p_sizes in ([3, 5, 1, 5, 2, 4, 5, 1], [4] * 8):                      # mixed lengths, then all patterns of one length
        g_sizes = [1, -1, 7, 2, 9, 3, 4, 6]                                    # a single-row graph and a dummy-only graph
        pp, pl, pi, _ = _ragged(rng, p_sizes, nlab=5)
        gp, gl, gi, _ = _ragged(rng, g_sizes, nlab=5)
        meta, gate = ops.si_filter_meta(pp, pl, pi, gp, gl, gi, (5, 16), (5, 16), dtype)
        assert meta.tolist()[:3] == [max(p_sizes), max(abs(s) for s in g_sizes), 0]
        want = R.gate({"sizes": [abs(s) for s in p_sizes], "label": pl.cpu().numpy()},
                      {"sizes": [abs(s) for s in g_sizes], "label": gl.cpu().numpy()})
        assert gate.dtype == dtype and torch.equal(gate.double().cpu(), want)
    meta, gate = ops.si_filter_meta(pp, pl, pi, gp, gl, gi, (4, 16), (5, 15), None)
    assert gate is None and meta.tolist()[2] != 0                           # labels / ids beyond the given table sizes


@pytest.mark.parametrize("dtype", DTYPES)
def test_exact_embedding_forward_and_weight_gradient(dtype):
    from dummynode4graphlearning_amd import ops
    rng = np.random.default_rng(12)
    N, H, K1, K2, rows1, rows2 = 300, 16, 6, 8, 7, 20                       # 300 rows: ten 32-row chunks in the gradient
    lab = torch.from_numpy(rng.integers(0, rows1, size=N)).to(DEV).int()
    ids = torch.from_numpy(rng.integers(0, rows2, size=N)).to(DEV).int()
    enc1, enc2 = _ints(rng, (rows1, K1), 0, 1, dtype), _ints(rng, (rows2, K2), -1, 2, dtype)
    W1 = _ints(rng, (K1, H), -2, 2, dtype).requires_grad_(True)
    W2 = _ints(rng, (K2, H), -2, 2, dtype).requires_grad_(True)
    G = _ints(rng, (N, H), -1, 1, dtype)
    G[torch.arange(N, device=DEV) % 3 != 0] = 0                              # <= 100 nonzero rows: |dW| <= 200, exact in bf16
    for two in (False, True):
        out = ops.si_embed(lab, enc1, W1, ids, enc2, W2) if two else ops.si_embed(lab, enc1, W1)
        want = enc1.double()[lab.long()] @ W1.detach().double()
        if two:
            want = want + enc2.double()[ids.long()] @ W2.detach().double()
        assert out.dtype == dtype and torch.equal(out.double(), want)
        W1.grad = W2.grad = None
        out.backward(G)
        assert torch.equal(W1.grad.double(), enc1.double()[lab.long()].t() @ G.double())
        if two:
            assert torch.equal(W2.grad.double(), enc2.double()[ids.long()].t() @ G.double())
        else:
            assert W2.grad is None


@pytest.mark.parametrize("dtype", DTYPES)
def test_exact_sum_pooling_both_ways(dtype):
    from dummynode4graphlearning_amd import ops
    rng = np.random.default_rng(13)
    sizes = [1, -1, 5, 3, 6, 2, 4]
    ptr, lab, ids, dm = _ragged(rng, sizes, nlab=5, nid=9)
    N, H = int(ptr[-1]), 32
    rep = _ints(rng, (N, H), -3, 3, dtype).requires_grad_(True)
    enc_v, enc_vl = _ints(rng, (9, 4), -2, 2, dtype), _ints(rng, (5, 6), -2, 2, dtype)
    E = 20
    src = torch.from_numpy(rng.integers(0, N, size=E)).to(DEV).int()
    dst = torch.from_numpy(rng.integers(0, N, size=E)).to(DEV).int()
    in_deg, out_deg = ops.degrees(src, dst, N)
    for with_enc, with_deg, with_dummy in ((True, True, True), (False, False, True), (True, False, False), (False, True, False)):
        enc = (ids, enc_v, lab, enc_vl) if with_enc else (None,) * 4
        deg = (out_deg, in_deg) if with_deg else (None, None)
        S, cnt = ops.si_pool_sum(rep, ptr, dm if with_dummy else None, *enc, *deg)
        parts = ([enc_v.double()[ids.long()], enc_vl.double()[lab.long()]] if with_enc else []) + \
            ([out_deg.double().view(-1, 1), in_deg.double().view(-1, 1)] if with_deg else [])
        rows = torch.cat(parts + [rep.detach().double()], 1)
        keep = ~dm if with_dummy else torch.ones_like(dm)
        seg = torch.repeat_interleave(torch.arange(len(sizes), device=DEV), (ptr[1:] - ptr[:-1]).long())
        want = torch.zeros(len(sizes), rows.shape[1], dtype=torch.float64, device=DEV).index_add(0, seg[keep], rows[keep])
        assert S.dtype == torch.float32 and torch.equal(S.double(), want)
        assert torch.equal(cnt.long().cpu(), torch.bincount(seg[keep].cpu(), minlength=len(sizes)))
        dS = _ints(rng, tuple(S.shape), -4, 4, torch.float32)
        rep.grad = None
        S.backward(dS)
        want_g = dS.double()[seg][:, rows.shape[1] - H:] * keep.double().view(-1, 1)
        assert rep.grad.dtype == dtype and torch.equal(rep.grad.double(), want_g)


@pytest.mark.parametrize("dtype", DTYPES)
def test_exact_max_pooling_both_ways(dtype):
    from dummynode4graphlearning_amd import ops
    rng = np.random.default_rng(14)
    sizes = [1, -1, 5, 3, 6, 2, 6]
    ptr, _, _, dm = _ragged(rng, sizes)
    N, C, B = int(ptr[-1]), 24, len(sizes)
    L = max(abs(s) for s in sizes)
    # no ties inside a graph: per column a permutation of distinct even integers; the bias is odd
    Y = np.zeros((N, C), np.float32)
    p = ptr.cpu().numpy()
    for b in range(B):
        n = p[b + 1] - p[b]
        for c in range(C):
            Y[p[b]:p[b + 1], c] = 2 * (rng.permutation(40)[:n] - 20)
    Y = torch.from_numpy(Y).to(DEV).to(dtype).requires_grad_(True)
    bias = (2 * _ints(rng, (C,), -10, 10, torch.float32) + 1).to(dtype).requires_grad_(True)
    for with_dummy in (True, False):
        out = ops.si_pool_max(Y, bias, ptr, L, dm if with_dummy else None)
        want, arg = torch.empty(B, C, dtype=torch.float64), torch.empty(B, C, dtype=torch.long)
        Yd, keep = Y.detach().double().cpu(), (~dm if with_dummy else torch.ones_like(dm)).cpu()
        for b in range(B):
            rows = [v for v in range(p[b], p[b + 1]) if keep[v]]
            for c in range(C):
                cand = [(float(Yd[v, c]), v) for v in rows] + ([(float(bias[c].detach()), -1)] if len(rows) < L else [])
                want[b, c], arg[b, c] = max(cand)
        assert out.dtype == dtype and torch.equal(out.double().cpu(), want)
        dout = _ints(rng, (B, C), -3, 3, dtype)
        Y.grad = bias.grad = None
        out.backward(dout)
        wy = torch.zeros(N, C, dtype=torch.float64)
        wb = torch.zeros(C, dtype=torch.float64)
        for b in range(B):
            for c in range(C):
                if arg[b, c] >= 0:
                    wy[arg[b, c], c] = float(dout[b, c])
                else:
                    wb[c] += float(dout[b, c])
        assert torch.equal(Y.grad.double().cpu(), wy) and torch.equal(bias.grad.double().cpu(), wb)


def test_exact_masks():
    from dummynode4graphlearning_amd import ops
    rng = np.random.default_rng(15)
    sizes = [1, -1, 5, 3, 6, 2]
    ptr, _, _, dm = _ragged(rng, sizes)
    L = 7
    for d in (dm, None):
        m = ops.si_len_mask(ptr, L, d)
        want = R.pad_mask([abs(s) for s in sizes] + [L], None if d is None else list(d.cpu().numpy()) + [False] * L)[:-1]
        assert m.dtype == torch.bool and torch.equal(m.cpu(), want)


# ------------------------------------------------------------------------------------------------ the scale case
SI_DEFAULTS = dict(max_ngv=64, max_ngvl=8, max_nge=256, max_ngel=8, max_npv=64, max_npvl=8, max_npe=256, max_npel=8, base=2,
                   enc_net="Multihot", emb_net="Equivariant", filter_net="ScalarFilter", rep_net="RGIN", rep_num_graph_layers=3,
                   rep_num_pattern_layers=3, rep_rgin_regularizer="bdd", rep_rgin_num_bases=4, rep_act_func="leaky_relu",
                   rep_residual=True, share_enc_net=True, share_emb_net=True, share_rep_net=True, pred_net="SumPredictNet",
                   pred_with_enc=True, pred_with_deg=True, hid_dim=64, pred_hid_dim=64, pred_dropout=0.0, rep_dropout=0.0,
                   pred_return_weights="none", init_neigenv=0.0, init_eeigenv=0.0)


def scale_batches(seed=0):
    """config-3 graphs (512 x 49 real nodes + dummy) and 512 seeded patterns of 3-9 real nodes (+ dummy), both through
    transforms.dummy_augment_si.  Returns (pattern dict, graph dict) of device tensors + the numpy view si_model_ref reads."""
    from dummynode4graphlearning_amd import synthetic, transforms
    raw = synthetic.config3()
    vocab = (raw["max_nv"], raw["max_nvl"], raw["max_ne"], raw["max_nel"])
    rng = np.random.default_rng(seed)
    G = 512
    n = rng.integers(3, 10, size=G)
    m = np.array([int(rng.integers(k, 2 * k + 1)) for k in n])
    node_ptr, edge_ptr = np.concatenate([[0], np.cumsum(n)]), np.concatenate([[0], np.cumsum(m)])
    src = np.concatenate([rng.integers(0, k, size=e) + o for k, e, o in zip(n, m, node_ptr[:-1])])
    dst = np.concatenate([rng.integers(0, k, size=e) + o for k, e, o in zip(n, m, node_ptr[:-1])])
    pat = dict(node_ptr=node_ptr, edge_ptr=edge_ptr, src=src, dst=dst, node_id=np.concatenate([np.arange(k) for k in n]),
               node_label=rng.integers(0, raw["max_nvl"], size=int(n.sum())), edge_id=np.concatenate([np.arange(e) for e in m]),
               edge_label=rng.integers(0, raw["max_nel"], size=int(m.sum())))
    keys = ("node_ptr", "edge_ptr", "src", "dst", "node_id", "node_label", "edge_id", "edge_label")
    out = []
    for b in (pat, raw):
        aug = transforms.dummy_augment_si(*(torch.from_numpy(np.asarray(b[k], np.int64)).to(DEV) for k in keys), *vocab)
        np_view = {"sizes": (aug["node_ptr"][1:] - aug["node_ptr"][:-1]).cpu().numpy(), "u": aug["src"].cpu().numpy(),
                   "v": aug["dst"].cpu().numpy(), "id": aug["node_id"].cpu().numpy(), "label": aug["node_label"].cpu().numpy(),
                   "elabel": aug["edge_label"].cpu().numpy(), "dummy": aug["is_dummy_node"].bool().cpu().numpy()}
        out.append((aug, np_view))
    return out


def _scale_graph(aug):
    from dummynode4graphlearning_amd import BatchedGraph
    N = int(aug["node_label"].numel())
    return BatchedGraph(aug["src"], aug["dst"], N, batch_num_nodes=(aug["node_ptr"][1:] - aug["node_ptr"][:-1]).long(),
                        ndata={"id": aug["node_id"], "label": aug["node_label"], "is_dummy": aug["is_dummy_node"].bool()},
                        edata={"label": aug["edge_label"]}, node_ptr=aug["node_ptr"], edge_ptr=aug["edge_ptr"])


def _scale_model(cfg, dtype=torch.float32, seed=21):
    from dummynode4graphlearning_amd.subgraph_isomorphism import RGIN
    torch.manual_seed(seed)
    model = RGIN(**cfg)
    with torch.no_grad():                                      # pred_fc2 starts at zero: perturb so every gradient flows
        for p in model.parameters():
            if p.requires_grad:
                p.add_(0.05 * torch.randn_like(p))
    return model.to(DEV).to(dtype).train()


def _scale_step(model, pg, gg):
    """Forward + backward under the goldens' loss sum(pred_c * (1..B) / B), the loss si_model_ref restates."""
    res = model(pg, gg)
    for k in ("p_v_emb", "g_v_emb", "p_v_rep", "g_v_rep"):
        res[k].retain_grad()
    B = res["pred_c"].shape[0]
    (res["pred_c"].float() * R.loss_coef(B, torch.float32, DEV)).sum().backward()
    return res


def _cpu_sd(model):
    return {k: v.detach().cpu() for k, v in model.state_dict().items()}


def test_scale_fp32_pieces_match_the_restatement():
    from dummynode4graphlearning_amd import ops
    (pa, p), (ga, g) = scale_batches()
    assert int(ga["node_label"].numel()) == 25600 and len(p["sizes"]) == 512
    model = _scale_model(SI_DEFAULTS)
    res = _scale_step(model, _scale_graph(pa), _scale_graph(ga))
    sd = _cpu_sd(model)
    # the gate the graph rep net received (same launch as inside forward)
    _, gate = ops.si_filter_meta(pa["node_ptr"], pa["node_label"], pa["node_id"], ga["node_ptr"], ga["node_label"], ga["node_id"],
                                 (8, 64), (8, 64), torch.float32)
    assert torch.equal(gate.double().cpu(), R.gate(p, g))
    ref = R.forward_outside_reps(sd, SI_DEFAULTS, p, g, res["p_v_rep"].detach().cpu(), res["g_v_rep"].detach().cpu())
    checks = [("p_v_emb", res["p_v_emb"], ref["p_v_emb"]), ("g_v_emb", res["g_v_emb"], ref["g_v_emb"]),
              ("pred_c", res["pred_c"], ref["pred_c"])]
    for k in ("p_v_mask", "g_v_mask"):
        assert torch.equal(res[k].cpu(), ref[k]), k
    checks += [("grad p_v_rep", res["p_v_rep"].grad, ref["grad_p_rep"]), ("grad g_v_rep", res["g_v_rep"].grad, ref["grad_g_rep"])]
    for k, want in ref["pred_grads"].items():
        checks.append(("grad " + k, dict(model.named_parameters())[k].grad, want))
    for side, d in (("g", g), ("p", p)):
        e = res[side + "_v_emb"].grad.double().cpu()
        lab = torch.from_numpy(np.asarray(d["label"], np.int64))
        want = sd["%s_enc_net.vl.weight" % side].double()[lab].t() @ e
        checks.append(("grad %s_emb_net.vl.weight" % side, dict(model.named_parameters())["%s_emb_net.vl.weight" % side].grad, want))
    bad = []
    for k, got, want in checks:
        err = R.rel_max(got, want)
        print("scale fp32 %s rel_max %.3e" % (k, err))
        if not err < RTOL:
            bad.append((k, err))
    assert not bad, bad
    assert dict(model.named_parameters())["g_emb_net.v.weight"].grad is None              # add_node_id off
    assert dict(model.named_parameters())["g_emb_net.vl.row_vec"].grad is None            # (sic) never used by the forward


def test_scale_bf16_kernels_match_the_restatement_on_the_same_values():
    """bf16: the new kernels' own outputs, each rounded once when stored (at most 2^-8 relative: bf16 keeps 8 significant
    bits), to 2^-8 of the largest magnitude:
    the embeddings, the pooled fp32 sums, the gradient into the rep rows and the embedding weight gradient, all on the bf16
    model's own values (its tables, weights and rep outputs)."""
    from dummynode4graphlearning_amd import ops
    (pa, p), (ga, g) = scale_batches()
    model = _scale_model(SI_DEFAULTS, torch.bfloat16)
    res = _scale_step(model, _scale_graph(pa), _scale_graph(ga))
    assert torch.isfinite(res["pred_c"].float()).all()
    sd = _cpu_sd(model)
    bound = 2.0 ** -8
    errs = {"p_v_emb": R.rel_max(res["p_v_emb"], R.embed(sd, "p", p, False)),
            "g_v_emb": R.rel_max(res["g_v_emb"], R.embed(sd, "g", g, False))}
    rng = np.random.default_rng(3)
    for side, aug, d in (("p", pa, p), ("g", ga, g)):
        rep = res[side + "_v_rep"].detach().clone().requires_grad_(True)
        in_deg, out_deg = ops.degrees(aug["src"], aug["dst"], rep.shape[0])
        enc_v, enc_vl = model.g_enc_net["v"].weight, model.g_enc_net["vl"].weight
        S, _ = ops.si_pool_sum(rep, aug["node_ptr"], aug["is_dummy_node"], aug["node_id"], enc_v, aug["node_label"], enc_vl,
                               out_deg, in_deg)
        rows = R.node_rows(sd, SI_DEFAULTS, side, d, rep.detach().double().cpu())
        keep = torch.from_numpy(~d["dummy"])
        seg = torch.repeat_interleave(torch.arange(len(d["sizes"])), torch.from_numpy(d["sizes"]).long())
        want = torch.zeros(S.shape, dtype=torch.float64).index_add(0, seg[keep], rows[keep])
        errs[side + " pooled"] = R.rel_max(S, want)
        dS = torch.from_numpy(rng.standard_normal(tuple(S.shape)).astype(np.float32)).to(DEV)
        S.backward(dS)
        want_g = dS.double().cpu()[seg][:, -rep.shape[1]:] * keep.double().view(-1, 1)
        errs[side + " grad rep"] = R.rel_max(rep.grad, want_g)
        W = model.g_emb_net["vl"].weight.detach().clone().requires_grad_(True)
        emb = ops.si_embed(aug["node_label"], enc_vl, W)
        G = torch.from_numpy(rng.standard_normal(tuple(emb.shape)).astype(np.float32)).to(DEV).bfloat16()
        emb.backward(G)
        lab = torch.from_numpy(np.asarray(d["label"], np.int64))
        errs[side + " grad emb W"] = R.rel_max(W.grad, enc_vl.detach().double().cpu()[lab].t() @ G.double().cpu())
    for k, e in errs.items():
        print("scale bf16 %s rel_max %.3e" % (k, e))
    assert all(e <= bound for e in errs.values()), errs


def test_scale_end_to_end_matches_a_float64_run_in_exact_mode():
    """f32_exact, rep_rgin_regularizer="basis" (config 3's own setting): pred_c against a float64 run of the whole forward,
    the rep nets restated through oracle.layers.rgin_layer_rel_grouped (as test_gpu_train_loop.py does), to 1e-4."""
    from dummynode4graphlearning_amd import ops
    from oracle import layers as OL
    cfg = dict(SI_DEFAULTS, rep_rgin_regularizer="basis", rep_rgin_num_bases=-1)
    (pa, p), (ga, g) = scale_batches()
    with ops.f32_exact(True):
        model = _scale_model(cfg)
        res = model(_scale_graph(pa), _scale_graph(ga))
    sd = _cpu_sd(model)

    def reps(d, x, gate):
        src, dst, et = (torch.from_numpy(np.asarray(d[k], np.int64)) for k in ("u", "v", "elabel"))
        x = x * gate if gate is not None else x
        for layer in model.g_rep_net.rgin:
            prm = {k: v.detach().double().cpu() for k, v in layer.named_parameters()}
            o = OL.rgin_layer_rel_grouped(x, src, dst, et, prm, 8, act="leaky_relu", num_mlp_layers=2)
            x = x + (o * gate if gate is not None else o)
        return x

    p_rep = reps(p, R.embed(sd, "p", p, False), None)
    g_rep = reps(g, R.embed(sd, "g", g, False), R.gate(p, g))
    ref = R.forward_outside_reps(sd, cfg, p, g, p_rep, g_rep)
    e = R.rel_max(res["pred_c"], ref["pred_c"])
    print("scale end to end pred_c rel_max %.3e" % e)
    assert e < 1e-4


def test_scale_two_runs_are_bit_identical():
    (pa, _), (ga, _) = scale_batches()
    outs = []
    for _ in range(2):
        model = _scale_model(SI_DEFAULTS)
        res = _scale_step(model, _scale_graph(pa), _scale_graph(ga))
        outs.append([res["pred_c"].detach().clone(), res["p_v_rep"].grad.clone(), res["g_v_rep"].grad.clone()] +
                    [q.grad.clone() for _, q in model.named_parameters() if q.grad is not None])
    assert all(torch.equal(x, y) for x, y in zip(*outs))
