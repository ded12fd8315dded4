"""GPU tests of the SI training objective (dn_objective.hip through ops.si_objective, SIObjective and the epoch meters).

* the exact goldens (every value a multiple of 1/8) bitwise, on the kernels and on the composed path;
* the general goldens in fp32 on both paths, and with bf16-rounded operands on the kernels against the float64 restatement of
  tests/objective_ref.py evaluated on those operands;
* shapes the goldens do not have: one pair with one position, a [1, 3], a [100001, 3] (many workgroups, a tail that is no multiple
  of the vector width) and a [4099, 64] representation, sliced (not 16-byte aligned) and strided inputs against their contiguous copies;
* (3 * loss).backward(), zero weights, two runs bit for bit, nothing read back under torch's sync debug mode;
* one whole RGIN through model + SIObjective against the reference's train_epoch.

Bounds (u = 2^-24; tests/objective_ref.py): a term, a sum of n non-negative addends, |x - golden| <= (n + 8) u golden; an elementwise
gradient relative 16 u and exact zero where the golden is zero; d pred_c (n + 8) u sum|addends|; bf16 gradients 2^-8 more."""
import numpy as np
import pytest
import torch

import objective_ref as R
import si_model_ref as MR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
META, A, CASES = R.golden()
EXACT = sorted(t for t, c in CASES.items() if c["kind"] == "exact")
GENERAL = sorted(t for t, c in CASES.items() if c["kind"] == "general")
PATHS = ("fused", "composed")


def _ops():
    from dummynode4graphlearning_amd import ops
    return ops


def _tags(fn):
    with _ops().KernelTimer() as timer:
        out = fn()
        return out, set(timer.summary())


def _run(tag, path, dtype=torch.float32):
    with _ops().objective_fused(path == "fused"):
        (out, loss, terms), tags = _tags(lambda: R.run_case(tag, DEV, dtype))
    want = {"si_objective_fwd", "si_objective_bwd"} if path == "fused" else {"si_objective_composed"}
    assert tags & {"si_objective_fwd", "si_objective_bwd", "si_objective_composed"} == want, tags
    return out, loss, terms


def _grads(out):
    return {k: (None if t.grad is None else t.grad.float().cpu().numpy()) for k, t in out.items() if t is not None and t.dtype != torch.bool}


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("tag", EXACT)
def test_exact_goldens_bitwise(tag, path):
    out, loss, terms = _run(tag, path)
    assert terms.dtype == torch.float64 and terms.shape == (7,) and not terms.requires_grad and loss.dim() == 0
    assert np.array_equal(terms.cpu().numpy(), A[tag + "/terms"]), (terms.tolist(), A[tag + "/terms"].tolist())
    assert float(loss.detach()) == A[tag + "/terms"][1]
    for k, g in R.grads_of(tag).items():
        assert np.array_equal(out[k].grad.double().cpu().numpy(), g), k


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("tag", GENERAL)
def test_general_goldens_fp32(tag, path):
    out, loss, terms = _run(tag, path)
    R.check_against_golden(tag, terms.cpu().numpy(), _grads(out), path)
    assert abs(float(loss.detach()) - float(terms[1])) <= R.U * abs(float(terms[1]))


def _restated(out, counts, nw, ew, cfg, is_graph=True):
    """The restatement on the operands as the tensors hold them (bf16-rounded ones included)."""
    inp = {k: t.detach().float().cpu().numpy() if t.dtype != torch.bool else t.cpu().numpy() for k, t in out.items() if t is not None}
    inp["counts"] = counts.cpu().numpy()
    if nw is not None:
        inp["node_weights"] = nw.float().cpu().numpy()
    if ew is not None:
        inp["edge_weights"] = ew.float().cpu().numpy()
    return R.objective(**R.kwargs_of(inp, cfg, is_graph))


def _check_restated(want, terms, out, what, extra=0.0):
    R.check_terms(terms.cpu().numpy(), want["terms"], want["terms_n"], what)
    g = want["grads"]
    reps = [k for k in R.REP_KEYS if out[k] is not None]
    R.check_pred_c_grad(out["pred_c"].grad.float().cpu().numpy(), g["pred_c"], want["pred_c_n"], want["pred_c_abs"], what, extra)
    for k in ("pred_v", "pred_e"):
        if g[k] is None:
            assert out[k] is None or out[k].grad is None, k
        else:
            R.check_elementwise(out[k].grad.float().cpu().numpy(), g[k], "%s %s" % (what, k), extra)
    for i, k in enumerate(reps):
        R.check_elementwise(out[k].grad.float().cpu().numpy(), g["reps"][i], "%s %s" % (what, k), extra)


@pytest.mark.parametrize("tag", GENERAL)
def test_general_cases_with_bf16_operands(tag):
    case, inp = CASES[tag], R.inputs(A, tag)
    out = R.output_of(inp, DEV, torch.bfloat16)
    nw, ew = (None if w is None else w.to(torch.bfloat16) for w in R.weights_of(inp, DEV))
    counts = torch.from_numpy(inp["counts"]).to(DEV)
    with _ops().objective_fused(True):
        (loss, terms), tags = _tags(lambda: R.objective_of(case["cfg"])(out, counts, nw, ew, is_graph=case["is_graph"]))
        loss.backward()
    assert "si_objective_fwd" in tags and loss.dtype == torch.float32
    assert all(t.grad is None or t.grad.dtype == torch.bfloat16 for t in out.values() if t is not None and t.dtype != torch.bool)
    cfg = dict(case["cfg"], neg_pred_slp=float(np.float32(case["cfg"]["neg_pred_slp"])))
    _check_restated(_restated(out, counts, nw, ew, cfg, case["is_graph"]), terms, out, "bf16 " + tag, extra=2.0 ** -8)


CFG = dict(bp_loss="MSE", eval_metric="MAE", neg_pred_slp=0.125, match_loss_w=0.75, match_reg_w=0.5, rep_reg_w=0.25)


def _shape_case(B, Lv, Le, rep_shapes, seed, bp_loss="MSE"):
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    out = {k: None for k in R.OUT_KEYS}
    out.update(pred_c=rn(B, 1), pred_v=rn(B, Lv), pred_e=rn(B, Le), g_v_mask=torch.rand(B, Lv, generator=g) < 0.7,
               g_e_mask=torch.rand(B, Le, generator=g) < 0.7)
    for k, s in zip(("p_v_rep", "g_v_rep", "p_e_rep", "g_e_rep"), rep_shapes):
        out[k] = rn(*s)
    counts = torch.randint(0, 4, (B,), generator=g)
    return out, counts, rn(B, Lv).abs(), rn(B, Le).abs(), dict(CFG, bp_loss=bp_loss)


def _on_device(out, dtype=torch.float32):
    return {k: (None if t is None else (t.to(DEV) if t.dtype == torch.bool else t.to(DEV).to(dtype).requires_grad_(True))) for k, t in out.items()}


@pytest.mark.parametrize("name,B,Lv,Le,reps,bp", [
    ("one_pair_one_position", 1, 1, 1, [(1, 3)], "MSE"),
    ("many_workgroups_odd_tail", 5, 7, 13, [(100001, 3), (4099, 64)], "SMSE"),
    ("four_reps_two_ranks", 3, 70, 130, [(4099, 64), (1, 3), (3, 9, 5), (3, 1, 64)], "MAE"),
])
def test_shapes_beyond_the_goldens(name, B, Lv, Le, reps, bp):
    host, counts, nw, ew, cfg = _shape_case(B, Lv, Le, reps, seed=len(name), bp_loss=bp)
    results = {}
    for path in PATHS:
        out = _on_device(host)
        with _ops().objective_fused(path == "fused"):
            loss, terms = R.objective_of(cfg)(out, counts.to(DEV), nw.to(DEV), ew.to(DEV))
            loss.backward()
        results[path] = (out, terms)
    out, terms = results["fused"]
    want = _restated(out, counts, nw, ew, cfg)
    R.check_terms(terms.cpu().numpy(), want["terms"], want["terms_n"], name)
    R.check_terms(results["composed"][1].cpu().numpy(), want["terms"], want["terms_n"], name + " composed")
    for k, t in out.items():                                                   # the same fp32 operations in the same order on both paths
        if t is not None and t.dtype != torch.bool and k != "pred_c":
            R.check_elementwise(t.grad.cpu().numpy(), results["composed"][0][k].grad.cpu().numpy(), "%s %s" % (name, k))
    R.check_pred_c_grad(out["pred_c"].grad.cpu().numpy(), want["grads"]["pred_c"], want["pred_c_n"], want["pred_c_abs"], name)
    for i, k in enumerate(k for k in R.REP_KEYS if out[k] is not None):
        R.check_elementwise(out[k].grad.cpu().numpy(), want["grads"]["reps"][i], "%s %s restated" % (name, k))


def test_sliced_and_strided_inputs_equal_their_contiguous_copies():
    host, counts, nw, ew, cfg = _shape_case(5, 7, 13, [(4099, 3), (33, 64)], seed=77)
    ops, got = _ops(), {}
    for layout in ("contiguous", "views"):
        leaves = {}
        if layout == "views":                                                  # rows behind an odd element offset; every other column; a transposed target
            flat = {k: torch.cat([torch.zeros(1), host[k].reshape(-1)]).to(DEV).requires_grad_(True) for k in ("p_v_rep", "g_v_rep")}
            wide = {k: torch.stack([host[k], host[k] + 1], dim=2).reshape(host[k].shape[0], -1).to(DEV).requires_grad_(True)
                    for k in ("pred_c", "pred_v", "pred_e")}
            leaves.update(flat)
            leaves.update(wide)
            out = {k: None for k in R.OUT_KEYS}
            out.update({k: flat[k][1:].view(host[k].shape) for k in flat})
            out.update({k: wide[k][:, ::2] for k in wide})
            out.update(g_v_mask=host["g_v_mask"].t().contiguous().to(DEV).t(), g_e_mask=host["g_e_mask"].to(DEV))
            assert out["p_v_rep"].data_ptr() % 16 != 0 and not out["pred_v"].is_contiguous() and not out["g_v_mask"].is_contiguous()
            nwd, ewd = nw.t().contiguous().to(DEV).t(), ew.to(DEV)
        else:
            out = _on_device(host)
            nwd, ewd = nw.to(DEV), ew.to(DEV)
        with ops.objective_fused(True):
            loss, terms = R.objective_of(cfg)(out, counts.to(DEV), nwd, ewd)
            loss.backward()
        if layout == "views":
            grads = {k: leaves[k].grad[1:].view(host[k].shape) for k in ("p_v_rep", "g_v_rep")}
            grads.update({k: leaves[k].grad[:, ::2] for k in ("pred_c", "pred_v", "pred_e")})
            assert all(bool((leaves[k].grad[:, 1::2] == 0).all()) for k in ("pred_c", "pred_v", "pred_e"))
        else:
            grads = {k: out[k].grad for k in ("p_v_rep", "g_v_rep", "pred_c", "pred_v", "pred_e")}
        got[layout] = (loss.detach(), terms, grads)
    a, b = got["contiguous"], got["views"]
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert all(torch.equal(a[2][k], b[2][k]) for k in a[2])


def test_scaled_loss_backward_and_zero_weights():
    host, counts, nw, ew, cfg = _shape_case(5, 7, 13, [(40, 6), (5, 13, 6)], seed=5)
    ops, results = _ops(), {}
    for path in PATHS:
        out = _on_device(host)
        with ops.objective_fused(path == "fused"):
            loss, _ = R.objective_of(cfg)(out, counts.to(DEV), nw.to(DEV), ew.to(DEV))
            (3 * loss).backward()
        results[path] = out
    for k, t in results["fused"].items():
        if t is not None and t.dtype != torch.bool:
            other = results["composed"][k].grad.cpu().numpy()
            if k == "pred_c":                                                  # a row sum: within its magnitude sum's bound of the composed one
                want = _restated(results["fused"], counts, nw, ew, cfg)
                R.check_pred_c_grad(t.grad.cpu().numpy(), 3 * want["grads"]["pred_c"], want["pred_c_n"], 3 * want["pred_c_abs"], "3 x loss")
            else:
                R.check_elementwise(t.grad.cpu().numpy(), other, "3 x loss " + k)
    out = _on_device(host)
    with ops.objective_fused(True):
        loss, terms = R.objective_of(dict(cfg, match_loss_w=0, match_reg_w=0, rep_reg_w=0))(out, counts.to(DEV), nw.to(DEV), ew.to(DEV))
        loss.backward()
    for k, t in out.items():
        if t is not None and t.dtype != torch.bool:
            assert t.grad is not None, k
            assert k == "pred_c" or bool((t.grad == 0).all()), k
    assert bool((out["pred_c"].grad != 0).any()) and float(terms[2]) != 0 and float(terms[6]) != 0


def test_two_runs_are_bit_identical():
    host, counts, nw, ew, cfg = _shape_case(37, 50, 90, [(100001, 3), (4099, 64)], seed=9)
    runs = []
    for _ in range(2):
        out = _on_device(host)
        with _ops().objective_fused(True):
            loss, terms = R.objective_of(cfg)(out, counts.to(DEV), nw.to(DEV), ew.to(DEV))
            loss.backward()
        runs.append([loss.detach(), terms] + [t.grad for t in out.values() if t is not None and t.dtype != torch.bool])
    assert all(torch.equal(x, y) for x, y in zip(*runs))


def test_nothing_is_read_back():
    """Forward + backward, SITrainMeter.update and SIEvalMeter.update under torch's sync debug mode "error", after checking that this
    build honours the mode at all."""
    from dummynode4graphlearning_amd.subgraph_isomorphism import SIEvalMeter, SITrainMeter
    host, counts, nw, ew, cfg = _shape_case(5, 7, 13, [(4099, 64), (5, 13, 6)], seed=3)
    counts, nw, ew = counts.to(DEV), nw.to(DEV), ew.to(DEV)
    obj, ops = R.objective_of(cfg), _ops()

    def step(out, train, ev):
        loss, terms = obj(out, counts, nw, ew)
        loss.backward()
        train.update(terms, 5)
        ev.update(out, counts, nw, ew)
        return loss.detach(), terms

    with ops.objective_fused(True):
        warm = step(_on_device(host), SITrainMeter(), SIEvalMeter(8))         # (the library is loaded and probed outside the mode)
        out, train, ev = _on_device(host), SITrainMeter(), SIEvalMeter(8)
        probe = torch.ones(1, device=DEV)
        torch.cuda.synchronize()
        prev = torch.cuda.get_sync_debug_mode()
        torch.cuda.set_sync_debug_mode("error")
        try:
            with pytest.raises(RuntimeError):
                probe.item()                                                   # the mode is honoured: a plain read-back raises
            got = step(out, train, ev)
        finally:
            torch.cuda.set_sync_debug_mode(prev)
    assert torch.equal(got[0], warm[0]) and torch.equal(got[1], warm[1])
    assert abs(train.result()["bp_loss"] - float(got[1][1])) <= 1e-6 * abs(float(got[1][1]))
    ae, se, ned, eed, cls = R.eval_errors(out["pred_c"].detach().cpu().numpy(), counts.cpu().numpy(), out["pred_v"].detach().cpu().numpy(),
                                          nw.cpu().numpy(), out["pred_e"].detach().cpu().numpy(), ew.cpu().numpy())
    res = ev.result()
    assert np.array_equal(res["AE"].numpy(), ae.astype(np.float32)) and np.array_equal(res["SE"].numpy(), (ae.astype(np.float32)) ** 2)
    R.check_terms(res["NED"].numpy(), ned, 7, "NED")
    R.check_terms(res["EED"].numpy(), eed, 13, "EED")
    assert abs(res["AUC"] - R.auc(cls)) <= 1e-12


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("rid", range(len(META["eval"])))
def test_eval_meter_reproduces_the_recorded_epoch(rid, path):
    with _ops().objective_fused(path == "fused"):
        meter, tags = _tags(lambda: R.eval_meter(META["eval"][rid], DEV))
    assert ("si_objective_eval" in tags) == (path == "fused") and ("si_eval_composed" in tags) == (path != "fused")
    R.check_eval_result(META["eval"][rid], meter.result())


def _model_case():
    from dummynode4graphlearning_amd import BatchedGraph
    from dummynode4graphlearning_amd.subgraph_isomorphism import RGIN
    m = META["model"]
    torch.manual_seed(m["seed"])
    model = RGIN(**m["cfg"])
    model.load_state_dict({k: torch.from_numpy(np.array(A["model/param/" + m["alias"].get(k, k)])) for k in m["keys"]})

    def graph(side):
        d = {k: A["model/%s/%s" % (side, k)] for k in ("sizes", "u", "v", "id", "label", "elabel", "dummy")}
        to = lambda a: torch.as_tensor(np.asarray(a)).to(DEV)  # noqa: E731
        return BatchedGraph(to(d["u"]), to(d["v"]), int(np.sum(d["sizes"])), batch_num_nodes=torch.as_tensor(np.asarray(d["sizes"])),
                            ndata={"id": to(d["id"]), "label": to(d["label"]), "is_dummy": to(d["dummy"].astype(bool))},
                            edata={"label": to(d["elabel"])})

    return m, model.to(DEV).train(), graph("p"), graph("g")


@pytest.mark.parametrize("path", PATHS)
def test_whole_model_against_the_references_train_epoch(path):
    """RGIN with pred_return_weights="node" + SIObjective against train_epoch's terms and parameter gradients (exact-f32 products, as
    the existing whole-model test checks; gradients to its RTOL = 1e-4 of the tensor's largest magnitude)."""
    ops = _ops()
    m, model, pg, gg = _model_case()
    t = m["train_cfg"]
    counts, nw = torch.from_numpy(A["model/counts"]).to(DEV), torch.from_numpy(A["model/node_weights"]).to(DEV)
    with ops.f32_exact(True), ops.objective_fused(path == "fused"):
        out = model(pg, gg)
        assert out["pred_v"] is not None and tuple(out["pred_v"].shape) == tuple(nw.shape)
        loss, terms = R.objective_of(t)(out, counts, nw, None, model=model)
        loss.backward()
    assert [k for k, p in model.named_parameters() if p.grad is None] == m["none_grad"]
    bad = []
    for k, p in model.named_parameters():
        if p.grad is not None:
            e = MR.rel_max(p.grad, A["model/grad/" + k])
            print("%s grad %s rel_max %.3e" % (path, k, e))
            if not e < 1e-4:
                bad.append((k, e))
    assert not bad, bad
    inp = {k: v.detach().cpu().numpy() for k, v in out.items() if v is not None}
    inp.update(counts=A["model/counts"], node_weights=A["model/node_weights"])
    R.check_terms(terms.cpu().numpy(), A["model/terms"], R.objective(**R.kwargs_of(inp, t))["terms_n"], "model " + path)
