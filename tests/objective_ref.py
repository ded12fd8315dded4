"""Float64 restatement of the SI training objective and of the per-sample evaluation errors (subgraph_isomorphism/train.py:776-813,
:1101-1173), written from the formulas on numpy arrays, gradients by hand with torch's derivative conventions:

    crit(d)  = |d| (MAE), d^2 (MSE), smooth-L1 at beta 1 (SMSE)            crit'(d): sign(d) with sign(0) = 0; 2 d; d inside |d| < 1
    eval     = 1/B sum_b crit_eval(relu(pred_c_b) - c_b)
    bp       = 1/B sum_b crit(lrelu(pred_c_b, s) - c_b)                     lrelu' = 1 for x > 0, else s;  relu' = (x > 0)
    x_loss   = 1/B sum_bj crit(lrelu(m p_bj, s) - m w_bj)
    x_reg    = 1/B sum_bj crit(relu(m p_bj - pred_c_b))                     all positions; the gradient reaches masked ones too
    rep_reg  = sum_reps sum crit(rep) / (numel / rep.shape[1])
    loss     = bp + rep_reg_w rep_reg + match_loss_w (v_loss + e_loss) + match_reg_w (v_reg + e_reg)

Besides the values it returns, per output, the number of addends n and the sum of their magnitudes: the tests' bounds are
(n + 8) u times those (tests/test_si_objective_host.py pins this file against the goldens the reference itself produced)."""
import numpy as np

TERMS = ("eval", "bp_loss", "match_v_loss", "match_e_loss", "match_v_reg", "match_e_reg", "rep_reg")


def crit(name, d):
    a = np.abs(d)
    if name == "MAE":
        return a
    if name == "MSE":
        return d * d
    if name == "SMSE":
        return np.where(a < 1.0, 0.5 * d * d, a - 0.5)
    raise NotImplementedError(name)


def dcrit(name, d):
    if name == "MAE":
        return np.sign(d)
    if name == "MSE":
        return 2.0 * d
    if name == "SMSE":
        return np.where(np.abs(d) < 1.0, d, np.sign(d))
    raise NotImplementedError(name)


def lrelu(x, s):
    return np.where(x > 0, x, x * s)


def _f64(a):
    return None if a is None else np.asarray(a, dtype=np.float64)


def objective(pred_c, counts, bp_loss, eval_metric, neg_slp, rep_reg_w, match_loss_w, match_reg_w, reps=(), pred_v=None, v_mask=None,
              v_target=None, pred_e=None, e_mask=None, e_target=None):
    """-> dict: terms [7] (order TERMS), terms_n [7] (addends of each), loss, grads {pred_c [B], pred_v, pred_e, reps [..]} of the loss,
    pred_c_n / pred_c_abs [B]: the addends of each d pred_c and the sum of their magnitudes; abs {pred_v, pred_e}: the sum of the
    magnitudes of the two addends of each d pred_x (the match loss's and the regulariser's)."""
    pc, c = _f64(pred_c).reshape(-1), _f64(counts).reshape(-1)
    B, s = pc.size, float(neg_slp)
    ev = crit(eval_metric, np.maximum(pc, 0.0) - c).sum() / B
    bp = crit(bp_loss, lrelu(pc, s) - c).sum() / B
    d_pc = np.where(pc > 0, 1.0, s) * dcrit(bp_loss, lrelu(pc, s) - c) / B
    pc_n, pc_abs = np.ones(B), np.abs(d_pc)
    sides, grads, mags = {}, {"pred_v": None, "pred_e": None}, {}
    for x, pred, mask, target in (("v", pred_v, v_mask, v_target), ("e", pred_e, e_mask, e_target)):
        if pred is None or target is None:
            sides[x] = (0.0, 0.0, 0)
            continue
        m = np.asarray(mask).astype(bool).reshape(B, -1)
        p = np.where(m, _f64(pred).reshape(B, -1), 0.0)
        w = np.where(m, _f64(target).reshape(B, -1), 0.0)
        z = p - pc[:, None]
        loss = crit(bp_loss, lrelu(p, s) - w).sum() / B
        reg = crit(bp_loss, np.maximum(z, 0.0)).sum() / B
        t1 = np.where(p > 0, 1.0, s) * dcrit(bp_loss, lrelu(p, s) - w)
        t2 = np.where(z > 0, dcrit(bp_loss, z), 0.0)
        grads["pred_" + x] = ((match_loss_w / B) * t1 + (match_reg_w / B) * t2).reshape(np.shape(pred))
        mags["pred_" + x] = (np.abs((match_loss_w / B) * t1) + np.abs((match_reg_w / B) * t2)).reshape(np.shape(pred))
        d_pc = d_pc - (match_reg_w / B) * t2.sum(1)
        pc_n = pc_n + p.shape[1]
        pc_abs = pc_abs + np.abs((match_reg_w / B) * t2).sum(1)
        sides[x] = (loss, reg, p.size)
    rep_reg, rep_n, d_reps = 0.0, 0, []
    for r in reps:
        r64 = _f64(r)
        denom = r64.size // r64.shape[1]
        rep_reg = rep_reg + crit(bp_loss, r64).sum() / denom
        rep_n += r64.size
        d_reps.append(rep_reg_w * dcrit(bp_loss, r64) / denom)
    grads["reps"] = d_reps
    grads["pred_c"] = d_pc
    (vl, vr, vn), (el, er, en) = sides["v"], sides["e"]
    total = bp + rep_reg_w * rep_reg + match_loss_w * (vl + el) + match_reg_w * (vr + er)
    return {"terms": np.array([ev, total, vl, el, vr, er, rep_reg], dtype=np.float64),
            "terms_n": np.array([B, B + 2 * (vn + en) + rep_n, vn, en, vn, en, rep_n]), "loss": total, "grads": grads,
            "pred_c_n": pc_n, "pred_c_abs": pc_abs, "abs": mags}


def eval_errors(pred_c, counts, pred_v=None, v_target=None, pred_e=None, e_target=None):
    """-> AE, SE, NED, EED [B] float64 and cls [B] = (c > 0) + 2 (relu(pred_c) > 0); NED / EED over all positions, no mask, 0 when absent."""
    pc, c = np.maximum(_f64(pred_c).reshape(-1), 0.0), _f64(counts).reshape(-1)
    ae = np.abs(pc - c)

    def dist(pred, target):
        if pred is None or target is None:
            return np.zeros_like(ae)
        return np.abs(np.maximum(_f64(pred).reshape(ae.size, -1), 0.0) - _f64(target).reshape(ae.size, -1)).sum(1)

    return ae, ae * ae, dist(pred_v, v_target), dist(pred_e, e_target), (c > 0).astype(np.int64) + 2 * (pc > 0).astype(np.int64)


def auc(cls):
    """roc_auc_score of binary scores against binary labels from the four counts: (TPR + TNR) / 2."""
    tn, fn, fp, tp = (float(np.sum(np.asarray(cls) == k)) for k in (0, 1, 2, 3))
    return (tp / (tp + fn) + tn / (tn + fp)) / 2


# ------------------------------------------------------------------------------------------------ the goldens and the tests' bounds
import json  # noqa: E402
import os  # noqa: E402

import torch  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "si_objective.npz")
U = 2.0 ** -24
OUT_KEYS = ("p_v_emb", "p_e_emb", "g_v_emb", "g_e_emb", "p_v_rep", "p_e_rep", "g_v_rep", "g_e_rep", "p_v_mask", "p_e_mask", "g_v_mask",
            "g_e_mask", "pred_c", "pred_v", "pred_e")
REP_KEYS = ("p_v_rep", "p_e_rep", "g_v_rep", "g_e_rep")


def load_golden():
    """(meta, {name: array}) of si_objective.npz."""
    z = np.load(GOLDEN)
    return json.loads(bytes(z["meta"]).decode()), {k: z[k] for k in z.files if k != "meta"}


def inputs(arrays, tag):
    """{name: array} of <tag>/in/*."""
    pre = tag + "/in/"
    return {k[len(pre):]: v for k, v in arrays.items() if k.startswith(pre)}


def kwargs_of(inp, cfg, is_graph=True):
    """The restatement's arguments of one recorded batch (the skips of train.py:779 and :790 applied)."""
    kw = dict(pred_c=inp["pred_c"], counts=inp["counts"], bp_loss=cfg["bp_loss"], eval_metric=cfg["eval_metric"], neg_slp=cfg["neg_pred_slp"],
              rep_reg_w=cfg["rep_reg_w"], match_loss_w=cfg["match_loss_w"], match_reg_w=cfg["match_reg_w"],
              reps=[inp[k] for k in REP_KEYS if k in inp])
    if "node_weights" in inp and "pred_v" in inp and is_graph:
        kw.update(pred_v=inp["pred_v"], v_mask=inp["g_v_mask"], v_target=inp["node_weights"])
    if "edge_weights" in inp and "pred_e" in inp:
        kw.update(pred_e=inp["pred_e"], e_mask=inp["g_e_mask"], e_target=inp["edge_weights"])
    return kw


def check_terms(got, golden, n, what=""):
    """A term is a sum of n non-negative addends: |x - golden| <= (n + 8) u golden."""
    got, golden = np.asarray(got, np.float64), np.asarray(golden, np.float64)
    err, bound = np.abs(got - golden), (np.asarray(n) + 8) * U * np.abs(golden)
    print("%s terms err %s bound %s" % (what, err.tolist(), bound.tolist()))
    assert (err <= bound).all(), (what, got.tolist(), golden.tolist(), err.tolist(), bound.tolist())


def check_elementwise(got, golden, what="", extra=0.0):
    """A product of at most five rounded factors: relative 16 u (+ extra: one more rounding of a bf16 result), exact zero where the
    golden is zero."""
    got, golden = np.asarray(got, np.float64), np.asarray(golden, np.float64)
    assert got.shape == golden.shape, (what, got.shape, golden.shape)
    zero = golden == 0
    assert (got[zero] == 0).all(), (what, "non-zero where the golden is zero")
    rel = np.abs(got[~zero] - golden[~zero]) / np.abs(golden[~zero])
    print("%s elementwise rel max %.3e of %.3e" % (what, rel.max() if rel.size else 0.0, 16 * U + extra))
    assert (rel <= 16 * U + extra).all(), (what, float(rel.max()))


def check_pred_c_grad(got, golden, n, mag, what="", extra=0.0):
    """d pred_c mixes signs: (n + 8) u sum|addends| (+ extra |golden|)."""
    got, golden = np.asarray(got, np.float64).reshape(-1), np.asarray(golden, np.float64).reshape(-1)
    err, bound = np.abs(got - golden), (np.asarray(n) + 8) * U * np.asarray(mag) + extra * np.abs(golden)
    print("%s d pred_c err max %.3e bound min %.3e" % (what, err.max(), bound.min()))
    assert (err <= bound).all(), (what, err.tolist(), bound.tolist())


def check_two_addends(got, golden, mag, what=""):
    """An exact evaluation against the reference's fp32 one, for d pred_x = the match loss's product + the regulariser's: each
    product carries the elementwise rule's 16 u of its own magnitude and their sum one more rounding, so
    |x - golden| <= 16 u (|a1| + |a2|) + u |golden|; where one addend is zero this is the elementwise rule (and zero stays zero)."""
    got, golden, mag = (np.asarray(a, np.float64) for a in (got, golden, mag))
    assert (got[golden == 0] == 0).all(), (what, "non-zero where the golden is zero")
    single = mag == np.abs(got)
    err, bound = np.abs(got - golden), 16 * U * mag + np.where(single, 0.0, U * np.abs(golden))
    print("%s two-addend err/bound max %.3f (%d of %d elements have both addends)" % (what, (err / np.maximum(bound, 1e-300)).max(),
                                                                                     int((~single).sum()), got.size))
    assert (err <= bound).all(), (what, float((err / np.maximum(bound, 1e-300)).max()))


# ------------------------------------------------------------------------------------------------ shared by the host and the GPU tests
_GOLDEN = None


def golden():
    """(meta, arrays, {tag: case}) of si_objective.npz, read once."""
    global _GOLDEN
    if _GOLDEN is None:
        meta, arrays = load_golden()
        _GOLDEN = (meta, arrays, {c["tag"]: c for c in meta["cases"]})
    return _GOLDEN


def output_of(inp, dev="cpu", dtype=torch.float32, grad=True):
    out = {k: None for k in OUT_KEYS}
    for k in OUT_KEYS:
        if k in inp:
            t = torch.from_numpy(np.array(inp[k])).to(dev)
            out[k] = t if t.dtype == torch.bool else t.to(dtype).requires_grad_(grad)
    return out


def weights_of(inp, dev="cpu"):
    return tuple(None if k not in inp else torch.from_numpy(np.array(inp[k])).to(dev) for k in ("node_weights", "edge_weights"))


def objective_of(cfg, total_steps=1):
    from dummynode4graphlearning_amd.subgraph_isomorphism import SIObjective
    return SIObjective(bp_loss=cfg["bp_loss"], eval_metric=cfg["eval_metric"], neg_pred_slp=cfg["neg_pred_slp"], match_loss_w=cfg["match_loss_w"],
                       match_reg_w=cfg["match_reg_w"], rep_reg_w=cfg["rep_reg_w"], total_steps=total_steps)


def run_case(tag, dev="cpu", dtype=torch.float32):
    case, inp = golden()[2][tag], inputs(golden()[1], tag)
    out = output_of(inp, dev, dtype)
    nw, ew = weights_of(inp, dev)
    loss, terms = objective_of(case["cfg"])(out, torch.from_numpy(inp["counts"]).to(dev), nw, ew, is_graph=case["is_graph"])
    loss.backward()
    return out, loss, terms


def grads_of(tag):
    pre = tag + "/grad/"
    return {k[len(pre):]: v for k, v in golden()[1].items() if k.startswith(pre)}


def check_against_golden(tag, terms, grads, what, extra=0.0, skip=()):
    """terms [7] and {leaf: gradient} of one general case against its golden, by the derived bounds (skip: leaves checked elsewhere)."""
    case, inp = golden()[2][tag], inputs(golden()[1], tag)
    want = objective(**kwargs_of(inp, case["cfg"], case["is_graph"]))
    check_terms(terms, golden()[1][tag + "/terms"], want["terms_n"], "%s %s" % (what, tag))
    gold = {k: g for k, g in grads_of(tag).items() if k not in skip}
    assert sorted(k for k, g in grads.items() if g is not None) == sorted(gold), (sorted(grads), sorted(gold))
    for k, g in gold.items():
        if k == "pred_c":
            check_pred_c_grad(grads[k], g, want["pred_c_n"], want["pred_c_abs"], "%s %s" % (what, tag), extra)
        else:
            check_elementwise(grads[k], g, "%s %s %s" % (what, tag, k), extra)


def eval_meter(run, dev="cpu"):
    from dummynode4graphlearning_amd.subgraph_isomorphism import SIEvalMeter
    meter = SIEvalMeter(capacity=16)
    for i in range(run["batches"]):
        inp = inputs(golden()[1], "%s/%d" % (run["tag"], i))
        nw, ew = weights_of(inp, dev)
        meter.update(output_of(inp, dev, grad=False), torch.from_numpy(inp["counts"]).to(dev), nw, ew, is_graph=run["is_graph"])
    return meter


def check_eval_result(run, res):
    """AE / SE are single rounded operations (equal); NED / EED sums of L addends; the means sums of n; AUC a handful of double operations."""
    tag = run["tag"]
    n = len(golden()[1][tag + "/AE"])
    assert sorted(res) == sorted(["AE", "SE", "NED", "EED", "MAE", "MSE", "RMSE", "MNED", "MEED", "AUC"])        # no ragged lists
    assert np.array_equal(res["AE"].numpy(), golden()[1][tag + "/AE"]) and np.array_equal(res["SE"].numpy(), golden()[1][tag + "/SE"])
    for k, L in (("NED", 7), ("EED", 13)):
        check_terms(res[k].numpy(), golden()[1]["%s/%s" % (tag, k)], L, "%s %s" % (tag, k))
    mae, mse, rmse, mned, meed, auc, _ = golden()[1][tag + "/scalars"]
    check_terms([res["MAE"], res["MSE"], res["RMSE"]], [mae, mse, rmse], n, tag)
    check_terms([res["MNED"], res["MEED"]], [mned, meed], n * 13 + n, tag)
    assert abs(res["AUC"] - auc) <= 1e-12
    if not run["is_graph"]:
        assert mned == 0 and res["MNED"] == 0
