"""Golden vectors of the SI training objective and the epoch metrics, written from the reference's OWN train_epoch and evaluate_epoch
(subgraph_isomorphism/train.py:596-998, :1001-1222), imported unchanged with the stand-ins of _ref_standins.py and driven with stub
models that return dicts of leaf tensors, list-like loaders, an optimizer whose step / zero_grad do nothing and a writer that keeps
add_scalar's values.

Run on the authoring box only (needs the reference checkout and scikit-learn):  python tests/golden/make_golden_si_objective.py
Writes si_objective.npz (data only): a JSON meta plus arrays named <case>/<what>:
  exact_*    three cases, one per criterion, every value a multiple of 1/8: the fp32 results equal an fp64 evaluation bit for bit
  gen_*      randn values, B in {1, 5}, every presence combination, both representation ranks
  epoch      one train_epoch of three batches (per-step terms, the returned epoch averages)
  eval_*     two evaluate_epoch runs of three batches each
  schedules  schedule values over specs x steps, read back from train_epoch's own writer calls
  model      one RGIN with pred_return_weights="node" through train_epoch: terms and every parameter gradient"""
import json
import os
import sys

import numpy as np
import torch as th

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import _ref_standins as S  # noqa: E402

S.install()
import make_golden_si_models as M  # noqa: E402
import objective_ref as OR  # noqa: E402

MODELS = M._si_modules()                 # (also puts the reference's subgraph_isomorphism on sys.path)
import train as T  # noqa: E402

REP_KEYS = ("p_v_rep", "p_e_rep", "g_v_rep", "g_e_rep")
OUT_KEYS = ("pred_c", "pred_v", "pred_e", "g_v_mask", "g_e_mask") + REP_KEYS
TERM_TAGS = ("train/eval-%(eval_metric)s", "train/train-%(bp_loss)s", "train/match_v_loss", "train/match_e_loss", "train/match_v_reg",
             "train/match_e_reg", "train/rep_reg")
SCALAR_TAGS = ("train/neg_slp", "train/match_loss_w", "train/match_reg_w", "train/rep_reg_w")


class Movable:
    def to(self, device):
        return self


class Loader(list):
    dataset = None


class Writer:
    def __init__(self):
        self.values = {}

    def add_scalar(self, tag, value, step):
        self.values.setdefault(tag, []).append((step, value))


class Optimizer:
    def step(self):
        pass

    def zero_grad(self):
        pass


class StubModel:
    """Returns the prepared output dicts in turn; the weights pass through refine_* unchanged (basemodel.py's default)."""

    def __init__(self, outputs):
        self.outputs, self.calls = outputs, 0

    def train(self):
        return self

    def eval(self):
        return self

    def parameters(self):
        return []

    def refine_node_weights(self, w, use_max=False):
        return w

    def refine_edge_weights(self, w, use_max=False):
        return w

    def __call__(self, pattern, graph):
        self.calls += 1
        return self.outputs[self.calls - 1]


def config(bp_loss="MSE", eval_metric="MSE", neg_pred_slp=0.25, match_loss_w=0.5, match_reg_w=0.25, rep_reg_w=0.125, train_epochs=1):
    return dict(bp_loss=bp_loss, eval_metric=eval_metric, neg_pred_slp=neg_pred_slp, match_loss_w=match_loss_w, match_reg_w=match_reg_w,
                rep_reg_w=rep_reg_w, train_epochs=train_epochs, lr=1e-3, train_grad_steps=1, max_grad_norm=0.0, train_log_steps=1)


def leaf_output(arrs, dtype=th.float32):
    """The stub's output dict: float entries as leaves that take a gradient, masks as bool tensors, the rest None."""
    out = {k: None for k in ("p_v_emb", "p_e_emb", "g_v_emb", "g_e_emb", "p_v_mask", "p_e_mask") + OUT_KEYS}
    for k, a in arrs.items():
        a = np.asarray(a)
        out[k] = th.from_numpy(a.copy()) if a.dtype == bool else th.from_numpy(a.astype(np.float64)).to(dtype).requires_grad_(True)
    return out


def run_train(batches, cfg, is_graph=True, epoch=0, dtype=th.float32):
    """batches: [(arrs of OUT_KEYS, counts, node_weights | None, edge_weights | None)].  -> per-step terms [steps, 7], scalars [steps, 4],
    the .grad of every float leaf of every batch, the returned (eval, bp_loss) epoch averages."""
    outputs = [leaf_output(b[0], dtype) for b in batches]
    loader = Loader()
    for arrs, counts, nw, ew in batches:
        loader.append((list(range(len(counts))), Movable(), Movable(), th.from_numpy(np.asarray(counts)),
                       (None if nw is None else th.from_numpy(np.asarray(nw).copy()), None if ew is None else th.from_numpy(np.asarray(ew).copy()))))
    if not is_graph:
        loader.dataset = T.EdgeSeqDataset()
    writer = Writer()
    avg = T.train_epoch(StubModel(outputs), Optimizer(), None, "train", loader, th.device("cpu"), cfg, epoch, logger=None, writer=writer)
    terms = np.array([[v for _, v in writer.values[t % cfg]] for t in TERM_TAGS], dtype=np.float64).T
    scalars = np.array([[v for _, v in writer.values[t]] for t in SCALAR_TAGS], dtype=np.float64).T
    grads = [{k: (None if t.grad is None else t.grad.double().numpy()) for k, t in o.items() if t is not None and t.dtype.is_floating_point}
             for o in outputs]
    return terms, scalars, grads, np.array(avg, dtype=np.float64)


def ref_kwargs(arrs, counts, nw, ew, cfg, is_graph=True):
    """The restatement's arguments of one batch (the skips of train.py:779 and :790 applied)."""
    kw = dict(pred_c=arrs["pred_c"], counts=counts, bp_loss=cfg["bp_loss"], eval_metric=cfg["eval_metric"], neg_slp=cfg["neg_pred_slp"],
              rep_reg_w=cfg["rep_reg_w"], match_loss_w=cfg["match_loss_w"], match_reg_w=cfg["match_reg_w"],
              reps=[arrs[k] for k in REP_KEYS if k in arrs])
    if nw is not None and "pred_v" in arrs and is_graph:
        kw.update(pred_v=arrs["pred_v"], v_mask=arrs["g_v_mask"], v_target=nw)
    if ew is not None and "pred_e" in arrs:
        kw.update(pred_e=arrs["pred_e"], e_mask=arrs["g_e_mask"], e_target=ew)
    return kw


def store(out, tag, arrs, counts, nw, ew, terms=None, grads=None):
    for k, a in arrs.items():
        out["%s/in/%s" % (tag, k)] = np.asarray(a)
    out["%s/in/counts" % tag] = np.asarray(counts)
    if nw is not None:
        out["%s/in/node_weights" % tag] = np.asarray(nw)
    if ew is not None:
        out["%s/in/edge_weights" % tag] = np.asarray(ew)
    if terms is not None:
        out["%s/terms" % tag] = terms
    for k, g in (grads or {}).items():
        if g is not None:
            out["%s/grad/%s" % (tag, k)] = g


def eighths(rng, shape, lo=-4.0, hi=4.0):
    return rng.integers(int(lo * 8), int(hi * 8) + 1, size=shape).astype(np.float64) / 8


def mask_of(rng, B, L, empty_row=None):
    """Pre-padded masks as the models build them: the last n positions kept, n >= 1 (0 in the fully masked row)."""
    n = rng.integers(1, L + 1, size=B)
    if empty_row is not None:
        n[empty_row] = 0
    return np.arange(L)[None, :] >= (L - n)[:, None]


def make_exact(out, meta):
    for cid, crit in enumerate(("MAE", "MSE", "SMSE")):
        rng = np.random.default_rng(4100 + cid)
        B, Lv, Le, H = 4, 8, 16, 8
        arrs = dict(pred_c=np.array([[-1.5], [2.25], [0.75], [-0.375]]), pred_v=eighths(rng, (B, Lv)), pred_e=eighths(rng, (B, Le)),
                    g_v_mask=mask_of(rng, B, Lv, empty_row=3), g_e_mask=mask_of(rng, B, Le, empty_row=3),
                    p_v_rep=eighths(rng, (8, H)), g_v_rep=eighths(rng, (16, H)))
        counts = np.array([0, 2, 1, 3], dtype=np.int64)
        nw, ew = eighths(rng, (B, Lv), 0.0, 4.0), eighths(rng, (B, Le), 0.0, 4.0)
        cfg = config(bp_loss=crit, eval_metric=("MSE", "SMSE", "MAE")[cid])
        terms, scalars, grads, avg = run_train([(arrs, counts, nw, ew)], cfg)
        assert (terms != 0).all(), (crit, terms)
        want = OR.objective(**ref_kwargs(arrs, counts, nw, ew, cfg))
        assert np.array_equal(terms[0], want["terms"]), (crit, terms[0], want["terms"])       # fp32 == fp64, bit for bit
        g = grads[0]
        for k, w in (("pred_c", want["grads"]["pred_c"].reshape(-1, 1)), ("pred_v", want["grads"]["pred_v"]), ("pred_e", want["grads"]["pred_e"]),
                     ("p_v_rep", want["grads"]["reps"][0]), ("g_v_rep", want["grads"]["reps"][1])):
            assert np.array_equal(g[k], w), (crit, k)
        assert (g["pred_v"][3] != 0).all() and (g["pred_e"][3] != 0).all()                   # the fully masked row, pred_c < 0: the regulariser's gradient
        if crit != "MSE":                                                                    # the reference loop itself on double leaves
            t64, _, g64, _ = run_train([(arrs, counts, nw, ew)], cfg, dtype=th.float64)
            assert np.array_equal(t64[0], terms[0]) and all(np.array_equal(g64[0][k], g[k]) for k in g), crit
        tag = "exact_" + crit
        store(out, tag, arrs, counts, nw, ew, terms[0], g)
        meta["cases"].append(dict(tag=tag, kind="exact", cfg=cfg, is_graph=True))


def make_general(out, meta):
    combos = ("c_only", "reps", "v_only", "e_only", "all", "not_graph")
    cid = 0
    for B in (1, 5):
        for combo in combos:
            rng = np.random.default_rng(4200 + cid)
            Lv, Le, H = 7, 13, 6
            arrs = dict(pred_c=rng.standard_normal((B, 1)))
            if combo == "c_only" and B == 5:
                arrs["pred_c"][0, 0] = -abs(arrs["pred_c"][0, 0])
            if combo in ("v_only", "all", "not_graph"):
                arrs.update(pred_v=rng.standard_normal((B, Lv)), g_v_mask=mask_of(rng, B, Lv, empty_row=B - 1 if B > 1 else None))
            if combo in ("e_only", "all", "not_graph"):
                arrs.update(pred_e=rng.standard_normal((B, Le)), g_e_mask=mask_of(rng, B, Le))
            if combo in ("reps", "all"):                                                     # ragged rows of the graph models
                arrs.update(p_v_rep=rng.standard_normal((3 * B, H)), g_v_rep=rng.standard_normal((5 * B + 1, H)))
            if combo == "all":
                arrs.update(p_e_rep=rng.standard_normal((4 * B, H)), g_e_rep=rng.standard_normal((7 * B, H)))
            if combo == "not_graph":                                                         # padded rows of the sequence models
                arrs.update(p_e_rep=rng.standard_normal((B, 4, H)), g_e_rep=rng.standard_normal((B, Le, H)))
            counts = rng.integers(0, 4, size=B).astype(np.int64)
            nw = np.abs(rng.standard_normal((B, Lv))) if "pred_v" in arrs else None
            ew = np.abs(rng.standard_normal((B, Le))) if "pred_e" in arrs else None
            if combo == "reps":                                                              # weights without a prediction: skipped (train.py:779)
                nw = np.abs(rng.standard_normal((B, Lv)))
            crit = ("MAE", "MSE", "SMSE")[cid % 3]
            cfg = config(bp_loss=crit, eval_metric=("SMSE", "MAE", "MSE")[cid % 3], neg_pred_slp=0.01 + 0.1 * (cid % 4), match_loss_w=0.7,
                         match_reg_w=0.3, rep_reg_w=0.05)
            is_graph = combo != "not_graph"
            arrs = {k: (a if a.dtype == bool else a.astype(np.float32)) for k, a in arrs.items()}
            nw, ew = (None if a is None else a.astype(np.float32) for a in (nw, ew))
            terms, scalars, grads, avg = run_train([(arrs, counts, nw, ew)], cfg, is_graph=is_graph)
            tag = "gen_%s_B%d" % (combo, B)
            store(out, tag, arrs, counts, nw, ew, terms[0], grads[0])
            meta["cases"].append(dict(tag=tag, kind="general", cfg=cfg, is_graph=is_graph))
            cid += 1


def make_epoch(out, meta):
    rng = np.random.default_rng(4300)
    batches = []
    for B in (3, 5, 2):
        arrs = dict(pred_c=rng.standard_normal((B, 1)), pred_v=rng.standard_normal((B, 7)), g_v_mask=mask_of(rng, B, 7),
                    p_v_rep=rng.standard_normal((2 * B, 6)), g_v_rep=rng.standard_normal((4 * B, 6)))
        arrs = {k: (a if a.dtype == bool else a.astype(np.float32)) for k, a in arrs.items()}
        batches.append((arrs, rng.integers(0, 4, size=B).astype(np.int64), np.abs(rng.standard_normal((B, 7))).astype(np.float32), None))
    cfg = config(neg_pred_slp="anneal_cosine$1.0$0.01", match_loss_w=1.0, match_reg_w="anneal_cosine$0.01$0.0", rep_reg_w=1e-5, train_epochs=4)
    terms, scalars, grads, avg = run_train(batches, cfg, epoch=1)
    for i, (arrs, counts, nw, ew) in enumerate(batches):
        store(out, "epoch/%d" % i, arrs, counts, nw, ew, terms[i])
    out["epoch/scalars"] = scalars
    out["epoch/avg"] = avg
    meta["epoch"] = dict(cfg=cfg, epoch=1, steps=len(batches), total_steps=4 * len(batches))


def make_eval(out, meta):
    meta["eval"] = []
    for rid, (is_graph, with_v) in enumerate(((True, True), (False, True))):
        rng = np.random.default_rng(4400 + rid)
        outputs, loader = [], Loader()
        if not is_graph:
            loader.dataset = T.EdgeSeqDataset()
        for i, B in enumerate((4, 3, 5)):
            arrs = dict(pred_c=rng.standard_normal((B, 1)), pred_v=rng.standard_normal((B, 7)), g_v_mask=mask_of(rng, B, 7),
                        pred_e=rng.standard_normal((B, 13)), g_e_mask=mask_of(rng, B, 13))
            if rid == 0 and i == 1:
                del arrs["pred_e"], arrs["g_e_mask"]                                         # a batch without edge predictions: EED 0
            arrs = {k: (a if a.dtype == bool else a.astype(np.float32)) for k, a in arrs.items()}
            counts = rng.integers(0, 3, size=B).astype(np.int64)
            counts[0], counts[-1] = 0, 2                                                     # both classes in every run
            nw, ew = np.abs(rng.standard_normal((B, 7))).astype(np.float32), np.abs(rng.standard_normal((B, 13))).astype(np.float32)
            outputs.append(leaf_output(arrs))
            loader.append((list(range(B)), Movable(), Movable(), th.from_numpy(counts), (th.from_numpy(nw.copy()), th.from_numpy(ew.copy()))))
            store(out, "eval_%d/%d" % (rid, i), arrs, counts, nw, ew)
        cfg = config(eval_metric=("MAE", "SMSE")[rid])
        avg, res = T.evaluate_epoch(StubModel(outputs), "dev", loader, th.device("cpu"), cfg, 0, logger=None, writer=Writer())
        err = res["error"]
        for k in ("AE", "SE", "NED", "EED"):
            out["eval_%d/%s" % (rid, k)] = err[k].detach().numpy()
        out["eval_%d/scalars" % rid] = np.array([err[k] for k in ("MAE", "MSE", "RMSE", "MNED", "MEED", "AUC")] + [avg], dtype=np.float64)
        meta["eval"].append(dict(tag="eval_%d" % rid, is_graph=is_graph, batches=3, eval_metric=cfg["eval_metric"]))


def make_schedules(out, meta):
    specs = [0.25, 1, "anneal_cosine$1.0$0.01", "anneal_cosine$0.01$0.0", "anneal_linear$0.0$2.0", "anneal_constant$1.0$0.5", "anneal_$3.0$0.5",
             "cyclical_cosine$1.0$0.01", "cyclical_linear$0.0$2.0", "cyclical_none$1.0$0.25"]
    total = 12
    steps = list(range(0, total + 2))                                                        # one step behind the last one too
    arrs = dict(pred_c=np.ones((1, 1), np.float32))
    table = np.zeros((len(specs), len(steps)), dtype=np.float64)
    for i, spec in enumerate(specs):
        for j, step in enumerate(steps):
            cfg = config(neg_pred_slp=spec, train_epochs=total)                              # one batch an epoch: step = epoch, total_steps = train_epochs
            _, scalars, _, _ = run_train([(arrs, np.array([1]), None, None)], cfg, epoch=step)
            table[i, j] = scalars[0, 0]
    out["schedules/table"] = table
    meta["schedules"] = dict(specs=specs, steps=steps, total_steps=total)


class MovableGraph(M.BatchedFakeGraph, Movable):
    pass


def make_model(out, meta):
    cfg = dict(M.BASE_CFG)
    cfg.update(pred_return_weights="node")
    rng = np.random.default_rng(4500)
    B = 6
    pb = M._batch(rng, B, 2, 5, cfg["max_npv"], cfg["max_npvl"], cfg["max_npel"], True, False)
    gb = M._batch(rng, B, 3, 9, cfg["max_ngv"], cfg["max_ngvl"], cfg["max_ngel"], True, False)
    seed = 9500
    th.manual_seed(seed)
    model = MODELS["RGIN"](**cfg)
    with th.no_grad():
        for p in model.parameters():
            if p.requires_grad:
                p.add_(0.05 * th.randn_like(p))
    alias, first = {}, {}
    for k, t in model.state_dict(keep_vars=True).items():
        if id(t) in first:
            alias[k] = first[id(t)]
        else:
            first[id(t)] = k
    for k, t in model.state_dict().items():
        if k not in alias:
            out["model/param/%s" % k] = t.numpy().copy()
    for side, d in (("p", pb), ("g", gb)):
        for k, a in d.items():
            out["model/%s/%s" % (side, k)] = a

    def fake(d):
        g = MovableGraph(d["u"], d["v"], d["sizes"])
        g.ndata["id"], g.ndata["label"] = th.from_numpy(d["id"]), th.from_numpy(d["label"])
        g.ndata["is_dummy"] = th.from_numpy(d["dummy"])
        g.edata["label"] = th.from_numpy(d["elabel"])
        return g

    counts = rng.integers(0, 4, size=B).astype(np.int64)
    nw = rng.integers(0, 3, size=(B, int(gb["sizes"].max()))).astype(np.float32)
    out["model/counts"], out["model/node_weights"] = counts, nw
    loader = Loader([(list(range(B)), fake(pb), fake(gb), th.from_numpy(counts), (th.from_numpy(nw.copy()), None))])
    tcfg = config(neg_pred_slp=0.05, match_loss_w=1.0, match_reg_w=0.01, rep_reg_w=1e-5)
    writer = Writer()
    T.train_epoch(model, Optimizer(), None, "train", loader, th.device("cpu"), tcfg, 0, logger=None, writer=writer)
    terms = np.array([writer.values[t % tcfg][0][1] for t in TERM_TAGS], dtype=np.float64)
    assert terms[2] != 0 and terms[4] != 0 and terms[6] != 0, terms
    out["model/terms"] = terms
    none_grad = []
    for k, p in model.named_parameters():
        if p.grad is None:
            none_grad.append(k)
        else:
            out["model/grad/%s" % k] = p.grad.numpy()
    meta["model"] = dict(cfg=cfg, train_cfg=tcfg, seed=seed, B=B, alias=alias, keys=list(model.state_dict().keys()), none_grad=none_grad)


def make():
    out, meta = {}, {"cases": []}
    make_exact(out, meta)
    make_general(out, meta)
    make_epoch(out, meta)
    make_eval(out, meta)
    make_schedules(out, meta)
    make_model(out, meta)
    out["meta"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    path = os.path.join(HERE, "si_objective.npz")
    np.savez_compressed(path, **out)
    print("si_objective.npz: %d arrays, %d bytes" % (len(out), os.path.getsize(path)))


if __name__ == "__main__":
    make()
