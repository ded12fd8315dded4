"""Golden vectors of the attention count heads and DIAMNet (subgraph_isomorphism/models/pred.py), run on the CPU from the reference's
own code with the stand-ins of _ref_standins.py.

Run on the authoring box only (needs the reference checkout), like make_golden_si_models.py:
    python tests/golden/make_golden_si_attn.py
Writes si_attn.npz (data only).  No further stand-ins are needed.

Per head case: the class and its keyword arguments, the seed, the state_dict at construction (keys in order, values), the perturbed
parameters the run used, the padded inputs and masks (masked rows zero, as the models hand them over), y, w, the gradients of both
inputs and of every parameter under loss = sum(y * c) (+ sum(w * c_w)), and the parameters whose gradient is None.
Per whole model (the reference constructors with pred_net set): what make_golden_si_models.py / make_golden_si_dual_models.py store."""
import importlib
import json
import os
import sys

import numpy as np
import torch as th

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_si_models as M  # noqa: E402  (installs the stand-ins)
import make_golden_si_dual_models as D  # noqa: E402

ATTN = ("MeanAttnPredictNet", "SumAttnPredictNet", "MaxAttnPredictNet")


def _lens_mask(B, L, lens, dummy):
    """Pre-padded [B, L] mask: the last lens[b] positions are rows; dummy[b] (an offset inside the rows, or None) is cleared."""
    m = np.zeros((B, L), bool)
    for b in range(B):
        m[b, L - lens[b]:] = True
        if dummy[b] is not None:
            m[b, L - lens[b] + dummy[b]] = False
    return m


# (name, class, kwargs, input_dim, pattern lens, pattern dummies, graph lens, graph dummies)
HEAD_CASES = []
for _i, _cls in enumerate(ATTN):
    for _rw in (False, True):
        HEAD_CASES.append(("%s_rw%d" % (_cls, _rw), _cls, dict(hidden_dim=8, num_heads=(1, 4, 4)[_i], infer_steps=_i + 1, return_weights=_rw),
                           12, [3, 1, 4], [0, None, 3], [7, 5, 6], [6, 2, 0]))
for _mi in ("mean", "sum", "max"):
    for _rw in (False, True):
        # graph lengths: L <= mem_len (3, 4 rows between the first and the last unmasked row), mem_len + 1, 11 (stride 2, kernel 5)
        HEAD_CASES.append(("DIAMNet_%s_rw%d" % (_mi, _rw), "DIAMNet",
                           dict(hidden_dim=8, num_heads=4 if _mi != "sum" else 1, infer_steps=2 if _mi == "mean" else 1, mem_len=4,
                                mem_init=_mi, return_weights=_rw),
                           12, [3, 1, 4, 2, 3], [0, None, 3, None, 1], [3, 5, 6, 12, 12], [None, 4, 0, 11, 5]))
HEAD_CASES.append(("DIAMNet_mean_steps3", "DIAMNet", dict(hidden_dim=16, num_heads=4, infer_steps=3, mem_len=4, mem_init="mean"),
                   10, [2, 5], [None, 2], [9, 12], [3, None]))

# (name, reference module, class name, base cfg, overrides)
MODEL_CASES = [
    ("rgin_diamnet", "rgin", "RGIN", dict(pred_net="DIAMNet", pred_hid_dim=16, pred_num_heads=4, pred_infer_steps=2, pred_mem_len=4,
                                          pred_mem_init="mean")),
    ("rgin_maxattn", "rgin", "RGIN", dict(pred_net="MaxAttnPredictNet", pred_hid_dim=16, pred_num_heads=4, pred_infer_steps=2)),
    ("dmpnn_meanattn", "dmpnn", "DMPNN", dict(rep_net="DMPNN", pred_net="MeanAttnPredictNet", pred_hid_dim=16, pred_num_heads=2,
                                              pred_infer_steps=1)),
]


def _heads():
    M._si_modules()
    return importlib.import_module("models.pred")


def make():
    pred = _heads()
    out, meta = {}, []
    for cid, (name, cls, kw, D_in, plens, pdum, glens, gdum) in enumerate(HEAD_CASES):
        rng = np.random.default_rng(4100 + cid)
        seed = 9500 + cid
        th.manual_seed(seed)
        net = getattr(pred, cls)(D_in, **kw)
        tag = "h%02d" % cid
        arrs = {}
        keys = list(net.state_dict().keys())
        for k, t in net.state_dict().items():
            arrs["init/%s" % k] = t.numpy().copy()
        with th.no_grad():
            for p in net.parameters():
                p.add_(0.1 * th.randn_like(p))
        for k, t in net.state_dict().items():
            arrs["param/%s" % k] = t.numpy().copy()
        B = len(plens)
        Lp, Lg = max(plens), max(glens)
        pm, gm = _lens_mask(B, Lp, plens, pdum), _lens_mask(B, Lg, glens, gdum)
        p = rng.standard_normal((B, Lp, D_in)).astype(np.float32) * pm[..., None]
        g = rng.standard_normal((B, Lg, D_in)).astype(np.float32) * gm[..., None]
        pt, gt = th.from_numpy(p).requires_grad_(True), th.from_numpy(g).requires_grad_(True)
        net.train()
        y, w = net(pt, th.from_numpy(pm), gt, th.from_numpy(gm))
        c = th.from_numpy(rng.standard_normal((B, 1)).astype(np.float32))
        loss = (y * c).sum()
        arrs.update({"in/p": p, "in/g": g, "in/p_mask": pm, "in/g_mask": gm, "in/coef": c.numpy(), "out/y": y.detach().numpy()})
        if w is not None:
            cw = th.from_numpy(rng.standard_normal(tuple(w.shape)).astype(np.float32))
            loss = loss + (w * cw).sum()
            arrs.update({"in/coef_w": cw.numpy(), "out/w": w.detach().numpy()})
        loss.backward()
        arrs["grad_in/p"], arrs["grad_in/g"] = pt.grad.numpy(), gt.grad.numpy()
        none_grad = []
        for k, q in net.named_parameters():
            if q.grad is None:
                none_grad.append(k)
            else:
                arrs["grad/%s" % k] = q.grad.numpy()
        assert all(np.isfinite(a).all() for a in arrs.values() if a.dtype.kind == "f"), name
        m = dict(tag=tag, name=name, kind="head", cls=cls, kw=kw, input_dim=D_in, seed=seed, keys=keys, none_grad=none_grad,
                 params=[k for k, _ in net.named_parameters()], has_w=w is not None)
        m["index"] = M._pack(out, tag, arrs)
        meta.append(m)
        print("%s: y %s none_grad %s" % (name, np.round(arrs["out/y"].reshape(-1)[:3], 4), none_grad))
    for mid, (name, mod, clsname, over) in enumerate(MODEL_CASES):
        dual = clsname == "DMPNN"
        G = D if dual else M
        G._si_modules()
        Model = getattr(importlib.import_module("models." + mod), clsname)
        cfg = dict(G.BASE_CFG)
        cfg.update(over)
        rng = np.random.default_rng(4200 + mid)
        B = 5
        if dual:
            pb = D._batch(rng, B, 2, 3, cfg["max_npv"], cfg["max_npvl"], cfg["max_npel"], True, True, False)
            gb = D._batch(rng, B, 3, 5, cfg["max_ngv"], cfg["max_ngvl"], cfg["max_ngel"], True, True, False)
        else:
            pb = M._batch(rng, B, 2, 5, cfg["max_npv"], cfg["max_npvl"], cfg["max_npel"], True, False)
            gb = M._batch(rng, B, 6, 13, cfg["max_ngv"], cfg["max_ngvl"], cfg["max_ngel"], True, False)
        seed = 9600 + mid
        th.manual_seed(seed)
        model = Model(**cfg)
        tag = "m%02d" % mid
        arrs, alias, first = {}, {}, {}
        for k, t in model.state_dict(keep_vars=True).items():
            if id(t) in first:
                alias[k] = first[id(t)]
            else:
                first[id(t)] = k
        with th.no_grad():
            for p in model.parameters():
                if p.requires_grad:
                    p.add_(0.05 * th.randn_like(p))
        for k, t in model.state_dict().items():
            if k not in alias:
                arrs["param/%s" % k] = t.numpy().copy()
        for side, d in (("p", pb), ("g", gb)):
            for k, a in d.items():
                arrs["%s/%s" % (side, k)] = a
        model.train()
        res = model(G._fake(pb), G._fake(gb))
        c = th.arange(1, B + 1, dtype=th.float32).view(-1, 1) / B
        (res["pred_c"] * c).sum().backward()
        none_out = []
        for k in M.KEYS:
            if res[k] is None:
                none_out.append(k)
            else:
                arrs["out/%s" % k] = res[k].detach().numpy()
        none_grad = []
        for k, p in model.named_parameters():
            if p.grad is None:
                none_grad.append(k)
            else:
                arrs["grad/%s" % k] = p.grad.numpy()
        m = dict(tag=tag, name=name, kind="model", cls=clsname, cfg=cfg, seed=seed, B=B, none_out=none_out, none_grad=none_grad,
                 alias=alias, keys=list(model.state_dict().keys()), params=[k for k, _ in model.named_parameters()])
        m["index"] = M._pack(out, tag, arrs)
        meta.append(m)
        print("%s: pred_c %s" % (name, np.round(arrs["out/pred_c"].reshape(-1)[:3], 4)))
    out["meta"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    path = os.path.join(HERE, "si_attn.npz")
    np.savez_compressed(path, **out)
    print("si_attn.npz: %d cases, %d bytes" % (len(meta), os.path.getsize(path)))


if __name__ == "__main__":
    make()
