"""Golden vectors of the SI count model DMPLRP(**cfg) and of DMPLRPPoolLayer (subgraph_isomorphism/models/dmplrp.py), run on the
CPU from the reference's own code, unmodified, with the stand-ins of _ref_standins.py and the three sparse matrices of LRPDataset
(subgraph_isomorphism/dataset.py:1750-1886).

Run on the authoring box only (needs the reference checkout and scipy), like make_golden_si_lrp.py, whose batches, matrix builder
and packing this uses:
    python tests/golden/make_golden_si_dmplrp.py
Writes si_dmplrp.npz (data only).  Per case: the config, the batches, the sequences per node (lrp_split; the index lists
themselves are pinned by si_lrp.npz); for the model cases a sha256 of every initial state_dict tensor (the tensors themselves for
INIT_VALUE_CASES), the perturbed parameters, every OutputDict tensor, the gradient of every parameter and of the four rep tensors
under loss = sum(pred_c * c) + sum(pred_v * c_v) + sum(pred_e * c_e), and the buffers after the step; for the layer cases the
inputs, the coefficients of the loss, both outputs and the gradients of the inputs and parameters."""
import hashlib
import importlib
import json
import os
import sys

import numpy as np
import torch as th

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_si_lrp as G  # noqa: E402  (installs the stand-ins through make_golden_si_dual_models)

D = G.D
KEYS, REPS = D.KEYS, D.REPS

BASE_CFG = dict(D.BASE_CFG, rep_net="DMPLRP", rep_num_graph_layers=1, rep_num_pattern_layers=1, lrp_seq_len=4,
                rep_dmpnn_num_mlp_layers=2, rep_dmpnn_batch_norm=False, rep_act_func="relu", max_nge=256, max_npe=256)
for _k in [k for k in BASE_CFG if k.startswith("rep_compgcn")]:
    del BASE_CFG[_k]

_NO_SHARE = {"share_enc_net": False, "share_emb_net": False, "share_rep_net": False}
_TWO = {"rep_num_graph_layers": 2, "rep_num_pattern_layers": 2}
# (name, config overrides, batch options)
CASES = [
    ("dmplrp_l4_relu", dict(_TWO), {}),
    ("dmplrp_l3_leaky_bn", {"lrp_seq_len": 3, "rep_act_func": "leaky_relu", "rep_dmpnn_batch_norm": True}, {}),
    ("dmplrp_no_share", dict(_NO_SHARE, emb_net="Equivariant", lrp_seq_len=3), {"dummy_both": True}),
    ("dmplrp_no_dummy", {"rep_act_func": "leaky_relu"}, {"dummy": False}),
    ("dmplrp_no_reversed", {}, {"reversed": False}),
    ("dmplrp_no_filter_no_residual", {"filter_net": "None", "rep_residual": False, "lrp_seq_len": 3}, {"dummy_both": True}),
]
# (name, DMPLRPPoolLayer keyword arguments, batch options)
LAYER_CASES = [
    ("layer_l4_default", dict(lrp_seq_len=4), {}),
    ("layer_l3_no_mlp_leaky", dict(lrp_seq_len=3, num_mlp_layers=0, act_func="leaky_relu"), {"reversed": False}),
    ("layer_l2_no_bias", dict(lrp_seq_len=2, bias=False, batch_norm=False), {"dummy": False}),
    ("layer_l4_bn_dummy_both", dict(lrp_seq_len=4, batch_norm=True, act_func="leaky_relu"), {"dummy_both": True}),
]
INIT_VALUE_CASES = ("dmplrp_l3_leaky_bn",)
H = 16


def _modules():
    SI = os.path.join(D.REF, "subgraph_isomorphism")
    D._si_modules()                                                 # sys.path + the bare `models` package
    m = importlib.import_module("models.dmplrp")
    dataset = importlib.import_module("dataset")
    assert os.path.dirname(os.path.abspath(dataset.__file__)) == SI
    return m.DMPLRP, m.DMPLRPPoolLayer, dataset.LRPDataset


def _sha(t):
    return hashlib.sha256(t.numpy().tobytes()).hexdigest()[:24]


def make():
    DMPLRP, DMPLRPPoolLayer, LRPDataset = _modules()
    out, meta = {}, []
    for cid, (name, over, bopt) in enumerate(CASES):
        cfg = dict(BASE_CFG)
        cfg.update(over)
        L = cfg["lrp_seq_len"]
        rng = np.random.default_rng(3600 + cid)
        B = 4 + cid % 3
        pb, gb = G._batches(rng, cfg, bopt, B)
        seed = 8800 + cid
        th.manual_seed(seed)
        model = DMPLRP(**cfg)
        tag = "m%02d" % cid
        arrs = {}
        alias, first = {}, {}
        for k, t in model.state_dict(keep_vars=True).items():
            if id(t) in first:
                alias[k] = first[id(t)]
            else:
                first[id(t)] = k
        init_sha = {k: _sha(t) for k, t in model.state_dict().items()}
        if name in INIT_VALUE_CASES:
            for k, t in model.state_dict().items():
                if k not in alias:
                    arrs["init/%s" % k] = t.numpy().copy()
        shapes = {k: list(t.shape) for k, t in model.state_dict().items()}
        with th.no_grad():
            for p in model.parameters():
                if p.requires_grad:
                    p.add_(0.05 * th.randn_like(p))
        for k, t in model.state_dict().items():
            if k not in alias:
                arrs["param/%s" % k] = t.numpy().copy()
        mats = {}
        for side, d in (("p", pb), ("g", gb)):
            for k, a in d.items():
                arrs["%s/%s" % (side, k)] = a
            mats[side], lists = G._lrp_inputs(LRPDataset, d, L)
            arrs["%s/lrp_split" % side] = lists["lrp_split"]
        model.train()
        res = model(G._fake(pb), *mats["p"], G._fake(gb), *mats["g"])
        assert list(res.keys()) == list(KEYS), list(res.keys())
        for k in REPS:
            res[k].retain_grad()
        c = th.arange(1, B + 1, dtype=th.float32).view(-1, 1) / B
        loss = (res["pred_c"] * c).sum()
        for k in ("pred_v", "pred_e"):
            if res[k] is not None:
                cv = th.from_numpy(rng.standard_normal(tuple(res[k].shape)).astype(np.float32))
                arrs["coef/%s" % k] = cv.numpy()
                loss = loss + (res[k] * cv).sum()
        loss.backward()
        none_out = []
        for k in KEYS:
            if res[k] is None:
                none_out.append(k)
            else:
                a = res[k].detach().numpy()
                assert a.dtype == bool or np.isfinite(a).all(), (name, k)
                arrs["out/%s" % k] = a
        none_rep = []
        for k in REPS:
            if res[k].grad is None:
                none_rep.append(k)
            else:
                arrs["grad_rep/%s" % k] = res[k].grad.numpy()
        none_grad = []
        for k, p in model.named_parameters():
            if p.grad is None:
                none_grad.append(k)
            else:
                arrs["grad/%s" % k] = p.grad.numpy()
        buffers = [k for k, _ in model.named_buffers()]
        for k in buffers:
            if k not in alias:
                arrs["after/%s" % k] = model.state_dict()[k].numpy().copy()
        m = dict(tag=tag, name=name, kind="model", cfg=cfg, bopt=bopt, seed=seed, B=B, alias=alias, init_sha=init_sha, shapes=shapes,
                 keys=list(model.state_dict().keys()), params=[k for k, _ in model.named_parameters()], none_out=none_out,
                 none_grad=none_grad, none_rep=none_rep, buffers=buffers)
        m["index"] = D._pack(out, tag, arrs)
        meta.append(m)
        print("%s: %d + %d sequences" % (name, arrs["p/lrp_split"].sum(), arrs["g/lrp_split"].sum()))
    for lid, (name, kw, bopt) in enumerate(LAYER_CASES):
        L = kw["lrp_seq_len"]
        rng = np.random.default_rng(3700 + lid)
        _, gb = G._batches(rng, BASE_CFG, bopt, 3)
        seed = 8900 + lid
        th.manual_seed(seed)
        layer = DMPLRPPoolLayer(H, H, **kw)
        tag = "l%02d" % lid
        arrs = {}
        keys = list(layer.state_dict().keys())
        init_sha = {k: _sha(t) for k, t in layer.state_dict().items()}
        with th.no_grad():
            for p in layer.parameters():
                p.add_(0.05 * th.randn_like(p))
        for k, t in layer.state_dict().items():
            arrs["param/%s" % k] = t.numpy().copy()
        for k, a in gb.items():
            arrs["g/%s" % k] = a
        mats, lists = G._lrp_inputs(LRPDataset, gb, L)
        arrs["g/lrp_split"] = lists["lrp_split"]
        g = G._fake(gb)
        x = th.from_numpy(rng.standard_normal((g.number_of_nodes(), H)).astype(np.float32)).requires_grad_(True)
        ef = th.from_numpy(rng.standard_normal((g.number_of_edges(), H)).astype(np.float32)).requires_grad_(True)
        coef = th.from_numpy(rng.standard_normal((g.number_of_nodes(), H)).astype(np.float32))
        coef_e = th.from_numpy(rng.standard_normal((g.number_of_edges(), H)).astype(np.float32))
        layer.train()
        node_out, edge_out = layer(g, x, ef, *mats)[:2]
        ((node_out * coef).sum() + (edge_out * coef_e).sum()).backward()
        arrs.update({"in/x": x.detach().numpy(), "in/ef": ef.detach().numpy(), "in/coef": coef.numpy(), "in/coef_e": coef_e.numpy(),
                     "out/node_out": node_out.detach().numpy(), "out/edge_out": edge_out.detach().numpy(),
                     "grad_in/x": x.grad.numpy(), "grad_in/ef": ef.grad.numpy()})
        none_grad = []
        for k, p in layer.named_parameters():
            if p.grad is None:                                        # out_weight on a batch without reversed edges
                none_grad.append(k)
            else:
                arrs["grad/%s" % k] = p.grad.numpy()
        buffers = [k for k, _ in layer.named_buffers()]
        for k in buffers:
            arrs["after/%s" % k] = layer.state_dict()[k].numpy().copy()
        m = dict(tag=tag, name=name, kind="layer", kw=kw, bopt=bopt, seed=seed, keys=keys, alias={}, init_sha=init_sha,
                 params=[k for k, _ in layer.named_parameters()], none_grad=none_grad, buffers=buffers)
        m["index"] = D._pack(out, tag, arrs)
        meta.append(m)
        print("%s: %d sequences" % (name, arrs["g/lrp_split"].sum()))
    out["meta"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    path = os.path.join(HERE, "si_dmplrp.npz")
    np.savez_compressed(path, **out)
    print("si_dmplrp.npz: %d cases, %d bytes" % (len(meta), os.path.getsize(path)))


if __name__ == "__main__":
    make()
