"""Golden vectors of the SI count models RGIN(**cfg) / RGCN(**cfg) (subgraph_isomorphism/models/basemodel.py:629-982,
rgin.py:175-260, rgcn.py:215-300), run on the CPU from the reference's own code with the stand-ins of _ref_standins.py.

Run on the authoring box only (needs the reference checkout), like make_golden.py:  python tests/golden/make_golden_si_models.py
Writes si_models.npz (data only): per case the config, the two batches, the init state_dict, the perturbed parameters (pred_fc2
is zero-initialised, so without a perturbation every upstream gradient is 0), every OutputDict tensor, the gradient of every
parameter (None recorded as such) and of p_v_rep / g_v_rep under loss = sum(pred_c * c) (+ sum(pred_v * c_v)), and for one case
the state_dict after expand()."""
import importlib
import json
import os
import sys
import types

import numpy as np
import torch as th

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
sys.path.insert(0, HERE)
import _ref_standins as S  # noqa: E402

S.install()

KEYS = ("p_v_emb", "p_e_emb", "g_v_emb", "g_e_emb", "p_v_rep", "p_e_rep", "g_v_rep", "g_e_rep", "p_v_mask", "p_e_mask",
        "g_v_mask", "g_e_mask", "pred_c", "pred_v", "pred_e")

BASE_CFG = dict(max_ngv=16, max_ngvl=8, max_nge=64, max_ngel=4, max_npv=16, max_npvl=8, max_npe=64, max_npel=4,
                base=2, enc_net="Multihot", emb_net="Equivariant", filter_net="ScalarFilter", rep_net="RGIN",
                rep_num_graph_layers=2, rep_num_pattern_layers=2, rep_rgin_regularizer="bdd", rep_rgin_num_bases=4,
                rep_rgcn_regularizer="bdd", rep_rgcn_num_bases=4, rep_act_func="leaky_relu", rep_residual=True,
                share_enc_net=True, share_emb_net=True, share_rep_net=True, pred_net="SumPredictNet", pred_with_enc=True,
                pred_with_deg=True, pred_hid_dim=8, pred_act_func="relu", hid_dim=16, pred_dropout=0.0, rep_dropout=0.0,
                pred_return_weights="none", init_neigenv=0.0, init_eeigenv=0.0)

CASES = [
    ("defaults", {"rep_num_graph_layers": 3, "rep_num_pattern_layers": 3}, {}),
    ("no_filter", {"filter_net": "None"}, {}),
    ("add_node_id", {"add_node_id": True}, {}),
    ("no_enc_no_deg", {"pred_with_enc": False, "pred_with_deg": False}, {}),
    ("mean_head", {"pred_net": "MeanPredictNet"}, {}),
    ("max_head", {"pred_net": "MaxPredictNet"}, {}),
    ("max_head_plain", {"pred_net": "MaxPredictNet", "pred_with_enc": False, "pred_with_deg": False}, {}),
    ("no_share", {"share_enc_net": False, "share_emb_net": False, "share_rep_net": False, "rep_num_pattern_layers": 2}, {}),
    ("position", {"enc_net": "Position"}, {}),
    ("orthogonal", {"emb_net": "Orthogonal", "add_node_id": True}, {}),
    ("no_residual", {"rep_residual": False}, {}),
    ("node_weights", {"pred_return_weights": "node"}, {}),
    ("no_dummy", {}, {"dummy": False}),
    ("equal_graphs", {}, {"equal_graphs": True}),
    ("equal_patterns", {}, {"equal_patterns": True}),
    ("rgcn_in", {"rep_net": "RGCN", "rep_rgcn_edge_norm": "in"}, {}),
    ("rgcn_both", {"rep_net": "RGCN", "rep_rgcn_edge_norm": "both", "rep_act_func": "relu"}, {}),
]
EXPAND_CASE = "no_share"
EXPAND_KW = dict(max_ngv=40, max_ngvl=20, max_npv=12, max_npvl=20)


def _si_modules():
    SI = os.path.join(REF, "subgraph_isomorphism")
    sys.path.insert(0, SI)
    if "models" not in sys.modules:
        pkg = types.ModuleType("models")
        pkg.__path__ = [os.path.join(SI, "models")]  # skip models/__init__ (pulls every rep net)
        sys.modules["models"] = pkg
    return {"RGIN": importlib.import_module("models.rgin").RGIN, "RGCN": importlib.import_module("models.rgcn").RGCN}


class BatchedFakeGraph(S.FakeDGLGraph):
    """FakeDGLGraph + the two batch queries of a dgl batch that GraphAdjModel.forward makes."""

    def __init__(self, u, v, sizes):
        super().__init__(u, v, int(sum(sizes)))
        self._bnn = th.as_tensor(sizes, dtype=th.long)

    @property
    def batch_size(self):
        return int(self._bnn.numel())

    def batch_num_nodes(self):
        return self._bnn


def _batch(rng, B, lo, hi, nv, nvl, nel, dummy, equal):
    """B graphs of lo..hi real nodes (+ one dummy node, label 0, last), ids = local positions, random edges inside each graph."""
    sizes, u, v, ids, labels, elab, flags = [], [], [], [], [], [], []
    off = 0
    n_equal = int(rng.integers(lo, hi + 1))
    for _ in range(B):
        n = n_equal if equal else int(rng.integers(lo, hi + 1))
        m = n + (1 if dummy else 0)
        assert m <= nv
        E = int(rng.integers(n, 2 * n + 1))
        a, b = rng.integers(0, n, size=E), rng.integers(0, n, size=E)
        if dummy:                                   # the dummy node links to every real node, both ways
            a = np.concatenate([a, np.full(n, n), np.arange(n)])
            b = np.concatenate([b, np.arange(n), np.full(n, n)])
        u += list(a + off)
        v += list(b + off)
        elab += list(rng.integers(0, nel, size=len(a)))
        ids += list(range(m))
        lab = list(rng.integers(1, nvl, size=n))
        labels += lab + ([0] if dummy else [])
        flags += [False] * n + ([True] if dummy else [])
        sizes.append(m)
        off += m
    d = dict(sizes=np.array(sizes, np.int64), u=np.array(u, np.int64), v=np.array(v, np.int64), id=np.array(ids, np.int64),
             label=np.array(labels, np.int64), elabel=np.array(elab, np.int64))
    if dummy:
        d["dummy"] = np.array(flags, bool)
    return d


def _fake(d):
    g = BatchedFakeGraph(d["u"], d["v"], d["sizes"])
    g.ndata["id"] = th.from_numpy(d["id"])
    g.ndata["label"] = th.from_numpy(d["label"])
    if "dummy" in d:
        g.ndata["is_dummy"] = th.from_numpy(d["dummy"])
    g.edata["label"] = th.from_numpy(d["elabel"])
    return g


def _pack(out, tag, arrs):
    """One array per case and element type (a few large zip members instead of ~150 small ones); the index goes to the meta."""
    index, blobs = [], {"f32": [], "i64": [], "u8": []}
    for k, a in arrs.items():
        a = np.asarray(a)
        kind = "f32" if a.dtype.kind == "f" else ("u8" if a.dtype == bool else "i64")
        off = sum(b.size for b in blobs[kind])
        blobs[kind].append(a.reshape(-1).astype({"f32": np.float32, "i64": np.int64, "u8": np.uint8}[kind]))
        index.append([k, kind, off, list(a.shape)])
    for kind, parts in blobs.items():
        if parts:
            out["%s/%s" % (tag, kind)] = np.concatenate(parts)
    return index


def make():
    models = _si_modules()
    out, meta = {}, []
    for cid, (name, over, bopt) in enumerate(CASES):
        cfg = dict(BASE_CFG)
        cfg.update(over)
        rng = np.random.default_rng(700 + cid)
        B = 6
        dummy = bopt.get("dummy", True)
        pb = _batch(rng, B, 2, 5, cfg["max_npv"], cfg["max_npvl"], cfg["max_npel"], dummy, bopt.get("equal_patterns", False))
        gb = _batch(rng, B, 3, 9, cfg["max_ngv"], cfg["max_ngvl"], cfg["max_ngel"], dummy, bopt.get("equal_graphs", False))
        seed = 9000 + cid
        th.manual_seed(seed)
        model = models[cfg["rep_net"]](**cfg)
        tag = "m%02d" % cid
        arrs = {}
        alias, first = {}, {}
        for k, t in model.state_dict(keep_vars=True).items():      # shared modules: their p_* keys are the g_* tensors
            if id(t) in first:
                alias[k] = first[id(t)]
            else:
                first[id(t)] = k
        for k, t in model.state_dict().items():
            if k not in alias:
                arrs["init/%s" % k] = t.numpy().copy()
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
        res = model(_fake(pb), _fake(gb))
        assert list(res.keys()) == list(KEYS), list(res.keys())
        res["p_v_rep"].retain_grad()
        res["g_v_rep"].retain_grad()
        c = th.arange(1, B + 1, dtype=th.float32).view(-1, 1) / B
        loss = (res["pred_c"] * c).sum()
        if res["pred_v"] is not None:
            cv = th.from_numpy(rng.standard_normal(tuple(res["pred_v"].shape)).astype(np.float32))
            arrs["coef_v"] = cv.numpy()
            loss = loss + (res["pred_v"] * cv).sum()
        loss.backward()
        none_out = []
        for k in KEYS:
            if res[k] is None:
                none_out.append(k)
            else:
                arrs["out/%s" % k] = res[k].detach().numpy()
        arrs["grad_rep/p"] = res["p_v_rep"].grad.numpy()
        arrs["grad_rep/g"] = res["g_v_rep"].grad.numpy()
        none_grad = []
        for k, p in model.named_parameters():
            if p.grad is None:
                none_grad.append(k)
            else:
                arrs["grad/%s" % k] = p.grad.numpy()
        m = dict(tag=tag, name=name, cfg=cfg, seed=seed, B=B, none_out=none_out, none_grad=none_grad, alias=alias,
                 keys=list(model.state_dict().keys()),
                 params=[k for k, _ in model.named_parameters()])
        if name == EXPAND_CASE:
            kw = dict(cfg)
            kw.update(EXPAND_KW)
            th.manual_seed(seed + 1)
            model.expand(**kw)
            for k, t in model.state_dict().items():
                arrs["expand/%s" % k] = t.numpy().copy()
            m["expand_kw"] = EXPAND_KW
            m["expand_seed"] = seed + 1
        m["index"] = _pack(out, tag, arrs)
        meta.append(m)
    out["meta"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    path = os.path.join(HERE, "si_models.npz")
    np.savez_compressed(path, **out)
    print("si_models.npz: %d cases, %d bytes" % (len(meta), os.path.getsize(path)))


if __name__ == "__main__":
    make()
