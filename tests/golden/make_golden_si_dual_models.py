"""Golden vectors of the SI count models CompGCN(**cfg) / DMPNN(**cfg) (subgraph_isomorphism/models/basemodel.py:985-1703,
compgcn.py:289-385, dmpnn.py:178-277), run on the CPU from the reference's own code with the stand-ins of _ref_standins.py.

Run on the authoring box only (needs the reference checkout), like make_golden_si_models.py:
    python tests/golden/make_golden_si_dual_models.py
Writes si_dual_models.npz (CompGCN cases) and si_dual_models_dmpnn.npz (data only): per case the config, the two batches (node
and edge is_dummy, is_reversed, the per-graph edge counts), a sha256 of every initial state_dict tensor (and the tensors themselves for INIT_VALUE_CASES), the perturbed parameters (pred_fc2 is zero-initialised, so without a perturbation every upstream
gradient is 0), every OutputDict tensor, the gradient of every parameter (None recorded as such) and of the four rep tensors under
loss = sum(pred_c * c) (+ sum(pred_v * c_v) + sum(pred_e * c_e)), the buffers after the step (BatchNorm statistics), and for one
case the state_dict after expand()."""
import hashlib
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
REPS = ("p_v_rep", "p_e_rep", "g_v_rep", "g_e_rep")

BASE_CFG = dict(max_ngv=16, max_ngvl=8, max_nge=64, max_ngel=4, max_npv=16, max_npvl=8, max_npe=64, max_npel=4,
                base=2, enc_net="Multihot", emb_net="Orthogonal", filter_net="ScalarFilter", rep_net="CompGCN",
                rep_num_graph_layers=2, rep_num_pattern_layers=2, rep_compgcn_comp_opt="mult", rep_compgcn_edge_norm="none",
                rep_compgcn_batch_norm=False, rep_dmpnn_num_mlp_layers=2, rep_dmpnn_batch_norm=False,
                rep_act_func="leaky_relu", rep_residual=True, share_enc_net=True, share_emb_net=True, share_rep_net=True,
                pred_net="SumPredictNet", pred_with_enc=True, pred_with_deg=True, pred_hid_dim=8, pred_act_func="relu",
                hid_dim=16, pred_dropout=0.0, rep_dropout=0.0, pred_return_weights="none", init_neigenv=4.0, init_eeigenv=4.0,
                node_pred=True, edge_pred=True, add_node_id=False, add_edge_id=False)

_D = {"rep_net": "DMPNN"}
_NO_SHARE = {"share_enc_net": False, "share_emb_net": False, "share_rep_net": False}
CASES = [
    ("compgcn_mult", {}, {}),
    ("compgcn_sub", {"rep_compgcn_comp_opt": "sub"}, {}),
    ("compgcn_corr", {"rep_compgcn_comp_opt": "corr"}, {}),
    ("compgcn_norm_in", {"rep_compgcn_edge_norm": "in"}, {}),
    ("compgcn_norm_out", {"rep_compgcn_edge_norm": "out", "rep_compgcn_comp_opt": "sub"}, {}),
    ("compgcn_norm_both", {"rep_compgcn_edge_norm": "both"}, {}),
    ("compgcn_bn", {"rep_compgcn_batch_norm": True}, {}),
    ("compgcn_3_layers", {"rep_num_graph_layers": 3, "rep_num_pattern_layers": 3, "rep_compgcn_comp_opt": "sub"}, {}),
    ("compgcn_no_residual", {"rep_residual": False}, {}),
    ("compgcn_no_reversed", {}, {"reversed": False}),
    ("compgcn_no_dummy", {"rep_compgcn_comp_opt": "sub"}, {"dummy": False}),
    ("compgcn_add_edge_id", {"add_edge_id": True}, {}),
    ("compgcn_no_filter", {"filter_net": "None"}, {}),
    ("compgcn_mean_head", {"pred_net": "MeanPredictNet"}, {}),
    ("compgcn_max_head", {"pred_net": "MaxPredictNet"}, {}),
    ("compgcn_node_only", {"edge_pred": False}, {}),
    ("compgcn_edge_only", {"node_pred": False}, {}),
    ("compgcn_no_share", dict(_NO_SHARE, emb_net="Equivariant"), {}),
    ("compgcn_position", {"enc_net": "Position", "pred_with_deg": False}, {}),
    ("compgcn_weights", {"pred_return_weights": "node_edge"}, {}),
    ("dmpnn", dict(_D), {}),
    ("dmpnn_1_mlp", dict(_D, rep_dmpnn_num_mlp_layers=1), {}),
    ("dmpnn_bn", dict(_D, rep_dmpnn_batch_norm=True), {}),
    ("dmpnn_tanh", dict(_D, rep_act_func="tanh"), {}),
    ("dmpnn_3_layers", dict(_D, rep_num_graph_layers=3, rep_num_pattern_layers=3), {}),
    ("dmpnn_no_reversed", dict(_D), {"reversed": False}),
    ("dmpnn_no_dummy", dict(_D), {"dummy": False}),
    ("dmpnn_add_ids", dict(_D, add_node_id=True, add_edge_id=True), {}),
    ("dmpnn_equal_graphs", dict(_D), {"equal_graphs": True}),
    ("dmpnn_expand", dict(_D, **_NO_SHARE), {"expand": True}),
]
INIT_VALUE_CASES = ("compgcn_mult", "compgcn_no_share", "compgcn_position", "dmpnn", "dmpnn_bn", "dmpnn_expand")
EXPAND_KW = dict(max_ngv=40, max_ngvl=20, max_ngel=9, max_npv=12, max_npvl=20, max_npel=3)


def _si_modules():
    SI = os.path.join(REF, "subgraph_isomorphism")
    sys.path.insert(0, SI)
    if "models" not in sys.modules:
        pkg = types.ModuleType("models")
        pkg.__path__ = [os.path.join(SI, "models")]  # skip models/__init__ (pulls every rep net)
        sys.modules["models"] = pkg
    return {"CompGCN": importlib.import_module("models.compgcn").CompGCN, "DMPNN": importlib.import_module("models.dmpnn").DMPNN}


class BatchedFakeGraph(S.FakeDGLGraph):
    """FakeDGLGraph + the batch queries of a dgl batch that GraphAdjModelV2.forward makes."""

    def __init__(self, u, v, sizes, esizes):
        super().__init__(u, v, int(sum(sizes)))
        self._bnn = th.as_tensor(sizes, dtype=th.long)
        self._bne = th.as_tensor(esizes, dtype=th.long)

    @property
    def batch_size(self):
        return int(self._bnn.numel())

    def batch_num_nodes(self):
        return self._bnn

    def batch_num_edges(self):
        return self._bne


def _batch(rng, B, lo, hi, nv, nvl, nel, dummy, reverse, equal):
    """B graphs of lo..hi real nodes (+ one dummy node, label 0, last).  Edges of a graph in order: the real edges (labels below
    nel / 2), their reversed copies (label + nel / 2, is_reversed), the dummy edges dummy -> node and node -> dummy (the second set
    is_reversed).  Without `reverse` the same edges carry no is_reversed key at all."""
    sizes, esizes, u, v, ids, labels, elab, flags, eflags, rflags = [], [], [], [], [], [], [], [], [], []
    off = 0
    n_equal, e_equal = int(rng.integers(lo, hi + 1)), None
    half = max(nel // 2, 1)
    for _ in range(B):
        n = n_equal if equal else int(rng.integers(lo, hi + 1))
        m = n + (1 if dummy else 0)
        assert m <= nv
        E = int(rng.integers(n, n + 2))
        if equal:
            E = e_equal = E if e_equal is None else e_equal
        a, b = rng.integers(0, n, size=E), rng.integers(0, n, size=E)
        el = rng.integers(0, half, size=E)
        src, dst, lab = np.concatenate([a, b]), np.concatenate([b, a]), np.concatenate([el, el + half])
        rv = np.concatenate([np.zeros(E, bool), np.ones(E, bool)])
        dm = np.zeros(2 * E, bool)
        if dummy:
            src = np.concatenate([src, np.full(n, n), np.arange(n)])
            dst = np.concatenate([dst, np.arange(n), np.full(n, n)])
            dl = rng.integers(0, half, size=n)
            lab = np.concatenate([lab, dl, dl + half])
            rv = np.concatenate([rv, np.zeros(n, bool), np.ones(n, bool)])
            dm = np.concatenate([dm, np.ones(2 * n, bool)])
        u += list(src + off)
        v += list(dst + off)
        elab += list(lab)
        eflags += list(dm)
        rflags += list(rv)
        ids += list(range(m))
        labels += list(rng.integers(1, nvl, size=n)) + ([0] if dummy else [])
        flags += [False] * n + ([True] if dummy else [])
        sizes.append(m)
        esizes.append(len(src))
        off += m
    d = dict(sizes=np.array(sizes, np.int64), esizes=np.array(esizes, np.int64), u=np.array(u, np.int64), v=np.array(v, np.int64),
             id=np.array(ids, np.int64), label=np.array(labels, np.int64), elabel=np.array(elab, np.int64))
    if dummy:
        d["dummy"] = np.array(flags, bool)
        d["edummy"] = np.array(eflags, bool)
    if reverse:
        d["rev"] = np.array(rflags, bool)
    return d


def _fake(d):
    g = BatchedFakeGraph(d["u"], d["v"], d["sizes"], d["esizes"])
    g.ndata["id"] = th.from_numpy(d["id"])
    g.ndata["label"] = th.from_numpy(d["label"])
    g.edata["label"] = th.from_numpy(d["elabel"])
    if "dummy" in d:
        g.ndata["is_dummy"] = th.from_numpy(d["dummy"])
        g.edata["is_dummy"] = th.from_numpy(d["edummy"])
    if "rev" in d:
        g.edata["is_reversed"] = th.from_numpy(d["rev"])
    return g


def _pack(out, tag, arrs):
    """One array per case and element type (a few large zip members instead of many small ones); the index goes to the meta."""
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
        rng = np.random.default_rng(1700 + cid)
        B = 6
        dummy, reverse, equal = bopt.get("dummy", True), bopt.get("reversed", True), bopt.get("equal_graphs", False)
        pb = _batch(rng, B, 2, 3, cfg["max_npv"], cfg["max_npvl"], cfg["max_npel"], dummy, reverse, False)
        gb = _batch(rng, B, 3, 5, cfg["max_ngv"], cfg["max_ngvl"], cfg["max_ngel"], dummy, reverse, equal)
        seed = 9500 + cid
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
        init_sha = {k: hashlib.sha256(t.numpy().tobytes()).hexdigest()[:24] for k, t in model.state_dict().items()}
        if name in INIT_VALUE_CASES:                               # (the values themselves where the file size allows: a digest
            for k, t in model.state_dict().items():                #  that differs says neither where nor by how much)
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
        for side, d in (("p", pb), ("g", gb)):
            for k, a in d.items():
                arrs["%s/%s" % (side, k)] = a
        m = dict(tag=tag, name=name, cfg=cfg, seed=seed, B=B, alias=alias, init_sha=init_sha, shapes=shapes, keys=list(model.state_dict().keys()),
                 params=[k for k, _ in model.named_parameters()])
        if bopt.get("expand"):
            kw = dict(cfg)
            kw.update(EXPAND_KW)
            th.manual_seed(seed + 1)
            model.expand(**kw)
            for k, t in model.state_dict().items():
                arrs["expand/%s" % k] = t.numpy().copy()
            m.update(expand_kw=EXPAND_KW, expand_seed=seed + 1, forward=False)
            m["index"] = _pack(out, tag, arrs)
            meta.append(m)
            continue
        model.train()
        res = model(_fake(pb), _fake(gb))
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
        m.update(none_out=none_out, none_grad=none_grad, none_rep=none_rep, buffers=buffers, forward=True)
        m["index"] = _pack(out, tag, arrs)
        meta.append(m)
    # two files (a committed file stays under 1 MiB): the CompGCN cases and the DMPNN cases
    for fname, rep in (("si_dual_models.npz", "CompGCN"), ("si_dual_models_dmpnn.npz", "DMPNN")):
        part = [m for m in meta if m["cfg"]["rep_net"] == rep]
        tags = set(m["tag"] for m in part)
        sub = {k: v for k, v in out.items() if k.split("/")[0] in tags}
        sub["meta"] = np.frombuffer(json.dumps(part).encode(), dtype=np.uint8)
        path = os.path.join(HERE, fname)
        np.savez_compressed(path, **sub)
        print("%s: %d cases, %d bytes" % (fname, len(part), os.path.getsize(path)))


if __name__ == "__main__":
    make()
