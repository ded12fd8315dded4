"""Golden vectors of the SI count model LRP(**cfg) and of LRPLayer (subgraph_isomorphism/models/lrp.py), with the ego-net
permutation index of LRPDataset (subgraph_isomorphism/dataset.py:1750-1886), run on the CPU from the reference's own code with
the stand-ins of _ref_standins.py.

Run on the authoring box only (needs the reference checkout and scipy), like make_golden_si_dual_models.py:
    python tests/golden/make_golden_si_lrp.py
Writes si_lrp.npz (data only).  Per case: the config, the batches (as make_golden_si_dual_models.py stores them), per batch the
reference's two COO index lists (node_to_perm / edge_to_perm rows and columns, in the order LRPDataset emits them) and the
sequences per node; for the model cases a sha256 of every initial state_dict tensor (the tensors themselves for
INIT_VALUE_CASES), the perturbed parameters, every OutputDict tensor, the gradient of every parameter and of the four rep tensors
under loss = sum(pred_c * c) + sum(pred_v * c_v) + sum(pred_e * c_e), and the buffers after the step; for the layer cases the
inputs, the coefficients of the loss, the output and the gradients of the inputs and parameters."""
import hashlib
import importlib
import json
import os
import sys

import numpy as np
import torch as th

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_si_dual_models as D  # noqa: E402  (installs the stand-ins; BASE_CFG, the fake batched graph, the packing)

S = D.S
KEYS, REPS = D.KEYS, D.REPS

BASE_CFG = dict(D.BASE_CFG, rep_net="LRP", rep_num_graph_layers=1, rep_num_pattern_layers=1, lrp_seq_len=4,
                rep_lrp_batch_norm=False, rep_act_func="relu", max_nge=256, max_npe=256)
for _k in [k for k in BASE_CFG if k.startswith(("rep_compgcn", "rep_dmpnn", "init_"))]:
    del BASE_CFG[_k]

_NO_SHARE = {"share_enc_net": False, "share_emb_net": False, "share_rep_net": False}
_TWO = {"rep_num_graph_layers": 2, "rep_num_pattern_layers": 2}
# (name, config overrides, batch options)
CASES = [
    ("lrp_l4_relu", dict(_TWO), {}),
    ("lrp_l3_leaky", {"lrp_seq_len": 3, "rep_act_func": "leaky_relu"}, {}),
    ("lrp_bn", dict(_TWO, rep_lrp_batch_norm=True, rep_act_func="leaky_relu"), {"dummy_both": True}),
    ("lrp_no_share", dict(_NO_SHARE, emb_net="Equivariant", lrp_seq_len=3), {"dummy_both": True}),
    ("lrp_no_dummy", {"rep_act_func": "leaky_relu"}, {"dummy": False}),
    ("lrp_no_reversed", {}, {"reversed": False}),
    ("lrp_no_reversed_l3", {"lrp_seq_len": 3, "rep_act_func": "leaky_relu", "rep_lrp_batch_norm": True}, {"reversed": False}),
    ("lrp_no_filter_no_residual", {"filter_net": "None", "rep_residual": False, "lrp_seq_len": 3}, {"dummy_both": True}),
]
# (name, LRPLayer keyword arguments, batch options)
LAYER_CASES = [
    ("layer_l4_relu", dict(lrp_seq_len=4, act_func="relu"), {"reversed": False}),
    ("layer_l3_leaky_bn_mlp", dict(lrp_seq_len=3, act_func="leaky_relu", batch_norm=True, mlp=True), {"dummy_both": True}),
    ("layer_l2_no_bias", dict(lrp_seq_len=2, act_func="relu", bias=False), {"reversed": False}),
    ("layer_l4_leaky_plain", dict(lrp_seq_len=4, act_func="leaky_relu"), {"dummy": False, "reversed": False}),
]
INIT_VALUE_CASES = ("lrp_l4_relu",)
H = 16


def _modules():
    SI = os.path.join(D.REF, "subgraph_isomorphism")
    D._si_modules()                                                 # sys.path + the bare `models` package
    lrp = importlib.import_module("models.lrp")
    dataset = importlib.import_module("dataset")
    assert os.path.dirname(os.path.abspath(dataset.__file__)) == SI
    return lrp.LRP, lrp.LRPLayer, dataset.LRPDataset


def _batch(rng, B, lo, hi, nvl, nel, dummy, reverse, dummy_both):
    """B graphs of lo..hi real nodes (+ one dummy node, label 0, last), no self-loops.  Every real node draws an out-degree of
    0..5 and that many distinct targets; every third graph repeats two of its edges (parallel edges).  Edges of a graph in
    order: the real edges, their reversed copies (label + nel / 2, is_reversed), the dummy edges dummy -> node and node -> dummy
    (the second set is_reversed unless dummy_both).  Without `reverse` no edge carries an is_reversed key and there are no
    reversed copies of the real edges."""
    sizes, esizes, u, v, ids, labels, elab, flags, eflags, rflags = [], [], [], [], [], [], [], [], [], []
    off = 0
    half = max(nel // 2, 1)
    for gi in range(B):
        n = int(rng.integers(lo, hi + 1))
        m = n + (1 if dummy else 0)
        a, b = [], []
        for x in range(n):
            deg = min(int(rng.integers(0, 6)), n - 1)
            if gi == 0 and x == 0:
                deg = 0                                               # an isolated real node (no dummy edge reaches it either way
            others = [y for y in range(n) if y != x]                  #  when the batch has no dummy node)
            for y in rng.choice(others, size=deg, replace=False):
                a.append(x)
                b.append(int(y))
        if gi % 3 == 0 and len(a) >= 2:
            a += a[:2]
            b += b[:2]
        a, b = np.array(a, np.int64), np.array(b, np.int64)
        E = len(a)
        el = rng.integers(0, half, size=E)
        if reverse:
            src, dst, lab = np.concatenate([a, b]), np.concatenate([b, a]), np.concatenate([el, el + half])
            rv = np.concatenate([np.zeros(E, bool), np.ones(E, bool)])
        else:
            src, dst, lab, rv = a, b, el, np.zeros(E, bool)
        dm = np.zeros(len(src), bool)
        if dummy:
            src = np.concatenate([src, np.full(n, n), np.arange(n)])
            dst = np.concatenate([dst, np.arange(n), np.full(n, n)])
            dl = rng.integers(0, half, size=n)
            lab = np.concatenate([lab, dl, dl + half])
            rv = np.concatenate([rv, np.zeros(n, bool), np.zeros(n, bool) if (dummy_both or not reverse) else np.ones(n, bool)])
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


def _split(d):
    """The graphs of a batch dict as separate FakeDGLGraphs (graph-local ids), as the dataset holds them before dgl.batch."""
    graphs = []
    n0 = e0 = 0
    for n, ne in zip(d["sizes"], d["esizes"]):
        g = S.FakeDGLGraph(d["u"][e0:e0 + ne] - n0, d["v"][e0:e0 + ne] - n0, int(n))
        if "dummy" in d:
            g.ndata["is_dummy"] = th.from_numpy(d["dummy"][n0:n0 + n])
        if "rev" in d:
            g.edata["is_reversed"] = th.from_numpy(d["rev"][e0:e0 + ne])
        graphs.append(g)
        n0 += n
        e0 += ne
    return graphs


def _lrp_inputs(LRPDataset, d, L):
    """(pooling matrix, node_to_perm, edge_to_perm) of a batch by the reference's own functions, and the lists behind them."""
    LRPDataset.seq_len = L
    graphs = _split(d)
    ego = [LRPDataset.graph_to_egonet_seq(g) for g in graphs]
    split = np.asarray([len(node) for seq in ego for node in seq], dtype=np.int64)
    pool = LRPDataset.build_perm_pooling_matrix(split, "mean")
    n2p, e2p = LRPDataset.build_batch_graph_to_perm_matrices(graphs, ego)
    ni, ei = n2p._indices().numpy(), e2p._indices().numpy()
    lists = dict(lrp_node_row=ni[0], lrp_node_col=ni[1], lrp_edge_row=ei[0], lrp_edge_col=ei[1], lrp_split=split)
    return (pool, n2p, e2p), lists


def _fake(d):
    g = D._fake(d)
    g.ndata["in_deg"] = g.in_degrees()                                # train.py:491-495
    return g


def _batches(rng, cfg, bopt, B):
    dummy, reverse, both = bopt.get("dummy", True), bopt.get("reversed", True), bopt.get("dummy_both", False)
    pb = _batch(rng, B, 3, 4, cfg["max_npvl"], cfg["max_npel"], dummy, reverse, both)
    gb = _batch(rng, B, 3, 12, cfg["max_ngvl"], cfg["max_ngel"], dummy, reverse, both)
    return pb, gb


def make():
    LRP, LRPLayer, LRPDataset = _modules()
    out, meta = {}, []
    for cid, (name, over, bopt) in enumerate(CASES):
        cfg = dict(BASE_CFG)
        cfg.update(over)
        L = cfg["lrp_seq_len"]
        rng = np.random.default_rng(2600 + cid)
        B = 4 + cid % 3
        pb, gb = _batches(rng, cfg, bopt, B)
        seed = 9800 + cid
        th.manual_seed(seed)
        model = LRP(**cfg)
        tag = "m%02d" % cid
        arrs = {}
        alias, first = {}, {}
        for k, t in model.state_dict(keep_vars=True).items():
            if id(t) in first:
                alias[k] = first[id(t)]
            else:
                first[id(t)] = k
        init_sha = {k: hashlib.sha256(t.numpy().tobytes()).hexdigest()[:24] for k, t in model.state_dict().items()}
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
            mats[side], lists = _lrp_inputs(LRPDataset, d, L)
            for k, a in lists.items():
                arrs["%s/%s" % (side, k)] = a
        model.train()
        res = model(_fake(pb), *mats["p"], _fake(gb), *mats["g"])
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
        m = dict(tag=tag, name=name, kind="model", cfg=cfg, seed=seed, B=B, alias=alias, init_sha=init_sha, shapes=shapes,
                 keys=list(model.state_dict().keys()), params=[k for k, _ in model.named_parameters()], none_out=none_out,
                 none_grad=none_grad, none_rep=none_rep, buffers=buffers)
        m["index"] = D._pack(out, tag, arrs)
        meta.append(m)
        print("%s: %d + %d sequences" % (name, arrs["p/lrp_split"].sum(), arrs["g/lrp_split"].sum()))
    for lid, (name, kw, bopt) in enumerate(LAYER_CASES):
        L = kw["lrp_seq_len"]
        rng = np.random.default_rng(2700 + lid)
        _, gb = _batches(rng, BASE_CFG, bopt, 5)
        seed = 9900 + lid
        th.manual_seed(seed)
        layer = LRPLayer(H, H, **kw)
        tag = "l%02d" % lid
        arrs = {}
        keys = list(layer.state_dict().keys())
        init_sha = {k: hashlib.sha256(t.numpy().tobytes()).hexdigest()[:24] for k, t in layer.state_dict().items()}
        with th.no_grad():
            for p in layer.parameters():
                p.add_(0.05 * th.randn_like(p))
        for k, t in layer.state_dict().items():
            arrs["param/%s" % k] = t.numpy().copy()
        for k, a in gb.items():
            arrs["g/%s" % k] = a
        mats, lists = _lrp_inputs(LRPDataset, gb, L)
        for k, a in lists.items():
            arrs["g/%s" % k] = a
        g = _fake(gb)
        x = th.from_numpy(rng.standard_normal((g.number_of_nodes(), H)).astype(np.float32)).requires_grad_(True)
        ef = th.from_numpy(rng.standard_normal((g.number_of_edges(), H)).astype(np.float32)).requires_grad_(True)
        coef = th.from_numpy(rng.standard_normal((g.number_of_nodes(), H)).astype(np.float32))
        layer.train()
        node_out, edge_out = layer(g, x, ef, *mats)
        assert edge_out is ef
        (node_out * coef).sum().backward()
        arrs.update({"in/x": x.detach().numpy(), "in/ef": ef.detach().numpy(), "in/coef": coef.numpy(),
                     "out/node_out": node_out.detach().numpy(), "grad_in/x": x.grad.numpy(), "grad_in/ef": ef.grad.numpy()})
        for k, p in layer.named_parameters():
            arrs["grad/%s" % k] = p.grad.numpy()
        buffers = [k for k, _ in layer.named_buffers()]
        for k in buffers:
            arrs["after/%s" % k] = layer.state_dict()[k].numpy().copy()
        m = dict(tag=tag, name=name, kind="layer", kw=kw, seed=seed, keys=keys, alias={}, init_sha=init_sha,
                 params=[k for k, _ in layer.named_parameters()], buffers=buffers)
        m["index"] = D._pack(out, tag, arrs)
        meta.append(m)
        print("%s: %d sequences" % (name, arrs["g/lrp_split"].sum()))
    out["meta"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    path = os.path.join(HERE, "si_lrp.npz")
    np.savez_compressed(path, **out)
    print("si_lrp.npz: %d cases, %d bytes" % (len(meta), os.path.getsize(path)))


if __name__ == "__main__":
    make()
