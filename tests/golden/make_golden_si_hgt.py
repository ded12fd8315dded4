"""Golden vectors of the SI count model HGT(**cfg) and of HeteroGraphTransLayer (subgraph_isomorphism/models/hgt.py), run on the CPU
from the reference's own code with the stand-ins of _ref_standins.py.

Run on the authoring box only (needs the reference checkout), like make_golden_si_models.py:
    python tests/golden/make_golden_si_hgt.py
Writes si_hgt.npz (data only).  Two additions to the stand-ins, made here (the reference's HGT needs nothing else):

* the fake batched graph gets `canonical_etypes = [("_N", "_E", "_N")]` (one edge type object: the reference then reads the edge
  type of every edge from edata);
* `dgl.ops.edge_softmax(graph, e)`: the softmax of e over the in-edges of every destination, per trailing dimension.  This RESTATES
  DGL's documented behaviour; like the PyG stand-ins it is unpinned third-party arithmetic, not reference source.

Per model case: the config, the two batches (as make_golden_si_models.py stores them), a sha256 of every initial state_dict tensor
(the tensors themselves for INIT_VALUE_CASES), the perturbed parameters, every OutputDict tensor, the gradient of every parameter
(None recorded as such) and of p_v_rep / g_v_rep under loss = sum(pred_c * c) (+ sum(pred_v * c_v)), the buffers after the step.
Per layer case: the graph, the inputs, the coefficients of the loss, the output and the gradients of the input and the parameters."""
import hashlib
import importlib
import json
import os
import sys
import types

import numpy as np
import torch as th

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_si_models as M  # noqa: E402  (installs the stand-ins; BASE_CFG, the batches, the fake batched graph, the packing)

KEYS = M.KEYS

BASE_CFG = dict(M.BASE_CFG, rep_net="HGT", rep_num_graph_layers=2, rep_num_pattern_layers=2, rep_act_func="relu", max_ngvl=5, max_npvl=5)
for _k in [k for k in BASE_CFG if k.startswith(("rep_rgin", "rep_rgcn"))]:
    del BASE_CFG[_k]


def _reg(name, bases, heads=4):
    return {"rep_hgt_regularizer": name, "rep_hgt_num_bases": bases, "rep_hgt_num_heads": heads}


_NO_SHARE = {"share_enc_net": False, "share_emb_net": False, "share_rep_net": False}
# (name, config overrides, batch options)
CASES = [
    ("default", {}, {}),                                             # rep_hgt_* absent: "diag" with num_bases -1 -> dense weights
    ("none_b2", dict(_reg("none", 2), rep_num_graph_layers=1, rep_num_pattern_layers=1), {}),
    ("basis_b2", _reg("basis", 2), {}),
    ("bdd_b4_h2", _reg("bdd", 4, 2), {}),
    ("diag_b3", _reg("diag", 3), {}),
    ("scalar_b2", _reg("scalar", 2), {}),
    ("heads1", _reg("basis", 3, 1), {}),
    ("heads2", _reg("bdd", 2, 2), {}),
    ("batch_norm", dict(_reg("basis", 2), rep_hgt_batch_norm=True), {}),
    ("no_share", dict(_reg("diag", 2), **_NO_SHARE), {}),
    ("no_filter", dict(_reg("bdd", 4), filter_net="None"), {}),
    ("no_dummy", _reg("diag", 2), {"dummy": False}),
    ("leaky_relu", dict(_reg("basis", 2, 2), rep_act_func="leaky_relu"), {}),
    ("layers1", {"rep_num_graph_layers": 1, "rep_num_pattern_layers": 1}, {}),
    ("layers3", dict(_reg("bdd", 4), rep_num_graph_layers=3, rep_num_pattern_layers=3), {}),
]
INIT_VALUE_CASES = ("default",)
# (name, HeteroGraphTransLayer keyword arguments)
H, T, R = 16, 5, 3
LAYER_CASES = [
    ("layer_none_h4", dict(regularizer="none", num_bases=-1, num_heads=4, act_func="relu")),
    ("layer_bdd_h2_leaky", dict(regularizer="bdd", num_bases=4, num_heads=2, act_func="leaky_relu")),
    ("layer_basis_h1_bn", dict(regularizer="basis", num_bases=2, num_heads=1, batch_norm=True, act_func="relu")),
    ("layer_diag_h4", dict(regularizer="diag", num_bases=3, num_heads=4, act_func="leaky_relu")),
    ("layer_scalar_h2_plain", dict(regularizer="scalar", num_bases=2, num_heads=2, self_loop=False, bias=False, act_func="none")),
]


def edge_softmax(graph, e):
    """dgl.ops.edge_softmax(graph, logits), norm_by="dst": softmax over the edges that share a destination, per trailing dimension."""
    n = graph.number_of_nodes()
    idx = graph._v.view(-1, *([1] * (e.dim() - 1))).expand_as(e)
    mx = th.full((n,) + tuple(e.shape[1:]), float("-inf"), dtype=e.dtype).scatter_reduce(0, idx, e.detach(), "amax", include_self=True)
    p = th.exp(e - mx[graph._v])
    sm = th.zeros((n,) + tuple(e.shape[1:]), dtype=e.dtype).index_add(0, graph._v, p)
    return p / sm[graph._v]


def install():
    dgl = sys.modules["dgl"]
    if not hasattr(dgl, "ops"):
        ops = types.ModuleType("dgl.ops")
        ops.edge_softmax = edge_softmax
        dgl.ops = ops
        sys.modules["dgl.ops"] = ops
    M.S.FakeDGLGraph.canonical_etypes = [("_N", "_E", "_N")]


def _modules():
    install()
    M._si_modules()                                                  # sys.path + the bare `models` package
    hgt = importlib.import_module("models.hgt")
    return hgt.HGT, hgt.HeteroGraphTransLayer


def _sha(t):
    return hashlib.sha256(t.detach().contiguous().numpy().tobytes()).hexdigest()[:24]


def _layer_graph(rng):
    """Two graphs in one batch.  Graph 0 (nodes 0..8): node 0 has no in-edge, 1 -> 2 of type 0 twice (a multi-edge), 3 -> 3 (a
    self-loop edge), node 4 has the single in-edge 0 -> 4, node 5 collects an edge from every other node (a small hub), random
    edges among 1..8 that avoid the destinations 0 and 4.  Graph 1 (nodes 9..13): a ring with random chords."""
    u = [1, 1, 3, 0] + [x for x in range(9) if x != 5]
    v = [2, 2, 3, 4] + [5] * 8
    et = [0, 0, 1, 2] + list(rng.integers(0, R, size=8))
    for _ in range(14):
        a, b = int(rng.integers(0, 9)), int(rng.choice([1, 2, 3, 5, 6, 7, 8]))
        u.append(a)
        v.append(b)
        et.append(int(rng.integers(0, R)))
    for i in range(5):
        u += [9 + i, 9 + int(rng.integers(0, 5))]
        v += [9 + (i + 1) % 5, 9 + int(rng.integers(0, 5))]
        et += [int(rng.integers(0, R)), int(rng.integers(0, R))]
    return dict(sizes=np.array([9, 5], np.int64), u=np.array(u, np.int64), v=np.array(v, np.int64),
                id=np.array(list(range(9)) + list(range(5)), np.int64), label=rng.integers(0, T, size=14).astype(np.int64),
                elabel=np.array(et, np.int64))


def make():
    HGT, Layer = _modules()
    out, meta = {}, []
    for cid, (name, over, bopt) in enumerate(CASES):
        cfg = dict(BASE_CFG)
        cfg.update(over)
        rng = np.random.default_rng(3100 + cid)
        B = 6
        dummy = bopt.get("dummy", True)
        pb = M._batch(rng, B, 2, 5, cfg["max_npv"], cfg["max_npvl"], cfg["max_npel"], dummy, False)
        gb = M._batch(rng, B, 3, 9, cfg["max_ngv"], cfg["max_ngvl"], cfg["max_ngel"], dummy, False)
        seed = 9300 + cid
        th.manual_seed(seed)
        model = HGT(**cfg)
        tag = "m%02d" % cid
        arrs = {}
        alias, first = {}, {}
        for k, t in model.state_dict(keep_vars=True).items():        # shared modules: their p_* keys are the g_* tensors
            if id(t) in first:
                alias[k] = first[id(t)]
            else:
                first[id(t)] = k
        init_sha = {k: _sha(t) for k, t in model.state_dict().items()}
        shapes = {k: list(t.shape) for k, t in model.state_dict().items()}
        if name in INIT_VALUE_CASES:
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
        res = model(M._fake(pb), M._fake(gb))
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
                a = res[k].detach().numpy()
                assert a.dtype == bool or np.isfinite(a).all(), (name, k)
                arrs["out/%s" % k] = a
        arrs["grad_rep/p"] = res["p_v_rep"].grad.numpy()
        arrs["grad_rep/g"] = res["g_v_rep"].grad.numpy()
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
        m = dict(tag=tag, name=name, kind="model", cfg=cfg, seed=seed, B=B, none_out=none_out, none_grad=none_grad, alias=alias,
                 init_sha=init_sha, shapes=shapes, keys=list(model.state_dict().keys()),
                 params=[k for k, _ in model.named_parameters()], buffers=buffers)
        m["index"] = M._pack(out, tag, arrs)
        meta.append(m)
        print("%s: pred_c %s" % (name, np.round(arrs["out/pred_c"].reshape(-1)[:3], 4)))
    for lid, (name, kw) in enumerate(LAYER_CASES):
        rng = np.random.default_rng(3200 + lid)
        gb = _layer_graph(rng)
        seed = 9400 + lid
        th.manual_seed(seed)
        layer = Layer(H, H, num_node_types=T, num_edge_types=R, **kw)
        tag = "l%02d" % lid
        arrs = {}
        keys = list(layer.state_dict().keys())
        init_sha = {k: _sha(t) for k, t in layer.state_dict().items()}
        with th.no_grad():
            for p in layer.parameters():
                p.add_(0.1 * th.randn_like(p))
        for k, t in layer.state_dict().items():
            arrs["param/%s" % k] = t.numpy().copy()
        for k, a in gb.items():
            arrs["g/%s" % k] = a
        g = M._fake(gb)
        n = g.number_of_nodes()
        x = th.from_numpy(rng.standard_normal((n, H)).astype(np.float32)).requires_grad_(True)
        coef = th.from_numpy(rng.standard_normal((n, H)).astype(np.float32))
        layer.train()
        y = layer(g, x)
        (y * coef).sum().backward()
        arrs.update({"in/x": x.detach().numpy(), "in/coef": coef.numpy(), "out/node_out": y.detach().numpy(), "grad_in/x": x.grad.numpy()})
        none_grad = []
        for k, p in layer.named_parameters():
            if p.grad is None:
                none_grad.append(k)
            else:
                arrs["grad/%s" % k] = p.grad.numpy()
        buffers = [k for k, _ in layer.named_buffers()]
        for k in buffers:
            arrs["after/%s" % k] = layer.state_dict()[k].numpy().copy()
        m = dict(tag=tag, name=name, kind="layer", kw=kw, dims=dict(H=H, T=T, R=R), seed=seed, keys=keys, alias={}, init_sha=init_sha,
                 params=[k for k, _ in layer.named_parameters()], none_grad=none_grad, buffers=buffers)
        m["index"] = M._pack(out, tag, arrs)
        meta.append(m)
        print("%s: |out| max %.4f" % (name, float(np.abs(arrs["out/node_out"]).max())))
    out["meta"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    path = os.path.join(HERE, "si_hgt.npz")
    np.savez_compressed(path, **out)
    print("si_hgt.npz: %d cases, %d bytes" % (len(meta), os.path.getsize(path)))


if __name__ == "__main__":
    make()
