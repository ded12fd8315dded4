"""Golden vectors of the SI count model CNN(**cfg) on edge sequences and of CNNLayer (subgraph_isomorphism/models/cnn.py,
basemodel.py EdgeSeqModel, dataset.py EdgeSeq), run on the CPU from the reference's own code with the stand-ins of _ref_standins.py.

Run on the authoring box only (needs the reference checkout), like make_golden_si_hgt.py:
    python tests/golden/make_golden_si_cnn.py
Writes si_cnn.npz (the first FIRST_FILE_CASES model cases) and si_cnn_layers.npz (the other model cases and the CNNLayer cases): data
only, two files because a committed file stays under 1 MiB.

Per model case: the config, both batches as graphs (sizes, edges, ids, labels -- what EdgeSeq.from_graph reads) and as the
reference's batched EdgeSeq (the five padded code tensors, the lengths, REVFLAG when carried, the padded degree tables), a sha256 of
every initial state_dict tensor (the tensors themselves for INIT_VALUE_CASES), the perturbed parameters, every OutputDict tensor, the
gradient of every parameter and of p_e_rep / g_e_rep under loss = sum(pred_c * c) (+ sum(pred_e * c_e)), the buffers after the step.
Per layer case: the input, the gate, the lengths, the loss coefficients, the gated (and residual) output in rows layout [B, L, C]
and the gradients of the input and the parameters.  The per-sequence tuples are sorted here by (u, v, ul, el, vl) with numpy's
lexsort, which is what the reference's from_graph does with a structured sort."""
import hashlib
import importlib
import json
import os
import sys

import numpy as np
import torch as th
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_si_models as M  # noqa: E402  (installs the stand-ins; BASE_CFG, the packing)

KEYS = M.KEYS
BASE_CFG = dict(M.BASE_CFG, rep_net="CNN", rep_num_graph_layers=2, rep_num_pattern_layers=2, rep_act_func="relu",
                rep_cnn_batch_norm=False, rep_cnn_kernel_sizes=2, rep_cnn_paddings=-1, rep_cnn_strides=1, emb_net="Equivariant")
for _k in [k for k in BASE_CFG if k.startswith(("rep_rgin", "rep_rgcn"))]:
    del BASE_CFG[_k]

_NO_SHARE = {"share_enc_net": False, "share_emb_net": False, "share_rep_net": False}


def _layers(n):
    return {"rep_num_graph_layers": n, "rep_num_pattern_layers": n}


# (name, config overrides, batch options)
CASES = [
    ("k2_default", {}, {}),
    ("k3_residual", {"rep_cnn_kernel_sizes": 3}, {}),
    ("k3_no_residual", {"rep_cnn_kernel_sizes": 3, "rep_residual": False}, {}),
    ("k4", {"rep_cnn_kernel_sizes": 4}, {}),
    ("k5", {"rep_cnn_kernel_sizes": 5, "rep_act_func": "leaky_relu"}, {}),
    ("k3_pad0", {"rep_cnn_kernel_sizes": 3, "rep_cnn_paddings": 0}, {}),
    ("k_list_2_3", {"rep_cnn_kernel_sizes": [2, 3]}, {}),
    ("layers1", _layers(1), {}),
    ("layers3", dict(_layers(3), rep_cnn_kernel_sizes=3), {}),
    ("batch_norm", {"rep_cnn_batch_norm": True, "rep_cnn_kernel_sizes": 3}, {}),
    ("leaky_relu", {"rep_act_func": "leaky_relu"}, {}),
    ("tanh", {"rep_act_func": "tanh", "rep_cnn_kernel_sizes": 3}, {}),
    ("no_share", dict(_NO_SHARE, rep_cnn_kernel_sizes=3), {}),
    ("position", {"enc_net": "Position"}, {}),
    ("orthogonal", {"emb_net": "Orthogonal"}, {}),
    ("no_enc_no_deg", {"pred_with_enc": False, "pred_with_deg": False}, {}),
    ("mean_head", {"pred_net": "MeanPredictNet", "rep_cnn_kernel_sizes": 3}, {}),
    ("max_head", {"pred_net": "MaxPredictNet"}, {}),
    ("edge_weights", {"pred_return_weights": "edge", "rep_cnn_kernel_sizes": 3}, {}),
    ("equal_lengths", {"rep_cnn_kernel_sizes": 3}, {"equal": True}),
    ("all_filtered", {"rep_cnn_kernel_sizes": 3}, {"all_filtered": True}),
    ("revflag", {}, {"rev": True}),
]
INIT_VALUE_CASES = ("k2_default",)
FIRST_FILE_CASES = 16                                                # the model cases si_cnn.npz holds; the rest go with the layer cases
C = 16
# (name, k, padding, act, residual, batch norm)
LAYER_CASES = [
    ("layer_k2_p1_relu", 2, 1, "relu", True, False),
    ("layer_k2_p0_leaky", 2, 0, "leaky_relu", True, False),
    ("layer_k3_p1_relu_res", 3, 1, "relu", True, False),
    ("layer_k3_p1_none", 3, 1, "none", False, False),
    ("layer_k3_p0_leaky", 3, 0, "leaky_relu", True, False),
    ("layer_k4_p2_relu", 4, 2, "relu", True, False),
    ("layer_k5_p2_leaky_res", 5, 2, "leaky_relu", True, False),
    ("layer_k3_p1_tanh_bn", 3, 1, "tanh", True, True),
]


def _graphs(rng, B, lo, hi, nvl, nel, equal=False):
    """B graphs of lo..hi real nodes + a dummy node (label 0, last) linked to every real node both ways; ids = local positions."""
    sizes, nedges, u, v, ids, labels, elab = [], [], [], [], [], [], []
    off = 0
    n_eq = int(rng.integers(lo, hi + 1))
    for _ in range(B):
        n = n_eq if equal else int(rng.integers(lo, hi + 1))
        E = n if equal else int(rng.integers(n - 1, n + 3))         # (sparse: the file has to stay under 1 MB)
        a = np.concatenate([rng.integers(0, n, size=E), np.full(n, n), np.arange(n)])
        b = np.concatenate([rng.integers(0, n, size=E), np.arange(n), np.full(n, n)])
        u += list(a + off)
        v += list(b + off)
        elab += list(rng.integers(0, nel, size=len(a)))
        ids += list(range(n + 1))
        labels += list(rng.integers(1, nvl, size=n)) + [0]
        sizes.append(n + 1)
        nedges.append(len(a))
        off += n + 1
    return dict(sizes=np.array(sizes, np.int64), nedges=np.array(nedges, np.int64), u=np.array(u, np.int64), v=np.array(v, np.int64),
                id=np.array(ids, np.int64), label=np.array(labels, np.int64), elabel=np.array(elab, np.int64))


def _codes(d):
    """Per graph the [n, 5] tuples (id[u], id[v], label[u], elabel, label[v]) sorted by (u, v, ul, el, vl), and the edge order."""
    out, orders, e0 = [], [], 0
    for ne in d["nedges"]:
        s = slice(e0, e0 + int(ne))
        u, v = d["u"][s], d["v"][s]
        code = np.stack([d["id"][u], d["id"][v], d["label"][u], d["elabel"][s], d["label"][v]], axis=-1)
        order = np.lexsort((code[:, 4], code[:, 3], code[:, 2], code[:, 1], code[:, 0]))
        out.append(code[order])
        orders.append(order + e0)
        e0 += int(ne)
    return out, np.concatenate(orders)


def _ref_batch(EdgeSeq, d, rev=None):
    codes, order = _codes(d)
    seqs = []
    e0 = 0
    for code in codes:
        s = EdgeSeq(code.copy())
        if rev is not None:
            s.tdata["is_reversed"] = th.from_numpy(rev[order[e0:e0 + len(code)]])
        e0 += len(code)
        seqs.append(s)
    return EdgeSeq.batch(seqs)


def _modules():
    M._si_modules()                                                  # sys.path + the bare `models` package
    cnn = importlib.import_module("models.cnn")
    dataset = importlib.import_module("dataset")
    return cnn.CNN, cnn.CNNLayer, dataset.EdgeSeq


def _sha(t):
    return hashlib.sha256(t.detach().contiguous().numpy().tobytes()).hexdigest()[:24]


def _save(fname, out, meta):
    out["meta"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    path = os.path.join(HERE, fname)
    np.savez_compressed(path, **out)
    print("%s: %d cases, %d bytes" % (fname, len(meta), os.path.getsize(path)))


def make():
    CNN, Layer, EdgeSeq = _modules()
    out, meta = {}, []
    for cid, (name, over, bopt) in enumerate(CASES):
        cfg = dict(BASE_CFG)
        cfg.update(over)
        rng = np.random.default_rng(4100 + cid)
        B = 4
        pd = _graphs(rng, B, 3, 5, cfg["max_npvl"], cfg["max_npel"], bopt.get("equal", False))
        gd = _graphs(rng, B, 6, 12, cfg["max_ngvl"], cfg["max_ngel"], bopt.get("equal", False))
        if bopt.get("all_filtered"):                                 # pair 0: the pattern's edge labels are all 1, the graph's all 2
            pd["elabel"][:int(pd["nedges"][0])] = 1
            gd["elabel"][:int(gd["nedges"][0])] = 2
        p_rev = g_rev = None
        if bopt.get("rev"):
            p_rev, g_rev = rng.random(len(pd["u"])) < 0.3, rng.random(len(gd["u"])) < 0.3
            pd["is_reversed"], gd["is_reversed"] = p_rev, g_rev
        pattern, graph = _ref_batch(EdgeSeq, pd, p_rev), _ref_batch(EdgeSeq, gd, g_rev)
        seed = 9500 + cid
        th.manual_seed(seed)
        model = CNN(**cfg)
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
        for side, d, seq in (("p", pd, pattern), ("g", gd, graph)):
            for k, a in d.items():
                arrs["%s/%s" % (side, k)] = a
            for k in ("u", "v", "ul", "el", "vl") + (("is_reversed",) if "is_reversed" in seq.tdata else ()):
                arrs["%s/seq/%s" % (side, k)] = seq.tdata[k].numpy().copy()
            arrs["%s/seq/lens" % side] = np.array(seq._batch_num_tuples, np.int64)
            arrs["%s/seq/num_nodes" % side] = seq.batch_num_nodes().numpy().copy()
        model.train()
        res = model(pattern, graph)
        assert list(res.keys()) == list(KEYS), list(res.keys())
        for side, seq in (("p", pattern), ("g", graph)):             # (the tables the forward cached, or builds now)
            arrs["%s/seq/in_deg" % side] = seq.in_degrees().numpy().copy()
            arrs["%s/seq/out_deg" % side] = seq.out_degrees().numpy().copy()
        res["p_e_rep"].retain_grad()
        res["g_e_rep"].retain_grad()
        c = th.arange(1, B + 1, dtype=th.float32).view(-1, 1) / B
        loss = (res["pred_c"] * c).sum()
        if res["pred_e"] is not None:
            ce = th.from_numpy(rng.standard_normal(tuple(res["pred_e"].shape)).astype(np.float32))
            arrs["coef_e"] = ce.numpy()
            loss = loss + (res["pred_e"] * ce).sum()
        loss.backward()
        none_out = []
        for k in KEYS:
            if res[k] is None:
                none_out.append(k)
            else:
                a = res[k].detach().numpy()
                assert a.dtype == bool or np.isfinite(a).all(), (name, k)
                arrs["out/%s" % k] = a
        arrs["grad_rep/p"] = res["p_e_rep"].grad.numpy()
        arrs["grad_rep/g"] = res["g_e_rep"].grad.numpy()
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
        print("%s: pred_c %s, gate %d of %d" % (name, np.round(arrs["out/pred_c"].reshape(-1)[:3], 4),
                                                int(arrs["out/g_e_mask"].sum()), arrs["out/g_e_mask"].size))
        if cid + 1 == FIRST_FILE_CASES:
            _save("si_cnn.npz", out, meta)
            out, meta = {}, []
    for lid, (name, k, p, act, residual, bn) in enumerate(LAYER_CASES):
        rng = np.random.default_rng(4200 + lid)
        seed = 9600 + lid
        th.manual_seed(seed)
        layer = Layer(C, C, kernel_size=k, padding=p, batch_norm=bn, act_func=act)
        tag = "l%02d" % lid
        arrs = {}
        keys = list(layer.state_dict().keys())
        init_sha = {kk: _sha(t) for kk, t in layer.state_dict().items()}
        with th.no_grad():
            for q in layer.parameters():
                q.add_(0.2 * th.randn_like(q))                       # (the bias gets both signs)
        for kk, t in layer.state_dict().items():
            arrs["param/%s" % kk] = t.numpy().copy()
        B, L = 4, 14
        lens = np.array([L, 1, k, 9], np.int64)
        gate = np.zeros((B, L), np.float32)
        for b in range(B):
            gate[b, L - lens[b]:] = 1.0
        gate[0, [L - lens[0], 5, 6, L - 1]] = 0.0                    # zeros at the first, two interior and the last live position
        gate[3, L - 9:] = (rng.random(9) < 0.5).astype(np.float32)
        x = th.from_numpy(rng.standard_normal((B, L, C)).astype(np.float32)).requires_grad_(True)
        g = th.from_numpy(gate).view(B, 1, L)
        x0 = x.transpose(1, 2) * g
        g2 = F.max_pool1d(F.max_pool1d(g, kernel_size=k, stride=1, padding=p), kernel_size=k, stride=1, padding=p)
        layer.train()
        o = layer(x0) * g2
        if residual and o.size() == x0.size():
            o = o + x0
        y = o.transpose(1, 2)
        coef = th.from_numpy(rng.standard_normal(tuple(y.shape)).astype(np.float32))
        (y * coef).sum().backward()
        arrs.update({"in/x": x.detach().numpy(), "in/gate": gate, "in/lens": lens, "in/coef": coef.numpy(),
                     "out/y": y.detach().numpy(), "out/gate": g2.view(B, -1).numpy(), "grad_in/x": x.grad.numpy()})
        for kk, q in layer.named_parameters():
            arrs["grad/%s" % kk] = q.grad.numpy()
        buffers = [kk for kk, _ in layer.named_buffers()]
        for kk in buffers:
            arrs["after/%s" % kk] = layer.state_dict()[kk].numpy().copy()
        m = dict(tag=tag, name=name, kind="layer", kw=dict(kernel_size=k, padding=p, batch_norm=bn, act_func=act), residual=residual,
                 C=C, seed=seed, keys=keys, alias={}, init_sha=init_sha, params=[kk for kk, _ in layer.named_parameters()],
                 none_grad=[], buffers=buffers)
        m["index"] = M._pack(out, tag, arrs)
        meta.append(m)
        print("%s: |y| max %.4f, L2 %d" % (name, float(np.abs(arrs["out/y"]).max()), y.shape[1]))
    _save("si_cnn_layers.npz", out, meta)


if __name__ == "__main__":
    make()
