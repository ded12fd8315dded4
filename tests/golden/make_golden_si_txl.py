"""Golden vectors of the SI count model TransformerXL(**cfg) on edge sequences and of TXLLayer (subgraph_isomorphism/models/txl.py,
basemodel.py EdgeSeqModel, dataset.py EdgeSeq), run on the CPU from the reference's own code with the stand-ins of _ref_standins.py.

Run on the authoring box only (needs the reference checkout), like make_golden_si_rnn.py:
    python tests/golden/make_golden_si_txl.py
Writes si_txl.npz and, because a committed file stays under 1 MiB, si_txl_2.npz, ... (the cases in order, as many per file as fit).
Data only.

The reference's MixtureDict does not work under this torch: `key in ParameterDict` is false for a parameter added through
register_parameter, so net["txl"] raises KeyError, and len(net) counts 1 where the reference's torch counted 3.  The shim below (local
to this script) looks a key up in _buffers / _parameters / _modules and has __len__ count all three, which is what the reference's
torch did; init_mems(len(net)) then makes 4 memories, enough for the 1 and 3 layers of these cases.

Per model case (hid_dim 16; 64 in the case heads4, so that its heads are 16 wide): what make_golden_si_rnn.py stores per model case.  The graph sequences have 70 - 150 tuples (2 - 3 segments of 64, a
length that is no multiple of 64).  Per layer case: ONE TXLLayer call on a 64-row segment with an empty, a 64-row or a 32-row memory:
the input w (width 16, or 64 at 4 heads), the memory, the position rows r (relative positions klen - 1 .. 0), r_w_bias, r_r_bias, the loss coefficients, the output
and the gradients of w, r_w_bias, r_r_bias and every parameter.

The perturbation: + 0.05 N(0, 1) on every weight, + 0.3 N(0, 1) on every bias and on the LayerNorm weights and biases, so that none of
them is trivial."""
import importlib
import os
import sys

import numpy as np
import torch as th

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_si_models as M  # noqa: E402  (installs the stand-ins; BASE_CFG, the packing)
import make_golden_si_cnn as C  # noqa: E402  (the batches, the hashing, the file writer)

KEYS = M.KEYS
BASE_CFG = dict(M.BASE_CFG, rep_net="TXL", rep_num_graph_layers=2, rep_num_pattern_layers=2, rep_act_func="relu",
                emb_net="Equivariant", max_ngv=64, max_nge=256, max_npv=64, max_npe=256)
for _k in [k for k in BASE_CFG if k.startswith(("rep_rgin", "rep_rgcn"))]:
    del BASE_CFG[_k]

_NO_SHARE = {"share_enc_net": False, "share_emb_net": False, "share_rep_net": False}


def _layers(n):
    return {"rep_num_graph_layers": n, "rep_num_pattern_layers": n}


# (name, config overrides, batch options)
CASES = [
    ("defaults", {}, {}),
    ("heads4", {"num_heads": 4, "hid_dim": 64}, {}),                 # (head width 16: inside the kernels' predicate)
    ("pre_lnorm", {"pre_lnorm": True}, {}),
    ("mem32", {"mem_len": 32}, {}),
    ("seg16", {"seg_len": 16}, {}),
    ("clamp20", {"clamp_len": 20}, {}),
    ("layers1", _layers(1), {}),
    ("layers3", dict(_layers(3), num_heads=4), {}),
    ("no_share", dict(_NO_SHARE, pre_lnorm=True), {}),
    ("position", {"enc_net": "Position"}, {}),
    ("mean_head", {"pred_net": "MeanPredictNet", "mem_len": 32}, {}),
    ("edge_weights", {"pred_return_weights": "edge", "num_heads": 4}, {}),
    ("equal_lengths", {}, {"equal": True}),
    ("all_filtered", {}, {"all_filtered": True}),
    ("revflag", {}, {"rev": True}),
    ("dropout_eval", {"rep_dropout": 0.3}, {"eval": True}),
]
INIT_VALUE_CASES = ("defaults",)
# TXLLayer cases: (memory rows, pre_lnorm, heads)
LAYER_GRID = [(mem, pre, heads) for mem in (0, 64, 32) for pre in (False, True) for heads in (1, 4)]
LAYER_H, LAYER_Q, LAYER_B = 16, 64, 3


def _shim(container):
    def getitem(self, key):
        for d in (self._buffer_dict._buffers, self._param_dict._parameters, self._module_dict._modules):
            if key in d:
                return d[key]
        raise KeyError(key)

    def length(self):
        return len(self._buffer_dict._buffers) + len(self._param_dict._parameters) + len(self._module_dict._modules)

    container.MixtureDict.__getitem__ = getitem
    container.MixtureDict.__len__ = length


def _modules():
    M._si_modules()
    _shim(importlib.import_module("models.container"))
    txl = importlib.import_module("models.txl")
    dataset = importlib.import_module("dataset")
    embed = importlib.import_module("models.embed")
    return txl.TransformerXL, txl.TXLLayer, dataset.EdgeSeq, embed.PositionEmbedding


def _perturb(named):
    with th.no_grad():
        for k, p in named:
            if p.requires_grad:
                p.add_((0.3 if ("bias" in k.split(".")[-1] or "layer_norm" in k) else 0.05) * th.randn_like(p))


def make():
    TXL, Layer, EdgeSeq, PositionEmbedding = _modules()
    items = []                                                       # (the case's packed arrays, its meta)
    for cid, (name, over, bopt) in enumerate(CASES):
        cfg = dict(BASE_CFG)
        cfg.update(over)
        B = 4
        for attempt in range(8):                                     # (redrawn while the longest sequence is a multiple of 64)
            rng = np.random.default_rng(6100 + cid + 1000 * attempt)
            pd = C._graphs(rng, B, 3, 5, cfg["max_npvl"], cfg["max_npel"], bopt.get("equal", False))
            gd = C._graphs(rng, B, 24, 48, cfg["max_ngvl"], cfg["max_ngel"], bopt.get("equal", False))
            if int(gd["nedges"].max()) % 64 != 0:
                break
        if bopt.get("all_filtered"):                                 # pair 0: the pattern's edge labels are all 1, the graph's all 2
            pd["elabel"][:int(pd["nedges"][0])] = 1
            gd["elabel"][:int(gd["nedges"][0])] = 2
        p_rev = g_rev = None
        if bopt.get("rev"):
            p_rev, g_rev = rng.random(len(pd["u"])) < 0.3, rng.random(len(gd["u"])) < 0.3
            pd["is_reversed"], gd["is_reversed"] = p_rev, g_rev
        pattern, graph = C._ref_batch(EdgeSeq, pd, p_rev), C._ref_batch(EdgeSeq, gd, g_rev)
        seed = 9900 + cid
        th.manual_seed(seed)
        model = TXL(**cfg)
        tag = "m%02d" % cid
        arrs = {}
        alias, first = {}, {}
        for k, t in model.state_dict(keep_vars=True).items():        # shared modules: their p_* keys are the g_* tensors
            if id(t) in first:
                alias[k] = first[id(t)]
            else:
                first[id(t)] = k
        init_sha = {k: C._sha(t) for k, t in model.state_dict().items()}
        shapes = {k: list(t.shape) for k, t in model.state_dict().items()}
        if name in INIT_VALUE_CASES:
            for k, t in model.state_dict().items():
                if k not in alias:
                    arrs["init/%s" % k] = t.numpy().copy()
        _perturb(model.named_parameters())
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
        mode = "eval" if bopt.get("eval") else "train"
        model.train(mode == "train")
        res = model(pattern, graph)
        assert list(res.keys()) == list(KEYS), list(res.keys())
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
        Lg = arrs["g/seq/u"].shape[1]
        if not bopt.get("equal"):
            assert 70 <= int(arrs["g/seq/lens"].min()) and Lg <= 150 and Lg % 64 != 0, arrs["g/seq/lens"]
        m = dict(tag=tag, name=name, kind="model", cfg=cfg, seed=seed, B=B, mode=mode, none_out=none_out, none_grad=none_grad,
                 alias=alias, init_sha=init_sha, shapes=shapes, keys=list(model.state_dict().keys()),
                 params=[k for k, _ in model.named_parameters()], buffers=buffers)
        out = {}
        m["index"] = M._pack(out, tag, arrs)
        items.append((out, m))
        print("%s: pred_c %s, Lg %d, gate %d of %d" % (name, np.round(arrs["out/pred_c"].reshape(-1)[:3], 4), Lg,
                                                       int(arrs["out/g_e_mask"].sum()), arrs["out/g_e_mask"].size))
    for lid, (mem, pre, heads) in enumerate(LAYER_GRID):
        name = "layer_mem%d_%s_h%d" % (mem, "pre" if pre else "post", heads)
        rng = np.random.default_rng(6200 + lid)
        seed = 10000 + lid
        th.manual_seed(seed)
        H, Q, B = LAYER_H * (4 if heads == 4 else 1), LAYER_Q, LAYER_B     # (head width 16 either way)
        layer = Layer(H, H, num_heads=heads, pre_lnorm=pre)
        pos_emb = PositionEmbedding(H, max_len=128)
        tag = "l%02d" % lid
        arrs = {}
        keys = list(layer.state_dict().keys())
        init_sha = {kk: C._sha(t) for kk, t in layer.state_dict().items()}
        _perturb(layer.named_parameters())
        for kk, t in layer.state_dict().items():
            arrs["param/%s" % kk] = t.numpy().copy()
        klen = Q + mem
        w = th.from_numpy(rng.standard_normal((B, Q, H)).astype(np.float32)).requires_grad_(True)
        mems = th.from_numpy(rng.standard_normal((B, mem, H)).astype(np.float32))
        r = pos_emb(th.arange(klen - 1, -1, -1)).detach().unsqueeze(0)
        rwb = th.from_numpy((0.5 * rng.standard_normal((heads, H // heads))).astype(np.float32)).requires_grad_(True)
        rrb = th.from_numpy((0.5 * rng.standard_normal((heads, H // heads))).astype(np.float32)).requires_grad_(True)
        mask = th.ones((Q, klen), dtype=th.bool).unsqueeze(0)
        layer.train()
        y = layer(w, r, rwb, rrb, attn_mask=mask, mems=mems if mem > 0 else None)
        coef = th.from_numpy(rng.standard_normal(tuple(y.shape)).astype(np.float32))
        (y * coef).sum().backward()
        arrs.update({"in/w": w.detach().numpy(), "in/mems": mems.numpy(), "in/r": r.numpy(), "in/r_w_bias": rwb.detach().numpy(),
                     "in/r_r_bias": rrb.detach().numpy(), "in/coef": coef.numpy(), "out/y": y.detach().numpy(),
                     "grad_in/w": w.grad.numpy(), "grad_in/r_w_bias": rwb.grad.numpy(), "grad_in/r_r_bias": rrb.grad.numpy()})
        for kk, q in layer.named_parameters():
            arrs["grad/%s" % kk] = q.grad.numpy()
        m = dict(tag=tag, name=name, kind="layer", mem=mem, pre_lnorm=pre, heads=heads, H=H, seed=seed, keys=keys, alias={},
                 init_sha=init_sha, params=[kk for kk, _ in layer.named_parameters()], none_grad=[], buffers=[])
        out = {}
        m["index"] = M._pack(out, tag, arrs)
        items.append((out, m))
        print("%s: |y| max %.4f" % (name, float(np.abs(arrs["out/y"]).max())))
    _write(items)


def _fname(i):
    return "si_txl.npz" if i == 0 else "si_txl_%d.npz" % (i + 1)


def _write(items, limit=1000000):
    """The cases in order into si_txl.npz, si_txl_2.npz, ...: as many per file as stay under `limit` bytes."""
    for f in os.listdir(HERE):
        if f.startswith("si_txl") and f.endswith(".npz"):
            os.remove(os.path.join(HERE, f))

    def save(i, chunk):
        out = {}
        for o, _ in chunk:
            out.update(o)
        C._save(_fname(i), out, [m for _, m in chunk])
        return os.path.getsize(os.path.join(HERE, _fname(i)))

    i, cur = 0, []
    for it in items:
        if cur and save(i, cur + [it]) > limit:
            save(i, cur)
            i, cur = i + 1, []
        cur.append(it)
    save(i, cur)


if __name__ == "__main__":
    make()
