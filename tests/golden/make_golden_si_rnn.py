"""Golden vectors of the SI count model RNN(**cfg) on edge sequences and of RNNLayer (subgraph_isomorphism/models/rnn.py,
basemodel.py EdgeSeqModel, dataset.py EdgeSeq), run on the CPU from the reference's own code with the stand-ins of _ref_standins.py.

Run on the authoring box only (needs the reference checkout), like make_golden_si_cnn.py:
    python tests/golden/make_golden_si_rnn.py
Writes si_rnn.npz and, because a committed file stays under 1 MiB, si_rnn_2.npz, ... (the cases in order, as many per file as fit).
Data only.

Per model case: what make_golden_si_cnn.py stores per model case (the config, both batches as graphs and as the reference's batched
EdgeSeq, a sha256 of every initial state_dict tensor, the perturbed parameters, every OutputDict tensor, the gradient of every
parameter and of p_e_rep / g_e_rep), plus the mode the forward ran in (eval for the dropout case).  Per layer case: the input, the
gate, the lengths, the loss coefficients, y = layer(x * gate) * gate (+ x * gate when residual) and the gradients of the input and
the parameters.

The perturbation keeps the recurrent weights at the scale they are initialised with (+ 0.05 N(0, 1)) and gives every bias of the
recurrent layers 0.3 N(0, 1): both signs, and b_ih != b_hh (the GRU's n gate tells them apart)."""
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
BASE_CFG = dict(M.BASE_CFG, rep_net="RNN", rep_num_graph_layers=2, rep_num_pattern_layers=2, rep_rnn_type="LSTM",
                rep_rnn_bidirectional=False, emb_net="Equivariant")
for _k in [k for k in BASE_CFG if k.startswith(("rep_rgin", "rep_rgcn", "rep_act_func"))]:
    del BASE_CFG[_k]

_NO_SHARE = {"share_enc_net": False, "share_emb_net": False, "share_rep_net": False}
_BI32 = {"rep_rnn_bidirectional": True, "hid_dim": 32}


def _layers(n):
    return {"rep_num_graph_layers": n, "rep_num_pattern_layers": n}


# (name, config overrides, batch options)
CASES = [
    ("lstm", {}, {}),
    ("gru", {"rep_rnn_type": "GRU"}, {}),
    ("rnn", {"rep_rnn_type": "RNN"}, {}),
    ("lstm_bi", dict(_BI32), {}),
    ("gru_bi", dict(_BI32, rep_rnn_type="GRU"), {}),
    ("rnn_bi", dict(_BI32, rep_rnn_type="RNN"), {}),
    ("gru_bi_hd8", {"rep_rnn_type": "GRU", "rep_rnn_bidirectional": True}, {}),
    ("lstm_no_residual", {"rep_residual": False}, {}),
    ("gru_layers1", dict(_layers(1), rep_rnn_type="GRU"), {}),
    ("lstm_layers3", _layers(3), {}),
    ("no_share", dict(_NO_SHARE, rep_rnn_type="GRU"), {}),
    ("position", {"enc_net": "Position"}, {}),
    ("mean_head", {"pred_net": "MeanPredictNet", "rep_rnn_type": "RNN"}, {}),
    ("edge_weights", {"pred_return_weights": "edge", "rep_rnn_type": "GRU"}, {}),
    ("equal_lengths", {}, {"equal": True}),
    ("all_filtered", {"rep_rnn_type": "GRU"}, {"all_filtered": True}),
    ("revflag", {}, {"rev": True}),
    ("dropout_eval", {"rep_dropout": 0.3, "rep_rnn_type": "GRU"}, {"eval": True}),
]
INIT_VALUE_CASES = ("lstm",)
# RNNLayer cases: (rnn type, bidirectional) x the (gate, residual) variants of the direction; width 16, or 32 when bidirectional
LAYER_GRID = [(t, bi) for t in ("LSTM", "GRU", "RNN") for bi in (False, True)]
VARIANTS = {False: [(True, True), (True, False), (False, True), (False, False)], True: [(True, True), (False, False)]}


def _modules():
    M._si_modules()
    rnn = importlib.import_module("models.rnn")
    dataset = importlib.import_module("dataset")
    return rnn.RNN, rnn.RNNLayer, dataset.EdgeSeq


def _perturb(named):
    with th.no_grad():
        for k, p in named:
            if p.requires_grad:
                p.add_((0.3 if "layer.bias" in k else 0.05) * th.randn_like(p))


def make():
    RNN, Layer, EdgeSeq = _modules()
    items = []                                                       # (the case's packed arrays, its meta)
    for cid, (name, over, bopt) in enumerate(CASES):
        cfg = dict(BASE_CFG)
        cfg.update(over)
        rng = np.random.default_rng(5100 + cid)
        B = 4
        pd = C._graphs(rng, B, 3, 5, cfg["max_npvl"], cfg["max_npel"], bopt.get("equal", False))
        gd = C._graphs(rng, B, 6, 12, cfg["max_ngvl"], cfg["max_ngel"], bopt.get("equal", False))
        if bopt.get("all_filtered"):                                 # pair 0: the pattern's edge labels are all 1, the graph's all 2
            pd["elabel"][:int(pd["nedges"][0])] = 1
            gd["elabel"][:int(gd["nedges"][0])] = 2
        p_rev = g_rev = None
        if bopt.get("rev"):
            p_rev, g_rev = rng.random(len(pd["u"])) < 0.3, rng.random(len(gd["u"])) < 0.3
            pd["is_reversed"], gd["is_reversed"] = p_rev, g_rev
        pattern, graph = C._ref_batch(EdgeSeq, pd, p_rev), C._ref_batch(EdgeSeq, gd, g_rev)
        seed = 9700 + cid
        th.manual_seed(seed)
        model = RNN(**cfg)
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
        for k in [k for k in model.state_dict() if ".layer.bias_ih" in k]:      # the two biases differ and carry both signs
            a, b = arrs["param/%s" % alias.get(k, k)], arrs["param/%s" % alias.get(k, k).replace("bias_ih", "bias_hh")]
            assert (a > 0).any() and (a < 0).any() and not np.array_equal(a, b), k
        m = dict(tag=tag, name=name, kind="model", cfg=cfg, seed=seed, B=B, mode=mode, none_out=none_out, none_grad=none_grad,
                 alias=alias, init_sha=init_sha, shapes=shapes, keys=list(model.state_dict().keys()),
                 params=[k for k, _ in model.named_parameters()], buffers=buffers)
        out = {}
        m["index"] = M._pack(out, tag, arrs)
        items.append((out, m))
        print("%s: pred_c %s, gate %d of %d" % (name, np.round(arrs["out/pred_c"].reshape(-1)[:3], 4),
                                                int(arrs["out/g_e_mask"].sum()), arrs["out/g_e_mask"].size))
    lid = 0
    for rnn_type, bi in LAYER_GRID:
        for gated, residual in VARIANTS[bi]:
            name = "layer_%s%s%s%s" % (rnn_type.lower(), "_bi" if bi else "", "_gate" if gated else "", "_res" if residual else "")
            rng = np.random.default_rng(5200 + lid)
            seed = 9800 + lid
            th.manual_seed(seed)
            H = 32 if bi else 16
            layer = Layer(rnn_type, H, H, bidirectional=bi)
            tag = "l%02d" % lid
            arrs = {}
            keys = list(layer.state_dict().keys())
            init_sha = {kk: C._sha(t) for kk, t in layer.state_dict().items()}
            _perturb(layer.named_parameters())
            for kk, t in layer.state_dict().items():
                arrs["param/%s" % kk] = t.numpy().copy()
            B, L = 4, 14
            lens = np.array([L, 1, 3, 9], np.int64)
            gate = np.ones((B, L), np.float32)
            if gated:
                gate[:] = 0.0
                for b in range(B):
                    gate[b, L - lens[b]:] = 1.0
                gate[0, [0, 5, 6, L - 1]] = 0.0                      # zeros at the first, two interior and the last live position
                gate[3, L - 9:] = (rng.random(9) < 0.5).astype(np.float32)
            else:
                lens = np.array([L] * B, np.int64)
            x = th.from_numpy(rng.standard_normal((B, L, H)).astype(np.float32)).requires_grad_(True)
            g = th.from_numpy(gate).view(B, L, 1)
            x0 = x * g
            layer.train()
            o = layer(x0) * g
            y = x0 + o if residual and o.size() == x0.size() else o
            coef = th.from_numpy(rng.standard_normal(tuple(y.shape)).astype(np.float32))
            (y * coef).sum().backward()
            arrs.update({"in/x": x.detach().numpy(), "in/gate": gate, "in/lens": lens, "in/coef": coef.numpy(),
                         "out/y": y.detach().numpy(), "grad_in/x": x.grad.numpy()})
            for kk, q in layer.named_parameters():
                arrs["grad/%s" % kk] = q.grad.numpy()
            m = dict(tag=tag, name=name, kind="layer", rnn_type=rnn_type, bidirectional=bi, H=H, gated=gated, residual=residual,
                     seed=seed, keys=keys, alias={}, init_sha=init_sha, params=[kk for kk, _ in layer.named_parameters()],
                     none_grad=[], buffers=[])
            out = {}
            m["index"] = M._pack(out, tag, arrs)
            items.append((out, m))
            lid += 1
            print("%s: |y| max %.4f" % (name, float(np.abs(arrs["out/y"]).max())))
    _write(items)


def _fname(i):
    return "si_rnn.npz" if i == 0 else "si_rnn_%d.npz" % (i + 1)


def _write(items, limit=1000000):
    """The cases in order into si_rnn.npz, si_rnn_2.npz, ...: as many per file as stay under `limit` bytes."""
    for f in os.listdir(HERE):
        if f.startswith("si_rnn") and f.endswith(".npz"):
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
