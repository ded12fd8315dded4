"""Step time of the SI count models CompGCN / DMPNN on the scale batch (config-3 graphs with reversed and dummy edges, 512 seeded
patterns, H = 64): eager, synchronised, median of --steps steps after --warmup warm-ups.

  --impl model      CompGCN(**cfg) / DMPNN(**cfg) of this package (HIP glue; the layers on their default path, --fused: on dn_dual.hip)
  --impl composed   the same model put together from the pieces a tree WITHOUT those models has: its CompGCNLayer / DMPLayer
                    (forced onto the composed path where ops.dual_composed exists), its embeddings and heads, and the glue written
                    as the reference writes it (padded filter, per-graph mask loops, concatenated padded head rows)
  --layer           time one CompGCNLayer / DMPLayer forward + backward alone (--comp-opt for CompGCN; --impl model --fused: the
                    fused layer, else the composed one)

The tool only needs what both trees have, so the same file runs on a parent checkout for A/B runs.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dummynode4graphlearning_amd import BatchedGraph, ops, synthetic, transforms  # noqa: E402
from dummynode4graphlearning_amd import subgraph_isomorphism as si  # noqa: E402
from dummynode4graphlearning_amd.subgraph_isomorphism import bookkeeping  # noqa: E402
from dummynode4graphlearning_amd.subgraph_isomorphism.graph_adj import MultihotEmbedding, OrthogonalEmbedding, get_enc_len  # noqa: E402

DEV = "cuda:0"


def scale_batches(seed=0):
    raw = synthetic.config3()
    vocab = (raw["max_nv"], raw["max_nvl"], raw["max_ne"], raw["max_nel"])
    rng = np.random.default_rng(seed)
    G = 512
    n = rng.integers(3, 10, size=G)
    m = np.array([int(rng.integers(k, 2 * k + 1)) for k in n])
    node_ptr, edge_ptr = np.concatenate([[0], np.cumsum(n)]), np.concatenate([[0], np.cumsum(m)])
    src = np.concatenate([rng.integers(0, k, size=e) + o for k, e, o in zip(n, m, node_ptr[:-1])])
    dst = np.concatenate([rng.integers(0, k, size=e) + o for k, e, o in zip(n, m, node_ptr[:-1])])
    pat = dict(node_ptr=node_ptr, edge_ptr=edge_ptr, src=src, dst=dst, node_id=np.concatenate([np.arange(k) for k in n]),
               node_label=rng.integers(0, raw["max_nvl"], size=int(n.sum())), edge_id=np.concatenate([np.arange(e) for e in m]),
               edge_label=rng.integers(0, raw["max_nel"], size=int(m.sum())))
    out, nel = [], 0
    for b in (pat, raw):
        t = {k: torch.from_numpy(np.asarray(b[k], np.int64)).to(DEV) for k in
             ("node_ptr", "edge_ptr", "src", "dst", "node_id", "node_label", "edge_id", "edge_label")}
        r = bookkeeping.add_reversed_edges(t["edge_ptr"], t["src"], t["dst"], t["edge_id"], t["edge_label"], vocab[2], vocab[3])
        aug = transforms.dummy_augment_si(t["node_ptr"], r["edge_ptr"], r["src"], r["dst"], t["node_id"], t["node_label"], r["edge_id"],
                                          r["edge_label"], vocab[0], vocab[1], 2 * vocab[2], 2 * vocab[3], is_reversed=r["is_reversed"])
        nel = max(nel, int(aug["edge_label"].max()) + 1)
        out.append(aug)
    return out[0], out[1], nel


def graph_of(aug):
    N = int(aug["node_label"].numel())
    return BatchedGraph(aug["src"], aug["dst"], N, batch_num_nodes=(aug["node_ptr"][1:] - aug["node_ptr"][:-1]).long(),
                        batch_num_edges=(aug["edge_ptr"][1:] - aug["edge_ptr"][:-1]).long(),
                        ndata={"id": aug["node_id"], "label": aug["node_label"], "is_dummy": aug["is_dummy_node"].bool()},
                        edata={"label": aug["edge_label"], "is_dummy": aug["is_dummy_edge"].bool(),
                               "is_reversed": aug["is_reversed"].bool()}, node_ptr=aug["node_ptr"], edge_ptr=aug["edge_ptr"])


def config(rep_net, nel):
    return dict(max_ngv=64, max_ngvl=8, max_nge=512, max_ngel=nel, max_npv=64, max_npvl=8, max_npe=512, max_npel=nel, base=2,
                enc_net="Multihot", emb_net="Orthogonal", filter_net="ScalarFilter", rep_net=rep_net, rep_num_graph_layers=3,
                rep_num_pattern_layers=3, rep_act_func="leaky_relu", rep_residual=True, share_enc_net=True, share_emb_net=True,
                share_rep_net=True, pred_net="SumPredictNet", pred_with_enc=True, pred_with_deg=True, hid_dim=64, pred_hid_dim=64,
                pred_dropout=0.0, rep_dropout=0.0, pred_return_weights="none")


class _layer_path:
    """ops.dual_fused(fused) where the tree has it (this tree), a no-op on a tree whose layers only have the composed path."""

    def __init__(self, fused):
        self.fused = fused

    def __enter__(self):
        self.cm = ops.dual_fused(self.fused) if hasattr(ops, "dual_fused") else None
        if self.cm is not None:
            self.cm.__enter__()

    def __exit__(self, *exc):
        if self.cm is not None:
            self.cm.__exit__(*exc)
        return False


class ComposedModel(nn.Module):
    """GraphAdjModelV2.forward (basemodel.py:1520-1703) written with torch ops around the package's dual layers, embeddings and
    pred nets: what a user of a tree without CompGCN / DMPNN would put together.  Defaults only (shared nets, Sum head with
    encodings and degrees, filter on, no id terms)."""

    def __init__(self, cfg):
        super().__init__()
        self.cfg, H, base = cfg, cfg["hid_dim"], cfg["base"]
        sizes = {"v": cfg["max_ngv"], "vl": cfg["max_ngvl"], "el": cfg["max_ngel"]}
        self.enc = nn.ModuleDict({k: MultihotEmbedding(n, base) for k, n in sizes.items()})
        for m in self.enc.values():
            m.weight.requires_grad = False
        dims = {k: get_enc_len(n - 1, base) * base for k, n in sizes.items()}
        self.emb = nn.ModuleDict({k: OrthogonalEmbedding(d, H) for k, d in dims.items()})
        if cfg["rep_net"] == "CompGCN":
            self.layers = nn.ModuleList([si.CompGCNLayer(H, H, comp_opt="mult", edge_norm="none", batch_norm=False,
                                                         act_func=cfg["rep_act_func"]) for _ in range(cfg["rep_num_graph_layers"])])
        else:
            self.layers = nn.ModuleList([si.DMPLayer(H, H, num_mlp_layers=2, batch_norm=False, act_func=cfg["rep_act_func"])
                                         for _ in range(cfg["rep_num_graph_layers"])])
        dv, de = dims["v"] + dims["vl"], 2 * (dims["v"] + dims["vl"]) + dims["el"]
        self.pred = nn.ModuleDict({"v": si.SumPredictNet(H + dv + 2, hidden_dim=cfg["pred_hid_dim"]),
                                   "e": si.SumPredictNet(H + de + 2, hidden_dim=cfg["pred_hid_dim"])})

    @staticmethod
    def _mask(lens):
        L = int(lens.max())
        return torch.arange(L, device=lens.device).view(1, -1) >= (L - lens).view(-1, 1)

    @staticmethod
    def _gate(p_lab, p_len, g_lab, g_len):
        pad = si.split_and_batchify_graph_feats
        p = pad(p_lab.view(-1, 1), p_len, pre_pad=True)[0]
        g = pad(g_lab.view(-1, 1), g_len, pre_pad=True)[0]
        gate = ((g.unsqueeze(2) - p.unsqueeze(1)) == 0).max(dim=2)[0]                       # ScalarFilter, filter.py:10-16
        keep = ComposedModel._mask(g_len)
        return gate.view(gate.shape[0], -1)[keep].view(-1, 1)

    def _reps(self, g, v, e, vg=None, eg=None):
        if vg is not None:
            v, e = v * vg, e * eg
        for layer in self.layers:
            nv, ne = layer(g, v, e)
            if vg is not None:
                nv, ne = nv * vg, ne * eg
            v, e = v + nv, e + ne
        return v, e

    def forward(self, pattern, graph):
        pad = si.split_and_batchify_graph_feats
        sides = []
        for g in (pattern, graph):
            u, v = (t.long() for t in g.all_edges())
            enc = {"v": self.enc["v"](g.ndata["id"].long()), "vl": self.enc["vl"](g.ndata["label"].long()),
                   "el": self.enc["el"](g.edata["label"].long())}
            sides.append(dict(g=g, u=u, v=v, enc=enc, v_emb=self.emb["vl"](enc["vl"]), e_emb=self.emb["el"](enc["el"]),
                              nl=g.batch_num_nodes(), el=g.batch_num_edges()))
        P, G = sides
        dt = P["v_emb"].dtype
        vg = self._gate(pattern.ndata["label"].long(), P["nl"], graph.ndata["label"].long(), G["nl"]).to(dt)
        eg = self._gate(pattern.edata["label"].long(), P["el"], graph.edata["label"].long(), G["el"]).to(dt)
        P["v_rep"], P["e_rep"] = self._reps(pattern, P["v_emb"], P["e_emb"])
        G["v_rep"], G["e_rep"] = self._reps(graph, G["v_emb"], G["e_emb"], vg, eg)
        outs = {}
        for s in sides:
            g = s["g"]
            vm = self._mask(s["nl"]).unsqueeze(-1)
            vm = vm.masked_fill(pad(g.ndata["is_dummy"].view(-1, 1), s["nl"], pre_pad=True)[0].bool(), 0)
            em = self._mask(s["el"]).unsqueeze(-1)
            em = em.masked_fill(pad(g.edata["is_dummy"].view(-1, 1), s["el"], pre_pad=True)[0].bool(), 0)
            em = em.masked_fill(pad(g.edata["is_reversed"].view(-1, 1), s["el"], pre_pad=True)[0].bool(), 0)
            od, idg = g.out_degrees().to(dt).view(-1, 1), g.in_degrees().to(dt).view(-1, 1)
            enc, u, v = s["enc"], s["u"], s["v"]
            vo = torch.cat([enc["v"], enc["vl"], od, idg, s["v_rep"]], dim=-1)
            eo = torch.cat([enc["v"][u], enc["v"][v], enc["vl"][u], enc["el"], enc["vl"][v], od[u], idg[v], s["e_rep"]], dim=-1)
            s["vo"] = pad(vo, s["nl"], pre_pad=True)[0].masked_fill(~vm, 0)
            s["eo"] = pad(eo, s["el"], pre_pad=True)[0].masked_fill(~em, 0)
            s["vm"], s["em"] = vm.squeeze(-1), em.squeeze(-1)
        yv, _ = self.pred["v"](P["vo"], P["vm"], G["vo"], G["vm"])
        ye, _ = self.pred["e"](P["eo"], P["em"], G["eo"], G["em"])
        lv, le = G["vm"].float().sum(1).view(-1, 1), G["em"].float().sum(1).view(-1, 1)
        return {"pred_c": (lv / (lv + le)).to(dt) * yv + (le / (lv + le)).to(dt) * ye}


def perturb(model):
    with torch.no_grad():
        for p in model.parameters():
            if p.requires_grad:
                p.add_(0.05 * torch.randn_like(p))
    return model


def timed(step, steps, warmup):
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    times = []
    for _ in range(steps):
        t0 = time.perf_counter()
        step()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return times


def run_one(a, batches):
    dtype = torch.float32 if a.dtype == "fp32" else torch.bfloat16
    pg, gg, nel = batches
    rep_net = "CompGCN" if a.model == "compgcn" else "DMPNN"
    cfg = config(rep_net, nel)
    torch.manual_seed(21)
    composed = a.impl == "composed"
    if a.layer:
        H = cfg["hid_dim"]
        layer = (si.CompGCNLayer(H, H, comp_opt=a.comp_opt, edge_norm="none", act_func="leaky_relu") if a.model == "compgcn"
                 else si.DMPLayer(H, H, batch_norm=False, act_func="leaky_relu")).to(DEV).to(dtype)
        x = torch.randn(gg.number_of_nodes(), H, device=DEV).to(dtype)
        ef = torch.randn(gg.number_of_edges(), H, device=DEV).to(dtype)

        def step():
            layer.zero_grad(set_to_none=True)
            xx, ee = x.clone().requires_grad_(True), ef.clone().requires_grad_(True)
            no, eo = layer(gg, xx, ee)
            (no.float().sum() + eo.float().sum()).backward()
    else:
        model = perturb(ComposedModel(cfg) if composed else {"CompGCN": si.CompGCN, "DMPNN": si.DMPNN}[rep_net](**cfg))
        model = model.to(DEV).to(dtype).train()
        coef = (torch.arange(1, 513, dtype=torch.float32, device=DEV) / 512).view(-1, 1)

        def step():
            model.zero_grad(set_to_none=True)
            res = model(pg, gg)
            (res["pred_c"].float() * coef).sum().backward()

    def run(fn):
        with _layer_path(bool(a.fused) and not composed):
            return fn()

    times = run(lambda: timed(step, a.steps, a.warmup))
    out = dict(tool="si_dual_model_bench", model=a.model, impl=a.impl, fused=bool(a.fused) and not composed, dtype=a.dtype, layer=bool(a.layer),
               comp_opt=a.comp_opt if a.model == "compgcn" else None, nodes=gg.number_of_nodes(), edges=gg.number_of_edges(),
               steps=a.steps, median_ms=statistics.median(times), min_ms=min(times), max_ms=max(times))
    if a.tags:
        with ops.KernelTimer() as timer:
            run(step)
        out["tags"] = {k: v[0] for k, v in timer.summary().items()}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", choices=["compgcn", "dmpnn"], default="dmpnn")
    ap.add_argument("--impl", choices=["model", "composed"], default="model")
    ap.add_argument("--dtype", choices=["fp32", "bf16"], default="fp32")
    ap.add_argument("--layer", action="store_true")
    ap.add_argument("--comp-opt", choices=["mult", "sub"], default="mult")
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--fused", action="store_true", help="with --impl model: the layers under ops.dual_fused()")
    ap.add_argument("--tags", action="store_true", help="also count the kernel-timer tags of one warm step")
    ap.add_argument("--suite", action="store_true",
                    help="one process, one JSON line each (--model / --dtype / --layer / --fused are set per run): both models in "
                         "fp32, the DMP layer and the CompGCN layer with mult and sub; for --impl model also both models and the "
                         "three layers under ops.dual_fused(), and both models in bf16")
    a = ap.parse_args()
    pa, ga, nel = scale_batches()
    batches = (graph_of(pa), graph_of(ga), nel)
    if not a.suite:
        print(json.dumps(run_one(a, batches)))
        return
    runs = [dict(model="dmpnn"), dict(model="compgcn"), dict(model="dmpnn", layer=True),
            dict(model="compgcn", layer=True, comp_opt="mult"), dict(model="compgcn", layer=True, comp_opt="sub")]
    if a.impl == "model":
        runs += [dict(kw, fused=True) for kw in runs] + [dict(model="dmpnn", dtype="bf16"), dict(model="compgcn", dtype="bf16")]
    for kw in runs:
        b = argparse.Namespace(**dict(vars(a), layer=False, dtype="fp32", fused=False))
        for k, v in kw.items():
            setattr(b, k, v)
        print(json.dumps(run_one(b, batches)), flush=True)


if __name__ == "__main__":
    main()
