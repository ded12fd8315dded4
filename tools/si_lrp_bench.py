"""LRP on a config-3-shaped batch with dummy nodes (tools/si_dual_model_bench.py's scale batch: reversed and dummy edges,
H = 64): one LRPLayer forward + backward, fused (dn_lrp_pool_*) against composed (gather_segsum over the materialised index +
dn_segment_mean), and the index build times.  Eager, synchronised, median of --steps steps after --warmup warm-ups.

  --impl fused | composed   one path
  --impl both               the two paths ALTERNATED in one process (--rounds rounds of --steps steps each), one JSON line each
  --index                   also time the ego-net index build and the materialised index build (fresh batch objects, --steps times)
  --model                   time LRP(**cfg) forward + backward (patterns + graphs) instead of the layer alone

Prints one JSON line per measurement."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import si_dual_model_bench as B  # noqa: E402  (graph_of, config, perturb, timed)
from dummynode4graphlearning_amd import ops, synthetic, transforms  # noqa: E402
from dummynode4graphlearning_amd import subgraph_isomorphism as si  # noqa: E402
from dummynode4graphlearning_amd.subgraph_isomorphism import bookkeeping  # noqa: E402

DEV = B.DEV


def _no_self_loops(b):
    """The ego-net sequences are undefined on a self-loop (the index build refuses it): u -> u becomes u -> the next node of
    its graph."""
    node_ptr, src, dst = (np.asarray(b[k], np.int64) for k in ("node_ptr", "src", "dst"))
    g = np.searchsorted(node_ptr, src, side="right") - 1
    base, n = node_ptr[g], node_ptr[g + 1] - node_ptr[g]
    b["dst"] = np.where(src == dst, base + (dst - base + 1) % n, dst)
    return b


def scale_batches(seed=0, graphs=512):
    """si_dual_model_bench.scale_batches (config-3 graphs of 49 real nodes and seeded patterns of 3-9 real nodes, both with
    reversed edges and a dummy node) without self-loops, the first `graphs` graphs of each."""
    raw = synthetic.config3(graphs=graphs)
    vocab = (raw["max_nv"], raw["max_nvl"], raw["max_ne"], raw["max_nel"])
    rng = np.random.default_rng(seed)
    n = rng.integers(3, 10, size=graphs)
    m = np.array([int(rng.integers(k, 2 * k + 1)) for k in n])
    node_ptr, edge_ptr = np.concatenate([[0], np.cumsum(n)]), np.concatenate([[0], np.cumsum(m)])
    src = np.concatenate([rng.integers(0, k, size=e) + o for k, e, o in zip(n, m, node_ptr[:-1])])
    dst = np.concatenate([rng.integers(0, k, size=e) + o for k, e, o in zip(n, m, node_ptr[:-1])])
    pat = dict(node_ptr=node_ptr, edge_ptr=edge_ptr, src=src, dst=dst, node_id=np.concatenate([np.arange(k) for k in n]),
               node_label=rng.integers(0, raw["max_nvl"], size=int(n.sum())), edge_id=np.concatenate([np.arange(e) for e in m]),
               edge_label=rng.integers(0, raw["max_nel"], size=int(m.sum())))
    out, nel = [], 0
    for b in (_no_self_loops(pat), _no_self_loops(raw)):
        t = {k: torch.from_numpy(np.asarray(b[k], np.int64)).to(DEV) for k in
             ("node_ptr", "edge_ptr", "src", "dst", "node_id", "node_label", "edge_id", "edge_label")}
        r = bookkeeping.add_reversed_edges(t["edge_ptr"], t["src"], t["dst"], t["edge_id"], t["edge_label"], vocab[2], vocab[3])
        aug = transforms.dummy_augment_si(t["node_ptr"], r["edge_ptr"], r["src"], r["dst"], t["node_id"], t["node_label"], r["edge_id"],
                                          r["edge_label"], vocab[0], vocab[1], 2 * vocab[2], 2 * vocab[3], is_reversed=r["is_reversed"])
        nel = max(nel, int(aug["edge_label"].max()) + 1)
        out.append(aug)
    return out[0], out[1], nel


def _path(impl):
    return ops.lrp_fused() if impl == "fused" else ops.lrp_composed()


def _sync_time(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


def index_times(aug, L, steps):
    """Median build times over fresh batch objects; the materialised index only when its P * L * L entries fit int32."""
    ego, mat = [], []
    for _ in range(steps + 1):
        g = B.graph_of(aug)
        g.node_ptr()
        t, ix = _sync_time(lambda: g.lrp_index(L))
        ego.append(t)
        if materialisable(ix):
            mat.append(_sync_time(ix.perm_index)[0])
    return dict(tool="si_lrp_bench", what="index", seq_len=L, nodes=g.number_of_nodes(), edges=g.number_of_edges(),
                sequences=int(ix.count.sum()), max_sequences_per_node=int(ix.count.max()),
                max_neighbours=int((ix.uptr[1:] - ix.uptr[:-1]).max()), steps=steps,
                ego_index_median_ms=statistics.median(ego[1:]), perm_index_median_ms=statistics.median(mat[1:]) if mat else None)


def materialisable(ix):
    return int(ix.count.sum()) * ix.seq_len * ix.seq_len < 2 ** 31


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--impl", choices=["fused", "composed", "both"], default="both")
    ap.add_argument("--seq-len", type=int, default=4)
    ap.add_argument("--graphs", type=int, default=512, help="graphs of the batch")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--index", action="store_true")
    ap.add_argument("--model", action="store_true")
    a = ap.parse_args()
    L = a.seq_len
    pa, ga, nel = scale_batches(graphs=a.graphs)
    pg, gg = B.graph_of(pa), B.graph_of(ga)
    if a.index:
        print(json.dumps(index_times(ga, L, a.steps)), flush=True)
    cfg = dict(B.config("LRP", nel), lrp_seq_len=L, rep_lrp_batch_norm=False)
    H = cfg["hid_dim"]
    torch.manual_seed(21)
    if a.model:
        model = B.perturb(si.LRP(**cfg)).to(DEV).train()
        coef = (torch.arange(1, a.graphs + 1, dtype=torch.float32, device=DEV) / a.graphs).view(-1, 1)

        def step():
            model.zero_grad(set_to_none=True)
            res = model(pg, gg)
            (res["pred_c"].float() * coef).sum().backward()
    else:
        layer = si.LRPLayer(H, H, lrp_seq_len=L, act_func="leaky_relu").to(DEV)
        x = torch.randn(gg.number_of_nodes(), H, device=DEV)
        ef = torch.randn(gg.number_of_edges(), H, device=DEV)

        def step():
            layer.zero_grad(set_to_none=True)
            xx, ee = x.clone().requires_grad_(True), ef.clone().requires_grad_(True)
            no, _ = layer(gg, xx, ee)
            no.sum().backward()

    impls = ["fused", "composed"] if a.impl == "both" else [a.impl]
    if "composed" in impls and not all(materialisable(g.lrp_index(L)) for g in ((pg, gg) if a.model else (gg,))):
        print(json.dumps(dict(tool="si_lrp_bench", what="skip", impl="composed", reason="the materialised index does not fit int32")))
        impls.remove("composed")
    for rnd in range(a.rounds if a.impl == "both" else 1):
        for impl in impls:
            with _path(impl):
                times = B.timed(step, a.steps, a.warmup)
                with ops.KernelTimer() as timer:
                    step()
                tags = {k: round(v[1], 3) for k, v in timer.summary().items() if k.startswith(("lrp_", "gather_segsum"))}
            print(json.dumps(dict(tool="si_lrp_bench", what="model" if a.model else "layer", impl=impl, round=rnd, seq_len=L, H=H,
                                  nodes=gg.number_of_nodes(), edges=gg.number_of_edges(), steps=a.steps,
                                  median_ms=statistics.median(times), min_ms=min(times), max_ms=max(times), kernel_ms=tags)),
                  flush=True)


if __name__ == "__main__":
    main()
