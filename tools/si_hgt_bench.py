"""HGT on a config-3-shaped batch with dummy nodes (tools/si_dual_model_bench.py's scale batch: reversed and dummy edges, H = 64):
one HeteroGraphTransLayer forward + backward, or a whole HGT(**cfg) step, with the attention on the fused kernels (dn_hgt.hip)
against the composed path (torch scatter ops over the same factorisation; it is built only from ops the tree had before the
kernels, so it is the speed of the model without them).  Eager, synchronised host clock, the two paths ALTERNATED in one process:
--rounds rounds of --steps steps each, after --warmup warm-up steps per path and round.

  --impl fused | composed | both
  --model          time HGT(**cfg) forward + backward (patterns + graphs) instead of the layer alone
  --heads / --regularizer / --num-bases   the layer's attention heads and node-type weights (default: the model's defaults)

Prints one JSON line per (round, path) and, for --impl both, a summary line: the median over all steps of each path, the spread of
the per-round medians (max - min) / median, and fused / composed."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import si_dual_model_bench as B  # noqa: E402  (scale_batches, graph_of, config, perturb, timed)
from dummynode4graphlearning_amd import ops  # noqa: E402
from dummynode4graphlearning_amd import subgraph_isomorphism as si  # noqa: E402

DEV = B.DEV
TAGS = ("hgt_", "rows_gemm", "gather_segsum")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--impl", choices=["fused", "composed", "both"], default="both")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--model", action="store_true")
    ap.add_argument("--heads", type=int, default=4)
    ap.add_argument("--regularizer", default="diag")
    ap.add_argument("--num-bases", type=int, default=-1)
    a = ap.parse_args()
    pa, ga, nel = B.scale_batches()
    pg, gg = B.graph_of(pa), B.graph_of(ga)
    cfg = dict(B.config("HGT", nel), rep_hgt_num_heads=a.heads, rep_hgt_regularizer=a.regularizer, rep_hgt_num_bases=a.num_bases)
    H = cfg["hid_dim"]
    torch.manual_seed(21)
    if a.model:
        model = B.perturb(si.HGT(**cfg)).to(DEV).train()
        graphs = pg.batch_size
        coef = (torch.arange(1, graphs + 1, dtype=torch.float32, device=DEV) / graphs).view(-1, 1)

        def step():
            model.zero_grad(set_to_none=True)
            res = model(pg, gg)
            (res["pred_c"].float() * coef).sum().backward()
    else:
        layer = si.HeteroGraphTransLayer(H, H, num_node_types=cfg["max_ngvl"], num_edge_types=nel, regularizer=a.regularizer,
                                         num_bases=a.num_bases, num_heads=a.heads, act_func="leaky_relu").to(DEV)
        x = torch.randn(gg.number_of_nodes(), H, device=DEV)

        def step():
            layer.zero_grad(set_to_none=True)
            xx = x.clone().requires_grad_(True)
            layer(gg, xx).sum().backward()

    impls = ["fused", "composed"] if a.impl == "both" else [a.impl]
    what = "model" if a.model else "layer"
    pairs = gg.hgt_index(gg.edata["label"], nel).num_pairs              # (destination, edge type) pairs of the graph batch
    all_times, round_medians = {i: [] for i in impls}, {i: [] for i in impls}
    for rnd in range(a.rounds if a.impl == "both" else 1):
        for impl in impls:
            with ops.hgt_fused(impl == "fused"):
                times = B.timed(step, a.steps, a.warmup)
                with ops.KernelTimer() as timer:
                    step()
                tags = {k: round(v[1], 3) for k, v in timer.summary().items() if k.startswith(TAGS)}
            all_times[impl] += times
            round_medians[impl].append(statistics.median(times))
            print(json.dumps(dict(tool="si_hgt_bench", what=what, impl=impl, round=rnd, H=H, heads=a.heads, relations=nel,
                                  nodes=gg.number_of_nodes(), edges=gg.number_of_edges(), pairs=pairs, steps=a.steps,
                                  median_ms=statistics.median(times), min_ms=min(times), max_ms=max(times), kernel_ms=tags)), flush=True)
    if a.impl == "both":
        med = {i: statistics.median(all_times[i]) for i in impls}
        spread = {i: (max(round_medians[i]) - min(round_medians[i])) / med[i] for i in impls}
        print(json.dumps(dict(tool="si_hgt_bench", what=what + "_summary", H=H, heads=a.heads, relations=nel, rounds=a.rounds,
                              steps=a.steps, fused_median_ms=med["fused"], composed_median_ms=med["composed"],
                              fused_round_spread=spread["fused"], composed_round_spread=spread["composed"],
                              fused_over_composed=med["fused"] / med["composed"])), flush=True)


if __name__ == "__main__":
    main()
