"""TransformerXL on the scale batch of tools/si_cnn_bench.py (512 pairs with dummy nodes and reversed edges, H = 64, turned into edge
sequences; graph sequences of 302 tuples, so 5 segments of 64): one TXLLayer forward + backward over the graph sequences, or a whole
TransformerXL(**cfg) step (3 layers), with the attention on the fused kernels (dn_txl.hip, whole sequence at once) against the
composed path (the reference's segment loop in torch ops).  Eager, fp32, synchronised host clock, the two paths ALTERNATED in one
process: --rounds rounds of --steps steps each, after --warmup warm-up steps per path and round.

  --impl fused | composed | all        (all: the two, alternated)
  --model          time TransformerXL(**cfg) forward + backward (patterns + graphs) instead of the layer alone
  --heads          1,4 (comma separated): the defaults and num_heads=4

Prints one JSON line per (heads, round, path) with the tagged launch groups of a step (count, ms) and the share of the step spent
outside ops.txl_attention (fused path: 1 - (txl_attn_fwd + txl_attn_bwd) / the tagged step), and for --impl all a summary line per
setting: the median over all steps of each path, the spread of the per-round medians (max - min) / median, and whether EVERY fused
round was faster than EVERY composed round (the project's rule for a default)."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import si_dual_model_bench as B  # noqa: E402  (scale_batches, graph_of, config, perturb, timed)
from dummynode4graphlearning_amd import EdgeSeq, ops  # noqa: E402
from dummynode4graphlearning_amd import subgraph_isomorphism as si  # noqa: E402

DEV = B.DEV
KERNELS = ("txl_proj", "txl_attn_fwd", "txl_attn_bwd", "txl_close", "txl_ff", "txl_composed", "eseq_filter_gate", "si_embed",
           "si_embed_wgrad")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--impl", choices=["fused", "composed", "all"], default="all")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--model", action="store_true")
    ap.add_argument("--heads", default="1,4")
    a = ap.parse_args()
    pa, ga, nel = B.scale_batches()
    ps, gs = EdgeSeq.from_graph(B.graph_of(pa)), EdgeSeq.from_graph(B.graph_of(ga))
    print(json.dumps(dict(tool="si_txl_bench", what="batch", pairs=gs.batch_size, pattern_L=int(ps.u.shape[1]), graph_L=int(gs.u.shape[1]),
                          pattern_tuples=ps.number_of_tuples(), graph_tuples=gs.number_of_tuples(),
                          segments=-(-int(gs.u.shape[1]) // 64))), flush=True)
    impls = ["fused", "composed"] if a.impl == "all" else [a.impl]
    what = "model" if a.model else "layer"
    for heads in (int(h) for h in a.heads.split(",")):
        cfg = dict(B.config("TXL", nel), num_heads=heads, rep_act_func="relu")
        H = cfg["hid_dim"]
        torch.manual_seed(21)
        if a.model:
            model = B.perturb(si.TransformerXL(**cfg)).to(DEV).train()
            coef = (torch.arange(1, gs.batch_size + 1, dtype=torch.float32, device=DEV) / gs.batch_size).view(-1, 1)

            def step():
                model.zero_grad(set_to_none=True)
                (model(ps, gs)["pred_c"].float() * coef).sum().backward()
        else:
            model = B.perturb(si.TransformerXL(**dict(cfg, rep_num_graph_layers=1, rep_num_pattern_layers=1))).to(DEV).train()
            Bn, L = gs.u.shape
            x = torch.randn(Bn, L, H, device=DEV)
            mask = si.edge_seq.len_mask(gs.lens, L, DEV).view(Bn, L, 1)
            c = torch.randn(Bn, L, H, device=DEV)

            def step():
                model.zero_grad(set_to_none=True)
                xx = x.clone().requires_grad_(True)
                (model.get_graph_rep(xx, mask=mask) * c).sum().backward()

        all_times, round_medians = {i: [] for i in impls}, {i: [] for i in impls}
        for rnd in range(a.rounds if a.impl == "all" else 1):
            for impl in impls:
                with ops.eseq_fused(impl == "fused"):
                    times = B.timed(step, a.steps, a.warmup)
                    with ops.KernelTimer() as timer:
                        t0 = time.perf_counter()
                        step()
                        torch.cuda.synchronize()
                        tagged_ms = (time.perf_counter() - t0) * 1e3
                    summ = timer.summary()
                launches = {t: [v[0], round(v[1], 3)] for t, v in summ.items() if t in KERNELS}
                attn = sum(summ[t][1] for t in ("txl_attn_fwd", "txl_attn_bwd") if t in summ)
                all_times[impl] += times
                round_medians[impl].append(statistics.median(times))
                print(json.dumps(dict(tool="si_txl_bench", what=what, impl=impl, heads=heads, round=rnd, H=H, steps=a.steps,
                                      median_ms=statistics.median(times), min_ms=min(times), max_ms=max(times), launches=launches,
                                      tagged_step_ms=round(tagged_ms, 3),
                                      share_outside_attention=round(1 - attn / tagged_ms, 3) if impl == "fused" else None)), flush=True)
        if a.impl == "all":
            med = {i: statistics.median(all_times[i]) for i in impls}
            spread = {i: (max(round_medians[i]) - min(round_medians[i])) / med[i] for i in impls}
            print(json.dumps(dict(tool="si_txl_bench", what=what + "_summary", heads=heads, H=H, rounds=a.rounds, steps=a.steps,
                                  median_ms=med, round_spread=spread, fused_over_composed=med["fused"] / med["composed"],
                                  every_fused_round_faster=max(round_medians["fused"]) < min(round_medians["composed"]))), flush=True)


if __name__ == "__main__":
    main()
