"""CNN on the config-3-shaped batch of tools/si_dual_model_bench.py (512 pairs with dummy nodes and reversed edges, H = 64) turned
into edge sequences: one CNNLayer forward + backward on the graph sequences, or a whole CNN(**cfg) step, with the filter, the
embedding and the layers on the fused kernels (dn_eseq.hip, ops.si_embed) against the composed path (torch ops on rows layout).
Eager, synchronised host clock, the two paths ALTERNATED in one process: --rounds rounds of --steps steps each, after --warmup warm-up
steps per path and round.

  --impl fused | composed | both
  --model          time CNN(**cfg) forward + backward (patterns + graphs) instead of the layer alone
  --k              kernel size(s), comma separated (default 2,3; padding k // 2, no BatchNorm, 3 layers, leaky_relu)

Prints one JSON line per (k, round, path) with the kernel launches of a step by tag (count, ms) and, for the model, the shares of
embedding, filter, mask / refine and head in the step's tagged time; and for --impl both a summary line per k: the median over all
steps of each path, the spread of the per-round medians (max - min) / median, fused / composed, and whether EVERY fused round was
faster than EVERY composed round (the project's rule for a default).  The batch line gives the share of padded positions."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import si_dual_model_bench as B  # noqa: E402  (scale_batches, graph_of, config, perturb, timed)
from dummynode4graphlearning_amd import EdgeSeq, ops  # noqa: E402
from dummynode4graphlearning_amd import subgraph_isomorphism as si  # noqa: E402

DEV = B.DEV
SHARES = {"embedding": "eseq_embed", "filter": "eseq_filter", "mask_refine": "eseq_mask_refine", "head": "si_head_padded"}
KERNELS = ("eseq_conv_pool_fwd", "eseq_dconv", "eseq_dgrad", "eseq_wgrad", "eseq_wgrad_combine", "eseq_filter_gate", "si_embed",
           "si_embed_wgrad", "eseq_layer_composed")


def padded_share(seq):
    return 1.0 - seq.number_of_tuples() / float(seq.u.numel())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--impl", choices=["fused", "composed", "both"], default="both")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--model", action="store_true")
    ap.add_argument("--k", default="2,3")
    a = ap.parse_args()
    pa, ga, nel = B.scale_batches()
    ps, gs = EdgeSeq.from_graph(B.graph_of(pa)), EdgeSeq.from_graph(B.graph_of(ga))
    print(json.dumps(dict(tool="si_cnn_bench", what="batch", pairs=gs.batch_size, pattern_L=int(ps.u.shape[1]), graph_L=int(gs.u.shape[1]),
                          pattern_tuples=ps.number_of_tuples(), graph_tuples=gs.number_of_tuples(),
                          pattern_padded_share=round(padded_share(ps), 4), graph_padded_share=round(padded_share(gs), 4))), flush=True)
    impls = ["fused", "composed"] if a.impl == "both" else [a.impl]
    what = "model" if a.model else "layer"
    for k in (int(v) for v in a.k.split(",")):
        cfg = dict(B.config("CNN", nel), rep_cnn_kernel_sizes=k, rep_cnn_paddings=-1, rep_cnn_strides=1, rep_cnn_batch_norm=False)
        H = cfg["hid_dim"]
        torch.manual_seed(21)
        if a.model:
            model = B.perturb(si.CNN(**cfg)).to(DEV).train()
            coef = (torch.arange(1, gs.batch_size + 1, dtype=torch.float32, device=DEV) / gs.batch_size).view(-1, 1)

            def step():
                model.zero_grad(set_to_none=True)
                (model(ps, gs)["pred_c"].float() * coef).sum().backward()
        else:
            layer = si.CNNLayer(H, H, kernel_size=k, batch_norm=False, act_func="leaky_relu").to(DEV)
            Bn, L = gs.u.shape
            x = torch.randn(Bn, L, H, device=DEV)
            gate = si.edge_seq.len_mask(gs.lens, L, DEV).float()

            def step():
                layer.zero_grad(set_to_none=True)
                xx = x.clone().requires_grad_(True)
                y, _ = ops.eseq_conv_pool(xx, gs.lens, layer.conv.weight, layer.conv.bias, gate, k // 2, "leaky_relu", True) \
                    if ops.eseq_fused_enabled() else ops.launch_tagged("eseq_layer_composed", lambda: ops.eseq_conv_pool_composed(
                        xx, layer.conv.weight, layer.conv.bias, gate, k // 2, "leaky_relu", k % 2 == 1))
                y.sum().backward()

        all_times, round_medians = {i: [] for i in impls}, {i: [] for i in impls}
        for rnd in range(a.rounds if a.impl == "both" else 1):
            for impl in impls:
                with ops.eseq_fused(impl == "fused"):
                    times = B.timed(step, a.steps, a.warmup)
                    with ops.KernelTimer() as timer:
                        step()
                    summ = timer.summary()
                launches = {t: [v[0], round(v[1], 3)] for t, v in summ.items() if t in KERNELS}
                line = dict(tool="si_cnn_bench", what=what, impl=impl, k=k, round=rnd, H=H, steps=a.steps,
                            median_ms=statistics.median(times), min_ms=min(times), max_ms=max(times), launches=launches)
                if a.model:
                    line["tagged_ms"] = {name: round(summ.get(tag, (0, 0.0))[1], 3) for name, tag in SHARES.items()}
                    line["share_of_step"] = {name: round(summ.get(tag, (0, 0.0))[1] / line["median_ms"], 3) for name, tag in SHARES.items()}
                all_times[impl] += times
                round_medians[impl].append(statistics.median(times))
                print(json.dumps(line), flush=True)
        if a.impl == "both":
            med = {i: statistics.median(all_times[i]) for i in impls}
            spread = {i: (max(round_medians[i]) - min(round_medians[i])) / med[i] for i in impls}
            print(json.dumps(dict(tool="si_cnn_bench", what=what + "_summary", k=k, H=H, rounds=a.rounds, steps=a.steps,
                                  fused_median_ms=med["fused"], composed_median_ms=med["composed"],
                                  fused_round_spread=spread["fused"], composed_round_spread=spread["composed"],
                                  fused_over_composed=med["fused"] / med["composed"],
                                  every_fused_round_faster=max(round_medians["fused"]) < min(round_medians["composed"]))), flush=True)


if __name__ == "__main__":
    main()
