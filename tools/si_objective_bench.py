"""The SI training objective on the scale batch of tools/si_full_model_bench.py (512 pairs, config-3 graphs with dummy nodes: 25,600
graph nodes, H = 64, node weights present): ops.si_objective on the kernels (dn_objective.hip) against the composed path (the
reference's torch ops), the two ALTERNATED in one process -- --rounds rounds of --steps steps each after --warmup warm-up steps per
path and round.  Eager, fp32, synchronised host clock.

  objective   SIObjective forward + backward on the RGIN model's own outputs as leaves (pred_c, pred_v, both representations)
  model       the whole RGIN step (pred_return_weights="node"): forward, SIObjective, backward, SITrainMeter.update

Prints one JSON line per (what, round, path) with the step's launches (the package's tagged launch groups, and every device kernel
torch's profiler sees in one step, where the profiler works), and a summary line per workload: the median over all steps of each
path, the spread of the per-round medians (max - min) / median, and whether EVERY fused round was faster than EVERY composed round
(the project's rule for ops.SI_OBJECTIVE_FUSED_DEFAULT)."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import si_dual_model_bench as B  # noqa: E402  (perturb, timed)
import si_full_model_bench as F  # noqa: E402  (batches, CFG)
from dummynode4graphlearning_amd import ops  # noqa: E402
from dummynode4graphlearning_amd import subgraph_isomorphism as si  # noqa: E402

DEV = B.DEV


def device_kernels(step):
    """The device kernels of one step as torch's profiler counts them (None where it cannot)."""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            step()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA"))
        return n or None
    except Exception:
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--what", default="objective,model")
    ap.add_argument("--profile", action="store_true", help="also count the device kernels of a step with torch's profiler")
    a = ap.parse_args()
    pg, gg = F.batches()
    cfg = dict(F.CFG, pred_return_weights="node")
    torch.manual_seed(21)
    model = B.perturb(si.RGIN(**cfg)).to(DEV).train()
    pairs = pg.batch_size
    gen = torch.Generator().manual_seed(3)
    counts = torch.randint(0, 5, (pairs,), generator=gen).to(DEV)
    obj = si.SIObjective(total_steps=1000)                                     # the reference's defaults: every term on
    out0 = model(pg, gg)
    node_weights = torch.randint(0, 3, tuple(out0["pred_v"].shape), generator=gen).float().to(DEV)
    print(json.dumps(dict(tool="si_objective_bench", what="batch", pairs=pairs, graph_nodes=gg.number_of_nodes(),
                          pattern_nodes=pg.number_of_nodes(), H=cfg["hid_dim"], L_v=int(out0["pred_v"].shape[1]),
                          scalars=obj.scalars(100))), flush=True)
    leaves = {k: (v.detach().clone().requires_grad_(True) if v is not None and v.dtype.is_floating_point else v) for k, v in out0.items()}
    meter = si.SITrainMeter()

    def objective_step():
        for v in leaves.values():
            if v is not None and v.dtype.is_floating_point:
                v.grad = None
        loss, _ = obj(leaves, counts, node_weights, None, step=100, model=model)
        loss.backward()

    def model_step():
        model.zero_grad(set_to_none=True)
        loss, terms = obj(model(pg, gg), counts, node_weights, None, step=100, model=model)
        loss.backward()
        meter.update(terms, pairs)

    tags = ("si_objective_fwd", "si_objective_bwd", "si_objective_composed")
    for what, step in (("objective", objective_step), ("model", model_step)):
        if what not in a.what.split(","):
            continue
        all_times, round_medians = {"fused": [], "composed": []}, {"fused": [], "composed": []}
        for rnd in range(a.rounds):
            for impl in ("fused", "composed"):
                with ops.objective_fused(impl == "fused"):
                    times = B.timed(step, a.steps, a.warmup)
                    with ops.KernelTimer() as timer:
                        step()
                    summ = timer.summary()
                    kernels = device_kernels(step) if a.profile and rnd == 0 else None
                all_times[impl] += times
                round_medians[impl].append(statistics.median(times))
                print(json.dumps(dict(tool="si_objective_bench", what=what, impl=impl, round=rnd, steps=a.steps,
                                      median_ms=statistics.median(times), min_ms=min(times), max_ms=max(times),
                                      tagged={t: [summ[t][0], round(summ[t][1], 3)] for t in tags if t in summ},
                                      device_kernels_per_step=kernels)), flush=True)
        med = {i: statistics.median(all_times[i]) for i in all_times}
        spread = {i: (max(round_medians[i]) - min(round_medians[i])) / med[i] for i in all_times}
        print(json.dumps(dict(tool="si_objective_bench", what=what + "_summary", rounds=a.rounds, steps=a.steps, median_ms=med,
                              round_spread=spread, fused_over_composed=med["fused"] / med["composed"],
                              every_fused_round_faster=max(round_medians["fused"]) < min(round_medians["composed"]))), flush=True)


if __name__ == "__main__":
    main()
