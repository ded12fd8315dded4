"""3-WL graph kernels (graph_kernels_k3wl.py) on one seeded synthetic dataset with the GC dummy node, node labels, H = 2:

  --shape mutag   MUTAG-shaped graphs: 188 of 10..28 nodes (a random tree plus ring-closing edges, about 1.1 edges per node, 7 node
                  labels), each with a dummy node joined to every other node
  --shape forty   16 graphs of 36..44 nodes built the same way (about 70,000 triples each), with the dummy node

Times, with a synchronised host clock around device work, per --kernel (default: all four):
  refine     k3wl_colors (the initial colours and H refinement steps over the whole dataset), the fused kernels (dn_k3wl_*) against the
             composed path (torch device ops, a device-wide segmented sort, dn_wl_fold_u64), ALTERNATED in one process: --rounds
             rounds of --steps calls each after --warmup warm-up calls per path and round;
  features   k3wl_features (one-off per dataset, torch device ops) once per round;
  gram       dn_wl_gram_i64, all H + 1 matrices in one launch.

Prints one JSON line per (kernel, round, what) and a summary line per kernel: the median over all calls of each path, the spread of
the per-round medians (max - min) / median, and fused / composed.  The two paths' colours are compared once (they must be equal)."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from graph_kernel_bench import DEV, timed  # noqa: E402
from dummynode4graphlearning_amd import graph_kernels as gk, graph_kernels_k3wl as kk, ops  # noqa: E402


def dataset(shape, graphs, seed):
    rng = np.random.default_rng(seed)
    lo, hi = (10, 29) if shape == "mutag" else (36, 45)
    gi, src, dst, labels, off = [], [], [], [], 0
    for g in range(1, graphs + 1):
        n = int(rng.integers(lo, hi))
        a, b = np.arange(1, n), (rng.random(n - 1) * np.arange(1, n)).astype(np.int64)          # a random tree ...
        extra = max(1, n // 8)
        x, y = rng.integers(0, n, extra), rng.integers(0, n, extra)                              # ... a few ring-closing edges ...
        keep = x != y
        a, b = np.concatenate([a, x[keep], np.arange(n)]), np.concatenate([b, y[keep], np.full(n, n)])     # ... and the dummy node n
        src.append(np.concatenate([a, b]) + off + 1)
        dst.append(np.concatenate([b, a]) + off + 1)
        labels.append(np.concatenate([rng.integers(1, 8, n), [0]]))
        gi.append(np.full(n + 1, g))
        off += n + 1
    return gk.GraphKernelData.from_arrays(np.concatenate(gi), np.stack([np.concatenate(src), np.concatenate(dst)], 1),
                                          np.concatenate(labels), None, [0] * graphs, device=DEV,
                                          source="synthetic %s-shaped, seed %d" % (shape, seed))


def _colors(data, H, kernel, fused):
    with ops.k3wl_fused(fused):
        return kk.k3wl_colors(data, H, kernel, True, False)[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=["mutag", "forty"], default="mutag")
    ap.add_argument("--kernel", choices=kk.KERNELS, action="append")
    ap.add_argument("--graphs", type=int, default=0, help="default: 188 (mutag), 16 (forty)")
    ap.add_argument("--iters", type=int, default=2)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    data = dataset(a.shape, a.graphs or (188 if a.shape == "mutag" else 16), a.seed)
    H = a.iters
    for kernel in a.kernel or kk.KERNELS:
        p = kk._plan(data, kernel)
        shape = dict(tool="graph_kernel_k3wl_bench", shape=a.shape, kernel=kernel, graphs=data.num_graphs, nodes=data.num_nodes,
                     largest_graph=data.max_nodes, items=p.num_tuples, H=H, graphs_composed=int((~p.fused_graph).sum()),
                     composed_entries_per_step=int(p._phys.sum()))
        cf, cc = _colors(data, H, kernel, True), _colors(data, H, kernel, False)
        assert torch.equal(cf, cc), "fused and composed colours differ"
        feats = kk.k3wl_features(data, H, kernel, True, False, colors=cf)
        shape.update(feature_entries=int(feats.color.numel()), longest_row=feats.max_row)
        print(json.dumps(dict(shape, what="shape")), flush=True)
        whats = {"refine_fused": lambda: _colors(data, H, kernel, True), "refine_composed": lambda: _colors(data, H, kernel, False),
                 "features": lambda: kk.k3wl_features(data, H, kernel, True, False, colors=cf),
                 "gram": lambda: kk.k3wl_gram_matrices(data, H, kernel, True, False, features=feats)}
        all_times, round_medians = {w: [] for w in whats}, {w: [] for w in whats}
        for rnd in range(a.rounds):
            for w, fn in whats.items():
                few = w in ("gram", "features")
                times = timed(fn, max(2, a.steps // 3) if few else a.steps, 1 if few else a.warmup)
                all_times[w] += times
                round_medians[w].append(statistics.median(times))
                print(json.dumps(dict(tool="graph_kernel_k3wl_bench", kernel=kernel, what=w, round=rnd, calls=len(times),
                                      median_ms=statistics.median(times), min_ms=min(times), max_ms=max(times))), flush=True)
        med = {w: statistics.median(t) for w, t in all_times.items()}
        spread = {w: (max(round_medians[w]) - min(round_medians[w])) / med[w] for w in whats}
        print(json.dumps(dict(shape, what="summary", rounds=a.rounds, median_ms={w: round(v, 4) for w, v in med.items()},
                              round_spread={w: round(v, 4) for w, v in spread.items()},
                              fused_over_composed=round(med["refine_fused"] / med["refine_composed"], 4))), flush=True)
        del cf, cc, feats
        data.__dict__.pop("_k3wl_plans", None)                               # (one kernel's arrays at a time)


if __name__ == "__main__":
    main()
