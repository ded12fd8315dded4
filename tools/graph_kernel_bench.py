"""WL / WLOA graph kernels on one seeded synthetic dataset: NCI1-shaped graphs (10..50 nodes, a random tree plus a few ring-closing
edges, 37 skewed node labels) with the GC dummy node (label 0, joined to every node of its graph), node labels, H = 5.

Times, with a synchronised host clock around device work:
  refine     wl_colors (H refinement steps over the whole dataset), the fused kernels (dn_wl_refine_u64) against the composed path (a
             device-wide segmented sort with torch ops, then dn_wl_fold_u64), ALTERNATED in one process: --rounds rounds of --steps
             calls each after --warmup warm-up calls per path and round;
  features   wl_features (one-off per dataset, torch device ops) once per round;
  gram       dn_wl_gram_i64, all H + 1 matrices of --graphs x --graphs in one launch, WL and WLOA.

Prints one JSON line per (round, what) and a summary line: the median over all calls of each path, the spread of the per-round
medians (max - min) / median, and fused / composed.  The two refinement paths' colours are compared once (they must be equal)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dummynode4graphlearning_amd import graph_kernels as gk, ops  # noqa: E402

DEV = "cuda:0"


def dataset(graphs, seed, edge_labels):
    rng = np.random.default_rng(seed)
    gi, src, dst, labels, off = [], [], [], [], 0
    weights = 1.0 / np.arange(1, 38)
    weights /= weights.sum()
    for g in range(1, graphs + 1):
        n = int(rng.integers(10, 51))
        parent = (rng.random(n - 1) * np.arange(1, n)).astype(np.int64)             # a random tree: node v joins an earlier node
        a, b = np.arange(1, n), parent
        extra = max(1, n // 10)
        x, y = rng.integers(0, n, extra), rng.integers(0, n, extra)
        keep = x != y
        a, b = np.concatenate([a, x[keep], np.arange(n)]), np.concatenate([b, y[keep], np.full(n, n)])     # ... and the dummy node n
        src.append(np.concatenate([a, b]) + off + 1)
        dst.append(np.concatenate([b, a]) + off + 1)
        labels.append(np.concatenate([rng.choice(37, n, p=weights) + 1, [0]]))
        gi.append(np.full(n + 1, g))
        off += n + 1
    A = np.stack([np.concatenate(src), np.concatenate(dst)], 1)
    el = None
    if edge_labels:
        el = np.where((np.concatenate(labels)[A[:, 0] - 1] == 0) | (np.concatenate(labels)[A[:, 1] - 1] == 0), 0, 1)
    return gk.GraphKernelData.from_arrays(np.concatenate(gi), A, np.concatenate(labels), el, [0] * graphs, device=DEV,
                                          source="synthetic NCI1-shaped, seed %d" % seed)


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--edge-labels", action="store_true", help="dummy edges labelled 0, the others 1 (entries 2 deg instead of deg)")
    a = ap.parse_args()
    data = dataset(a.graphs, a.seed, a.edge_labels)
    H, uel = a.iters, a.edge_labels
    plan = data.plan(uel)
    shape = dict(tool="graph_kernel_bench", graphs=data.num_graphs, nodes=data.num_nodes, slots=int(data.nbr.numel()), H=H,
                 edge_labels=uel, lists_8=int(plan.small.numel()), lists_64=int(plan.wave.numel()), lists_lds=int(plan.block.numel()),
                 lists_composed=int(plan.huge.numel()))
    with ops.wl_fused(True):
        cf = gk.wl_colors(data, H, True, uel)
    with ops.wl_fused(False):
        cc = gk.wl_colors(data, H, True, uel)
    assert torch.equal(cf, cc), "fused and composed colours differ"
    feats = gk.wl_features(data, H, True, uel, colors=cf)
    shape.update(feature_entries=int(feats.color.numel()), longest_row=feats.max_row)
    print(json.dumps(dict(shape, what="shape")), flush=True)
    whats = {"refine_fused": lambda: _colors(data, H, uel, True), "refine_composed": lambda: _colors(data, H, uel, False),
             "features": lambda: gk.wl_features(data, H, True, uel, colors=cf),
             "gram_WL": lambda: gk.wl_gram_matrices(data, H, "WL", True, uel, features=feats),
             "gram_WLOA": lambda: gk.wl_gram_matrices(data, H, "WLOA", True, uel, features=feats)}
    all_times, round_medians = {w: [] for w in whats}, {w: [] for w in whats}
    for rnd in range(a.rounds):
        for w, fn in whats.items():
            few = w.startswith("gram") or w == "features"
            times = timed(fn, max(2, a.steps // 3) if few else a.steps, 1 if few else a.warmup)
            all_times[w] += times
            round_medians[w].append(statistics.median(times))
            print(json.dumps(dict(tool="graph_kernel_bench", what=w, round=rnd, calls=len(times), median_ms=statistics.median(times),
                                  min_ms=min(times), max_ms=max(times))), flush=True)
    med = {w: statistics.median(t) for w, t in all_times.items()}
    spread = {w: (max(round_medians[w]) - min(round_medians[w])) / med[w] for w in whats}
    print(json.dumps(dict(shape, what="summary", rounds=a.rounds, median_ms={w: round(v, 4) for w, v in med.items()},
                          round_spread={w: round(v, 4) for w, v in spread.items()},
                          fused_over_composed=round(med["refine_fused"] / med["refine_composed"], 4))), flush=True)


def _colors(data, H, uel, fused):
    with ops.wl_fused(fused):
        return gk.wl_colors(data, H, True, uel)


if __name__ == "__main__":
    main()
