"""SP / GR graph-kernel feature builds on one seeded synthetic dataset with the GC dummy node (label 0, joined to every node of its
graph by edges labelled 0), node labels on:

  --shape nci1   --graphs NCI1-shaped graphs (10..50 nodes, a random tree plus a few ring-closing edges, 37 skewed node labels): the
                 dataset of tools/graph_kernel_bench.py
  --shape dd     --graphs DD-shaped graphs (log-normal sizes around 250 nodes, a few of several thousand, about 2.5 edges per node,
                 82 skewed node labels)

Times, with a synchronised host clock around device work, sp_features and gr_features whole (plans cached, so: launches, the scan,
the sort and run-length reduction, the read-back of the entry count), the dn_gk_* kernels against the composed torch-op path,
ALTERNATED in one process: --rounds rounds of --steps calls each after --warmup warm-up calls per path and round; and the gram
launch over each feature CSR.  Prints one JSON line per (round, what) and a summary line: the median over all calls of each path,
the spread of the per-round medians (max - min) / median, and fused / composed per kernel.  The two paths' features are compared
once (they must be equal)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dummynode4graphlearning_amd import graph_kernels as gk, graph_kernels_spgr as sg, ops  # noqa: E402

DEV = "cuda:0"


def dataset(shape, graphs, seed, edge_labels):
    rng = np.random.default_rng(seed)
    gi, src, dst, labels, off = [], [], [], [], 0
    vocab = 37 if shape == "nci1" else 82
    weights = 1.0 / np.arange(1, vocab + 1)
    weights /= weights.sum()
    for g in range(1, graphs + 1):
        if shape == "nci1":
            n = int(rng.integers(10, 51))
            extra = max(1, n // 10)
        else:
            n = int(min(5700, max(30, rng.lognormal(5.5, 0.75))))
            if g % 60 == 1:
                n = int(rng.integers(2000, 5700))                                   # the few proteins of several thousand residues
            extra = 3 * n // 2
        parent = (rng.random(n - 1) * np.arange(1, n)).astype(np.int64)             # a random tree: node v joins an earlier node
        a, b = np.arange(1, n), parent
        x, y = rng.integers(0, n, extra), rng.integers(0, n, extra)
        keep = x != y
        a, b = np.concatenate([a, x[keep], np.arange(n)]), np.concatenate([b, y[keep], np.full(n, n)])     # ... and the dummy node n
        src.append(np.concatenate([a, b]) + off + 1)
        dst.append(np.concatenate([b, a]) + off + 1)
        labels.append(np.concatenate([rng.choice(vocab, n, p=weights) + 1, [0]]))
        gi.append(np.full(n + 1, g))
        off += n + 1
    A = np.stack([np.concatenate(src), np.concatenate(dst)], 1)
    el = None
    if edge_labels:
        el = np.where((np.concatenate(labels)[A[:, 0] - 1] == 0) | (np.concatenate(labels)[A[:, 1] - 1] == 0), 0, 1)
    return gk.GraphKernelData.from_arrays(np.concatenate(gi), A, np.concatenate(labels), el, [0] * graphs, device=DEV,
                                          source="synthetic %s-shaped, seed %d" % (shape, seed))


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


def _with(fused, fn):
    def run():
        with ops.gk_fused(fused):
            return fn()
    return run


def _same(f, g):
    return all(torch.equal(getattr(f, a), getattr(g, a)) for a in ("ptr", "color", "count"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=("nci1", "dd"), default="nci1")
    ap.add_argument("--graphs", type=int, default=None, help="default: 4096 (nci1), 300 (dd)")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--edge-labels", action="store_true", help="GR keys with edge labels (dummy edges 0, the others 1)")
    ap.add_argument("--kernels", default="SP,GR")
    a = ap.parse_args()
    graphs = a.graphs or (4096 if a.shape == "nci1" else 300)
    data = dataset(a.shape, graphs, a.seed, a.edge_labels)
    uel = a.edge_labels
    sp = lambda: sg.sp_features(data, True)  # noqa: E731
    gr = lambda: sg.gr_features(data, True, uel)  # noqa: E731
    kernels = a.kernels.split(",")
    shape = dict(tool="graph_kernel_spgr_bench", shape=a.shape, graphs=data.num_graphs, nodes=data.num_nodes, slots=int(data.nbr.numel()),
                 largest_graph=data.max_nodes, edge_labels=uel)
    whats = {}
    if "SP" in kernels:
        fs, cs = _with(True, sp)(), _with(False, sp)()
        assert _same(fs, cs), "fused and composed SP features differ"
        plan = sg._sp_plan(data, True, ops.gk_sp_lds_max_nodes())
        shape.update(sp_graphs_wave=int(plan.wave.size), sp_graphs_lds=int(plan.block.size), sp_graphs_composed=int(plan.large.size),
                     sp_entries=int(fs.color.numel()), sp_longest_row=fs.max_row)
        whats.update(sp_fused=_with(True, sp), sp_composed=_with(False, sp), sp_gram=lambda: sg.sp_gram_matrix(data, True, features=fs))
    if "GR" in kernels:
        fg, cg = _with(True, gr)(), _with(False, gr)()
        assert _same(fg, cg), "fused and composed GR features differ"
        plan = sg._gr_plan(data, sg.GR_WORKSPACE_KEYS)
        shape.update(gr_pairs=plan.pairs, gr_chunks=len(plan.chunks), gr_entries=int(fg.color.numel()), gr_longest_row=fg.max_row)
        whats.update(gr_fused=_with(True, gr), gr_composed=_with(False, gr), gr_gram=lambda: sg.gr_gram_matrix(data, True, uel, features=fg))
    print(json.dumps(dict(shape, what="shape")), flush=True)
    all_times, round_medians = {w: [] for w in whats}, {w: [] for w in whats}
    for rnd in range(a.rounds):
        for w, fn in whats.items():
            times = timed(fn, a.steps, a.warmup)
            all_times[w] += times
            round_medians[w].append(statistics.median(times))
            print(json.dumps(dict(tool="graph_kernel_spgr_bench", what=w, round=rnd, calls=len(times), median_ms=statistics.median(times),
                                  min_ms=min(times), max_ms=max(times))), flush=True)
    med = {w: statistics.median(t) for w, t in all_times.items()}
    spread = {w: (max(round_medians[w]) - min(round_medians[w])) / med[w] for w in whats}
    ratio = {k: round(med[k.lower() + "_fused"] / med[k.lower() + "_composed"], 4) for k in kernels}
    print(json.dumps(dict(shape, what="summary", rounds=a.rounds, median_ms={w: round(v, 4) for w, v in med.items()},
                          round_spread={w: round(v, 4) for w, v in spread.items()}, fused_over_composed=ratio)), flush=True)


if __name__ == "__main__":
    main()
