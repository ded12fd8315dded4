"""Kernel-SVM evaluation on one seeded synthetic dataset: NCI1-shaped (4110 graphs of tools/graph_kernel_bench.py's generator with
dummy nodes, 2 classes), WL gram matrices at H = 5 computed on the device and normalised in memory, then the reference's search:
--seeds seeds x 6 matrices x 7 C = 420 C-SVC duals of about 3288 training rows each.

The classes are a noisy threshold on a graph statistic (the share of nodes with one of the two commonest labels, 10 % flipped), so
that the duals are neither separable nor pure noise.

Times, with a synchronised host clock around device work:
  full       graph_kernels_svm.evaluate_dataset on the whole workload, fused path (dn_svm_smo_f64): --full-rounds times;
  ab         the subset both paths can finish -- --ab-seeds seeds, all matrices, the C values of --ab-cs -- fused and composed
             (ops.svm_smo_composed: the same algorithm in torch ops, all solves side by side) ALTERNATED in one process, --rounds rounds;
  decision   the share of the fused evaluation spent outside the SMO launches (tables, decision values K_m @ W, votes);
  sklearn    where scikit-learn imports: SVC(kernel="precomputed", tol=1e-3) fit + predict on one core for the ab subset (for scale).
Prints one JSON line per measurement and a summary line: medians, spreads (max - min) / median, launches, total iterations,
iterations per second and the longest launch of the fused path."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
from dummynode4graphlearning_amd import graph_kernels as gk, graph_kernels_svm as svm, ops  # noqa: E402
import graph_kernel_bench  # noqa: E402

DEV = "cuda:0"


def classes_of(data, seed):
    lab = data.node_label.cpu().numpy()
    g = data.node_graph.cpu().numpy()
    common = np.bincount(g, weights=((lab == 1) | (lab == 2)), minlength=data.num_graphs)
    share = common / np.maximum(np.bincount(g, minlength=data.num_graphs) - 1, 1)
    cls = (share > np.median(share)).astype(np.int64)
    flip = np.random.default_rng(seed).random(data.num_graphs) < 0.10
    return np.where(flip, 1 - cls, cls)


def run(K, classes, splits, Cs, fused, ipl):
    """One evaluation: (seconds, seconds inside SMO launches, launches, longest launch ms, total iterations, accuracies)."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with ops.svm_fused(fused), ops.KernelTimer() as timer:
        batch = svm.solve_batch(K, classes, splits, Cs, 1e-3, ipl)
        acc = svm.select(batch, classes, splits)
    torch.cuda.synchronize()
    total = time.perf_counter() - t0
    per_launch = [a.elapsed_time(b) for tag, a, b in timer.records if tag == "svm_smo"]
    return dict(seconds=total, smo_seconds=sum(per_launch) / 1e3, launches=len(per_launch), longest_launch_ms=max(per_launch, default=0.0),
                iterations=int(batch["iterations"].sum()), longest_solve=int(batch["iterations"].max()), solves=int(batch["table"].shape[0]),
                capped=int((batch["status"] == ops.SVM_CAPPED).sum()), valid_acc=[round(float(x), 2) for x in acc[1].mean(0)])


def sklearn_seconds(K, classes, splits, Cs):
    try:
        from sklearn.svm import SVC
    except Exception:
        return None
    Kh = K.cpu().numpy()
    t0 = time.perf_counter()
    for tr, va, te in splits:
        for g in Kh:
            for c in Cs:
                clf = SVC(C=c, kernel="precomputed", tol=0.001).fit(g[tr][:, tr], classes[tr])
                clf.predict(g[va][:, tr])
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", type=int, default=4110)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--seeds", type=int, default=10)
    ap.add_argument("--full-rounds", type=int, default=2)
    ap.add_argument("--ab-seeds", type=int, default=1)
    ap.add_argument("--ab-cs", type=float, nargs="+", default=[1.0, 0.1, 0.01, 0.001])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters-per-launch", type=int, default=None)
    ap.add_argument("--no-sklearn", action="store_true")
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    data = graph_kernel_bench.dataset(a.graphs, a.seed, False)
    classes = classes_of(data, a.seed)
    mats = gk.wl_gram_matrices(data, a.iters, "WL", True, False)
    K = torch.stack([svm.normalize_gram_svm(m) for m in mats]).contiguous()
    splits = [svm.split_indices(a.graphs, s) for s in range(a.seeds)]
    ipl = ops.SVM_ITERS_PER_LAUNCH if a.iters_per_launch is None else a.iters_per_launch
    shape = dict(tool="graph_kernel_svm_bench", graphs=a.graphs, H=a.iters, matrices=len(mats), seeds=a.seeds, train_rows=len(splits[0][0]),
                 positives=int(classes.sum()), iters_per_launch=ipl, max_rows=ops.svm_max_rows())
    print(json.dumps(dict(shape, what="shape")), flush=True)
    ab_splits, ab_cs = splits[:a.ab_seeds], np.array(a.ab_cs)
    rounds = {"ab_fused": [], "ab_composed": []}
    run(K, classes, ab_splits, ab_cs[-1:], True, ipl)                        # warm-up: library load, allocator
    for rnd in range(a.rounds):
        for what, fused in (("ab_fused", True), ("ab_composed", False)):
            r = run(K, classes, ab_splits, ab_cs, fused, ipl)
            rounds[what].append(r)
            print(json.dumps(dict(r, tool="graph_kernel_svm_bench", what=what, round=rnd, cs=a.ab_cs, ab_seeds=a.ab_seeds)), flush=True)
    full = []
    for rnd in range(a.full_rounds):
        r = run(K, classes, splits, None, True, ipl)
        full.append(r)
        print(json.dumps(dict(r, tool="graph_kernel_svm_bench", what="full_fused", round=rnd)), flush=True)
    sk = None if a.no_sklearn else sklearn_seconds(K, classes, ab_splits, ab_cs)
    med = {w: statistics.median(r["seconds"] for r in rs) for w, rs in rounds.items()}
    spread = {w: (max(r["seconds"] for r in rs) - min(r["seconds"] for r in rs)) / med[w] for w, rs in rounds.items()}
    summary = dict(shape, what="summary", rounds=a.rounds, ab_subset=dict(seeds=a.ab_seeds, cs=a.ab_cs, solves=rounds["ab_fused"][0]["solves"]),
                   ab_median_s={w: round(v, 4) for w, v in med.items()}, ab_spread={w: round(v, 4) for w, v in spread.items()},
                   every_fused_round_faster=max(r["seconds"] for r in rounds["ab_fused"]) < min(r["seconds"] for r in rounds["ab_composed"]),
                   fused_over_composed=round(med["ab_fused"] / med["ab_composed"], 5), sklearn_one_core_s=None if sk is None else round(sk, 2))
    if full:
        f = min(full, key=lambda r: r["seconds"])
        summary.update(full_median_s=round(statistics.median(r["seconds"] for r in full), 3), full_launches=f["launches"],
                       full_iterations=f["iterations"], full_longest_solve=f["longest_solve"], full_capped=f["capped"],
                       full_longest_launch_ms=round(max(r["longest_launch_ms"] for r in full), 3),
                       full_iterations_per_s=round(f["iterations"] / f["smo_seconds"], 1),
                       full_share_outside_smo=round(1.0 - f["smo_seconds"] / f["seconds"], 4))
    print(json.dumps(summary), flush=True)


if __name__ == "__main__":
    main()
