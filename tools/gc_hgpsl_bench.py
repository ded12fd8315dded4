#!/usr/bin/env python3
"""GPU timing of HGP-SL on the BASELINE config-2 and config-4 batches (512 dummy-augmented PROTEINS- / NCI1-shaped graphs, as
tools/gc_diffpool_bench.py builds them; the edges coalesced, which HGPSLPool requires): the kernels of dn_hgpsl.hip against the
composed path (the same ragged mathematics in torch ops), H = 128, ratio 0.8, both score functions.

    python tools/gc_hgpsl_bench.py [--configs 2,4] [--steps 10] [--rounds 5] [--warmup 3]

Per config and score function, one JSON line each for
  select     ops.hgpsl_score + ops.hgpsl_topk
  structure  ops.hgpsl_structure forward + backward on the selected rows
  step       the training step of the two-level stack GCN -> pool -> GCN -> pool (forward + a sum loss + backward, no optimiser)
with the two paths alternated round by round in one process after a warm-up: per path the median over the rounds' medians and their
spread (min .. max), and `fused_wins` = every fused round faster than every composed round (the rule for making the kernels the
default).  The step line also carries edge_index_build_ms: the two per-call ops.EdgeIndex builds of the GCN convs, and their share of
the fused step."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from dummynode4graphlearning_amd import ops  # noqa: E402
from dummynode4graphlearning_amd.graph_classification import HGPSLPool, hgpsl  # noqa: E402
from gc_diffpool_bench import CONFIGS, DEV, batch_of, timed  # noqa: E402

H, RATIO = 128, 0.8


def alternate(step, steps, warmup, rounds):
    med = {"fused": [], "composed": []}
    for r in range(rounds):
        for impl in ("fused", "composed"):
            with ops.hgpsl_fused(impl == "fused"):
                med[impl].append(statistics.median(timed(step, steps, warmup if r == 0 else 1)))
    res = {i: dict(median_ms=round(statistics.median(m), 4), min_ms=round(min(m), 4), max_ms=round(max(m), 4)) for i, m in med.items()}
    res["fused_wins"] = max(med["fused"]) < min(med["composed"])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="2,4")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    for c in (int(v) for v in a.configs.split(",")):
        name, make, labels, F_ = CONFIGS[c]
        data = batch_of(make(), labels, F_)
        N = data.x.shape[0]
        key = torch.unique(data.edge_index[0] * N + data.edge_index[1])                        # coalesced: the layer's precondition
        ei = torch.stack([key // N, key % N])
        index = ops.HgpslIndex(ei[0], ei[1], data.ptr, N)
        pooled = index.pooled(RATIO)
        torch.manual_seed(c)
        x = torch.randn(N, H, device=DEV)
        for sparse in (False, True):
            conv1, conv2 = hgpsl.GCN(data.x.shape[1], H).to(DEV), hgpsl.GCN(H, H).to(DEV)
            pool1, pool2 = HGPSLPool(H, ratio=RATIO, sparse=sparse).to(DEV), HGPSLPool(H, ratio=RATIO, sparse=sparse).to(DEV)
            params = [p for m in (conv1, conv2, pool1, pool2) for p in m.parameters()]
            shape = dict(tool="gc_hgpsl_bench", config=name, score="sparsemax" if sparse else "softmax", graphs=index.num_graphs, nodes=N,
                         edges=index.num_edges, hidden=H, ratio=RATIO, pooled_nodes=pooled.num_rows, pairs=pooled.num_pairs, max_k=pooled.max_k,
                         dense_matrix_mb=round(4 * pooled.num_rows ** 2 / 1e6, 1), blocks_mb=round(4 * pooled.num_pairs / 1e6, 2))

            def select_step():
                return ops.hgpsl_topk(ops.hgpsl_score(x, index, None), index, pooled)
            print(json.dumps(dict(shape, what="select", **alternate(select_step, a.steps, a.warmup, a.rounds))), flush=True)

            with ops.hgpsl_fused(True):
                sel = select_step()
            xp0 = x.index_select(0, sel.perm)
            coef = torch.randn(pooled.num_pairs, device=DEV)

            def structure_step():
                pool1.att.grad = None
                xp = xp0.clone().requires_grad_(True)
                (ops.hgpsl_structure(xp, pool1.att, None, index, pooled, sel, sparse, 1.0, 0.2) * coef).sum().backward()
            print(json.dumps(dict(shape, what="structure", **alternate(structure_step, a.steps, a.warmup, a.rounds))), flush=True)

            def step():
                for p in params:
                    p.grad = None
                h = torch.relu(conv1(data.x, ei, None))
                h, e1, w1, b1, ix1 = pool1(h, ei, None, data.batch, index=index, return_index=True)
                h = torch.relu(conv2(h, e1, w1))
                h, e2, w2, b2 = pool2(h, e1, w1, b1, index=ix1)
                (h.sum() + (w2 * w2).sum()).backward()
                return e1
            res = alternate(step, a.steps, a.warmup, a.rounds)
            with ops.hgpsl_fused(True):
                e1 = step()

            def builds():
                ops.EdgeIndex(ei[0], ei[1], N)
                ops.EdgeIndex(e1[0], e1[1], pooled.num_rows)
            eb = statistics.median(timed(builds, a.steps, a.warmup))
            res["edge_index_build_ms"] = round(eb, 4)
            res["edge_index_build_share_of_fused_step"] = round(eb / res["fused"]["median_ms"], 3)
            res["level1_edges"] = int(e1.shape[1])
            print(json.dumps(dict(shape, what="step", **res)), flush=True)


if __name__ == "__main__":
    main()
