#!/usr/bin/env python3
"""GPU timing of DiffPool on the BASELINE config-2 and config-4 batches (512 dummy-augmented PROTEINS- / NCI1-shaped graphs): the fused
assignment kernels of dn_diffpool.hip against the composed path (the same ragged mathematics in torch ops).

    python tools/gc_diffpool_bench.py [--configs 2,4] [--steps 10] [--rounds 5] [--warmup 3] [--dense]

The model has the reference's default `additional` and max_num_nodes = the batch's largest graph.  Per config, one JSON line each for
  assign   ops.diffpool_assign forward + backward on random logits [N, C] / z [N, F] at the model's first-level widths
  step     the whole training step (forward + nll_loss + backward, no optimiser)
with the two paths alternated round by round in one process after a warm-up: per path the median over the rounds' medians and
their spread (min .. max), and `fused_wins` = every fused round faster than every composed round (the rule for making the kernels
the default).  The step line also carries dense_levels_ms: levels >= 1, final_embed and the head (torch.bmm + the Linear / BatchNorm
kernels) forward + backward, and their share of the fused step.  --dense: one reference-shaped run for scale (level 0 on the padded
[B, Nmax, F] / [B, Nmax, Nmax] tensors through the same modules); not a bar."""
import argparse
import json
import os
import statistics
import sys
from types import SimpleNamespace

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dummynode4graphlearning_amd import GraphBatch, ops, synthetic, transforms  # noqa: E402
from dummynode4graphlearning_amd import graph_classification as GC  # noqa: E402
from dummynode4graphlearning_amd.graph import diffpool_index_of  # noqa: E402

DEV = torch.device("cuda:0")
CONFIGS = {2: ("config 2", synthetic.config2, 3, 5), 4: ("config 4 (one rank)", synthetic.config4, 37, 38)}


def batch_of(raw, labels, F_):
    aug = transforms.dummy_augment_gc(*(torch.from_numpy(raw[k]).to(DEV) for k in ("node_ptr", "edge_ptr", "src", "dst", "node_label", "edge_label")))
    x = F.one_hot(aug["node_label"].long(), labels + 1).float()
    if x.shape[1] < F_:
        x = torch.cat([torch.rand(x.shape[0], F_ - x.shape[1], device=DEV), x], 1)
    node_ptr = aug["node_ptr"].long()
    G = node_ptr.numel() - 1
    batch = torch.repeat_interleave(torch.arange(G, device=DEV), node_ptr[1:] - node_ptr[:-1])
    return GraphBatch(x, torch.stack([aug["src"].long(), aug["dst"].long()]), batch, y=torch.randint(0, 2, (G,), device=DEV), ptr=node_ptr)


def timed(step, steps, warmup):
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    out = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        step()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return out


def alternate(step, steps, warmup, rounds):
    med = {"fused": [], "composed": []}
    for r in range(rounds):
        for impl in ("fused", "composed"):
            with ops.diffpool_fused(impl == "fused"):
                med[impl].append(statistics.median(timed(step, steps, warmup if r == 0 else 1)))
    res = {i: dict(median_ms=round(statistics.median(m), 4), min_ms=round(min(m), 4), max_ms=round(max(m), 4)) for i, m in med.items()}
    res["fused_wins"] = max(med["fused"]) < min(med["composed"])
    return res


def dense_level0(model, data, index):
    """The reference's shape of level 0: the batch padded to [B, Nmax, F] and a dense [B, Nmax, Nmax] adjacency."""
    B, nmax, N = index.num_graphs, index.max_nodes, index.num_nodes
    pos = torch.arange(N, device=DEV) - index.graph_ptr.long()[index.batch]
    x = data.x.new_zeros((B, nmax, data.x.shape[1]))
    x[index.batch, pos] = data.x
    mask = torch.zeros((B, nmax), dtype=torch.bool, device=DEV)
    mask[index.batch, pos] = True
    g = index.batch[index.src]
    adj = torch.zeros(B * nmax * nmax, device=DEV).index_add_(0, (g * nmax + pos[index.src]) * nmax + pos[index.dst],
                                                             torch.ones(index.src.numel(), device=DEV)).view(B, nmax, nmax)
    return model.diffpool_layers[0](x, adj, mask)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="2,4")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--dense", action="store_true")
    a = ap.parse_args()
    for c in (int(v) for v in a.configs.split(",")):
        name, make, labels, F_ = CONFIGS[c]
        data = batch_of(make(), labels, F_)
        index = diffpool_index_of(data)
        torch.manual_seed(c)
        model = GC.DiffPool(SimpleNamespace(num_features=data.x.shape[1], num_classes=2, max_num_nodes=index.max_nodes,
                                            additional=None)).to(DEV).train()
        C = model.diffpool_layers[0].gnn_pool.lin.out_features
        Fz = model.diffpool_layers[1].gnn_pool.conv1.in_channels
        shape = dict(tool="gc_diffpool_bench", config=name, graphs=index.num_graphs, nodes=index.num_nodes, edges=int(index.src.numel()),
                     max_nodes=index.max_nodes, clusters=C, features=Fz, whole_graph_rows=ops.diffpool_graph_rows(C),
                     graphs_taken_whole=sum(n <= ops.diffpool_graph_rows(C) for n in index.sizes))
        logits = torch.randn(index.num_nodes, C, device=DEV)
        z = torch.randn(index.num_nodes, Fz, device=DEV)
        wx = torch.randn(index.num_graphs, C, Fz, device=DEV)
        wa = torch.randn(index.num_graphs, C, C, device=DEV)

        def assign_step():
            s, zz = logits.clone().requires_grad_(True), z.clone().requires_grad_(True)
            X, A = ops.diffpool_assign(s, zz, index)
            ((X * wx).sum() + (A * wa).sum()).backward()
        print(json.dumps(dict(shape, what="assign", **alternate(assign_step, a.steps, a.warmup, a.rounds))), flush=True)

        def step():
            for p in model.parameters():
                p.grad = None
            F.nll_loss(model(data), data.y).backward()
        res = alternate(step, a.steps, a.warmup, a.rounds)

        with torch.no_grad(), ops.diffpool_fused(True):
            x0, adj0, _, _ = model.diffpool_layers[0](data.x, index)

        def dense_levels():
            for p in model.parameters():
                p.grad = None
            x, adj = x0.clone().requires_grad_(True), adj0.clone().requires_grad_(True)
            reads = [torch.max(x, dim=1)[0]]
            for layer in list(model.diffpool_layers)[1:]:
                x, adj, _, _ = layer(x, adj)
                reads.append(torch.max(x, dim=1)[0])
            reads.append(torch.max(model.final_embed(x, adj), dim=1)[0])
            h = F.relu(model.lin1(torch.cat(reads, dim=1)))
            F.nll_loss(F.log_softmax(model.lin2(h), dim=-1), data.y).backward()
        dl = statistics.median(timed(dense_levels, a.steps, a.warmup))
        res["dense_levels_ms"] = round(dl, 4)
        res["dense_levels_share_of_fused_step"] = round(dl / res["fused"]["median_ms"], 3)
        if a.dense:
            def dense_step():
                for p in model.parameters():
                    p.grad = None
                x, adj, _, _ = dense_level0(model, data, index)
                (x.sum() + adj.sum()).backward()

            def ragged_step():
                for p in model.parameters():
                    p.grad = None
                x, adj, _, _ = model.diffpool_layers[0](data.x, index)
                (x.sum() + adj.sum()).backward()
            res["level0_dense_padded_ms"] = round(statistics.median(timed(dense_step, 3, 1)), 4)
            with ops.diffpool_fused(True):
                res["level0_ragged_fused_ms"] = round(statistics.median(timed(ragged_step, a.steps, 2)), 4)
            res["dense_adjacency_mb"] = round(index.num_graphs * index.max_nodes ** 2 * 4 / 1e6, 1)
        print(json.dumps(dict(shape, what="step", **res)), flush=True)


if __name__ == "__main__":
    main()
