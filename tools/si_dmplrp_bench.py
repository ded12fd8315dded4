"""DMPLRP pooling on two batches: the config-3 scale batch of tools/si_lrp_bench.py (512 graphs of 49 + 1 nodes, every ego small)
and a batch of larger dummy-augmented graphs (--hub-graphs graphs of 63 + 1 nodes whose dummy node is connected forwards to every
node, so its ego of C(63, L - 1) combinations dominates).  H = 64, fp32, eager, synchronised.

Per batch:
  index   build times over fresh batch objects: the ego index, the materialised index (the composed path's), the collapsed index
          (ops.LrpIndex.collapsed), with the sequence count P, the collapsed entries Q and the composed list length
  op      ops.lrp_pool_linear forward + backward (pool = mean), the paths ALTERNATED in one process:
          collapsed | composed (lrp_pool(act="none") over the materialised index) | fused (dn_lrp_pool_*)
  layer   one DMPLRPPoolLayer forward + backward on the same three paths
--rounds rounds of --steps steps each after --warmup warm-ups; one JSON line per measurement with median, min and max ms."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import si_dual_model_bench as B  # noqa: E402  (graph_of, timed)
import si_lrp_bench as LB  # noqa: E402  (scale_batches, _sync_time, materialisable)
from dummynode4graphlearning_amd import BatchedGraph, ops  # noqa: E402
from dummynode4graphlearning_amd import subgraph_isomorphism as si  # noqa: E402

DEV = B.DEV
IMPLS = ("collapsed", "composed", "fused")


def hub_batch(graphs, real=63, out_deg=4, seed=0):
    """`graphs` graphs of `real` nodes + one dummy node (last): every real node has `out_deg` distinct targets, every real edge a
    reversed copy (is_reversed), and the dummy is connected to and from every real node with counted edges."""
    rng = np.random.default_rng(seed)
    n = real + 1
    a = np.repeat(np.arange(real), out_deg)
    srcs, dsts, revs = [], [], []
    for g in range(graphs):
        b = (a + 1 + np.concatenate([rng.choice(real - 1, size=out_deg, replace=False) for _ in range(real)])) % real
        hub = np.full(real, real)
        src = np.concatenate([a, b, hub, np.arange(real)]) + g * n
        dst = np.concatenate([b, a, np.arange(real), hub]) + g * n
        srcs.append(src)
        dsts.append(dst)
        revs.append(np.concatenate([np.zeros(len(a), bool), np.ones(len(a), bool), np.zeros(2 * real, bool)]))
    dummy = np.zeros(graphs * n, bool)
    dummy[real::n] = True
    t = lambda x: torch.from_numpy(np.concatenate(x)).to(DEV)                      # noqa: E731

    def make():
        return BatchedGraph(t(srcs), t(dsts), graphs * n, batch_num_nodes=torch.full((graphs,), n, dtype=torch.long),
                            batch_num_edges=torch.full((graphs,), len(srcs[0]), dtype=torch.long),
                            ndata={"is_dummy": torch.from_numpy(dummy).to(DEV)}, edata={"is_reversed": t(revs)})
    return make


class _path:
    def __init__(self, impl):
        self.cms = (ops.lrp_collapsed(impl == "collapsed"), ops.lrp_fused() if impl == "fused" else ops.lrp_composed())

    def __enter__(self):
        for c in self.cms:
            c.__enter__()

    def __exit__(self, *exc):
        for c in reversed(self.cms):
            c.__exit__(*exc)
        return False


def index_times(make, L, steps, batch):
    ego, mat, col = [], [], []
    for _ in range(steps + 1):
        g = make()
        g.node_ptr()
        t, ix = LB._sync_time(lambda: g.lrp_index(L))
        ego.append(t)
        if LB.materialisable(ix):
            mat.append(LB._sync_time(ix.composed_tables)[0])
        col.append(LB._sync_time(ix.collapsed)[0])
    med = lambda v: statistics.median(v[1:]) if len(v) > 1 else None                 # noqa: E731
    return dict(tool="si_dmplrp_bench", what="index", batch=batch, seq_len=L, nodes=g.number_of_nodes(), edges=g.number_of_edges(),
                sequences=int(ix.count.sum()), max_sequences_per_node=int(ix.count.max()),
                collapsed_entries=int(ix.collapsed().col_rows.numel()),
                composed_entries=int(ix.composed_tables()[0].numel()) if LB.materialisable(ix) else None, steps=steps,
                ego_index_median_ms=med(ego), composed_index_median_ms=med(mat), collapsed_index_median_ms=med(col),
                collapsed_index_min_max_ms=[min(col[1:]), max(col[1:])], composed_index_min_max_ms=[min(mat[1:]), max(mat[1:])] if mat else None)


def run_batch(batch, make, a):
    L, H = a.seq_len, a.width
    print(json.dumps(index_times(make, L, a.steps, batch)), flush=True)
    gg = make()
    torch.manual_seed(21)
    layer = si.DMPLRPPoolLayer(H, H, lrp_seq_len=L, batch_norm=False, act_func="leaky_relu").to(DEV)
    x = torch.randn(gg.number_of_nodes(), H, device=DEV)
    ef = torch.randn(gg.number_of_edges(), H, device=DEV)

    def op_step():
        layer.zero_grad(set_to_none=True)
        xx, ee = x.clone().requires_grad_(True), ef.clone().requires_grad_(True)
        ops.lrp_pool_linear(xx, ee, layer.lrp_weight, layer.lrp_bias, gg, L, pool="mean").sum().backward()

    def layer_step():
        layer.zero_grad(set_to_none=True)
        xx, ee = x.clone().requires_grad_(True), ef.clone().requires_grad_(True)
        no, eo = layer(gg, xx, ee)
        (no.sum() + eo.sum()).backward()

    impls = [i for i in IMPLS if i != "composed" or LB.materialisable(gg.lrp_index(L))]
    for what, step in (("op", op_step), ("layer", layer_step)):
        for rnd in range(a.rounds):
            for impl in impls:
                with _path(impl):
                    times = B.timed(step, a.steps, a.warmup)
                    with ops.KernelTimer() as timer:
                        step()
                    tags = {k: round(v[1], 3) for k, v in timer.summary().items() if k.startswith(("lrp_", "gather_segsum", "segment"))}
                print(json.dumps(dict(tool="si_dmplrp_bench", what=what, batch=batch, impl=impl, round=rnd, seq_len=L, H=H,
                                      steps=a.steps, median_ms=statistics.median(times), min_ms=min(times), max_ms=max(times),
                                      kernel_ms=tags)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seq-len", type=int, default=4)
    ap.add_argument("--width", type=int, default=64)
    ap.add_argument("--graphs", type=int, default=512, help="graphs of the config-3 scale batch")
    ap.add_argument("--hub-graphs", type=int, default=32, help="graphs of 63 + 1 nodes of the hub batch")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--batch", choices=["config3", "hub", "both"], default="both")
    a = ap.parse_args()
    if a.batch in ("config3", "both"):
        _, ga, _ = LB.scale_batches(graphs=a.graphs)
        run_batch("config3", lambda: B.graph_of(ga), a)
    if a.batch in ("hub", "both"):
        run_batch("hub", hub_batch(a.hub_graphs), a)


if __name__ == "__main__":
    main()
