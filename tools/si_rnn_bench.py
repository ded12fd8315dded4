"""RNN on the scale batch of tools/si_cnn_bench.py (512 pairs with dummy nodes and reversed edges, H = 64, turned into edge
sequences): one RNNLayer forward + backward on the graph sequences, or a whole RNN(**cfg) step (3 layers), with the recurrence on the
fused kernels (dn_eseq_rnn.hip) against the composed path -- torch's own nn.LSTM / nn.GRU / nn.RNN, on MIOpen (`composed`) and on
torch's native per-step kernels (`native`: the same module with the cuDNN / MIOpen backend switched off).  Eager, fp32, synchronised
host clock, the paths ALTERNATED in one process: --rounds rounds of --steps steps each, after --warmup warm-up steps per path and round.

  --impl fused | composed | native | all        (all: the three, alternated)
  --model          time RNN(**cfg) forward + backward (patterns + graphs) instead of the layer alone
  --cell           lstm,gru,rnn (comma separated)
  --bidirectional  hidden width 32 per direction instead of 64

Prints one JSON line per (cell, round, path) with the kernel launches of a step by tag (count, ms), and for --impl all a summary line
per cell: the median over all steps of each path, the spread of the per-round medians (max - min) / median, and whether EVERY fused
round was faster than EVERY round of the faster composed path (the project's rule for a default).  With 16 sequences per workgroup
the 512-pair batch fills 32 workgroups per direction of 256 CUs: the recurrence kernels are latency-bound by design."""
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
KERNELS = ("eseq_rnn_proj", "eseq_rnn_fwd", "eseq_rnn_bwd", "eseq_rnn_wgrad", "eseq_rnn_composed", "eseq_filter_gate", "si_embed",
           "si_embed_wgrad")
CELLS = {"lstm": "LSTM", "gru": "GRU", "rnn": "RNN"}


class _path:
    """fused: the kernels; composed / native: torch's module on MIOpen / on its own per-step kernels."""

    def __init__(self, impl):
        self.impl = impl

    def __enter__(self):
        self.keep = ops.ESEQ_RNN_COMPOSED_NATIVE
        ops.ESEQ_RNN_COMPOSED_NATIVE = self.impl == "native"
        self.cm = ops.eseq_fused(self.impl == "fused")
        self.cm.__enter__()

    def __exit__(self, *exc):
        self.cm.__exit__(*exc)
        ops.ESEQ_RNN_COMPOSED_NATIVE = self.keep
        return False


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--impl", choices=["fused", "composed", "native", "all"], default="all")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--model", action="store_true")
    ap.add_argument("--cell", default="lstm,gru,rnn")
    ap.add_argument("--bidirectional", action="store_true")
    a = ap.parse_args()
    pa, ga, nel = B.scale_batches()
    ps, gs = EdgeSeq.from_graph(B.graph_of(pa)), EdgeSeq.from_graph(B.graph_of(ga))
    print(json.dumps(dict(tool="si_rnn_bench", what="batch", pairs=gs.batch_size, pattern_L=int(ps.u.shape[1]), graph_L=int(gs.u.shape[1]),
                          pattern_tuples=ps.number_of_tuples(), graph_tuples=gs.number_of_tuples(),
                          workgroups_per_direction=(gs.batch_size + 15) // 16)), flush=True)
    impls = ["fused", "composed", "native"] if a.impl == "all" else [a.impl]
    what = "model" if a.model else "layer"
    for cell in (CELLS[c] for c in a.cell.split(",")):
        cfg = dict(B.config("RNN", nel), rep_rnn_type=cell, rep_rnn_bidirectional=a.bidirectional)
        H = cfg["hid_dim"]
        torch.manual_seed(21)
        if a.model:
            model = B.perturb(si.RNN(**cfg)).to(DEV).train()
            coef = (torch.arange(1, gs.batch_size + 1, dtype=torch.float32, device=DEV) / gs.batch_size).view(-1, 1)

            def step():
                model.zero_grad(set_to_none=True)
                (model(ps, gs)["pred_c"].float() * coef).sum().backward()
        else:
            layer = B.perturb(si.RNNLayer(cell, H, H, bidirectional=a.bidirectional)).to(DEV)
            Bn, L = gs.u.shape
            x = torch.randn(Bn, L, H, device=DEV)
            gate = si.edge_seq.len_mask(gs.lens, L, DEV).float()

            def step():
                layer.zero_grad(set_to_none=True)
                xx = x.clone().requires_grad_(True)
                if ops.eseq_rnn_fused_enabled():
                    y = ops.eseq_rnn(xx, gs.lens, layer.params(), gate, cell, a.bidirectional, True)
                else:
                    y = ops.launch_tagged("eseq_rnn_composed", lambda: ops.eseq_rnn_composed(xx, layer.params(), gate, cell,
                                                                                             a.bidirectional, True))
                y.sum().backward()

        all_times, round_medians = {i: [] for i in impls}, {i: [] for i in impls}
        for rnd in range(a.rounds if a.impl == "all" else 1):
            for impl in impls:
                with _path(impl):
                    times = B.timed(step, a.steps, a.warmup)
                    with ops.KernelTimer() as timer:
                        step()
                    summ = timer.summary()
                launches = {t: [v[0], round(v[1], 3)] for t, v in summ.items() if t in KERNELS}
                all_times[impl] += times
                round_medians[impl].append(statistics.median(times))
                print(json.dumps(dict(tool="si_rnn_bench", what=what, impl=impl, cell=cell, bidirectional=a.bidirectional, round=rnd, H=H,
                                      steps=a.steps, median_ms=statistics.median(times), min_ms=min(times), max_ms=max(times),
                                      launches=launches)), flush=True)
        if a.impl == "all":
            med = {i: statistics.median(all_times[i]) for i in impls}
            spread = {i: (max(round_medians[i]) - min(round_medians[i])) / med[i] for i in impls}
            base = min(("composed", "native"), key=lambda i: med[i])
            print(json.dumps(dict(tool="si_rnn_bench", what=what + "_summary", cell=cell, bidirectional=a.bidirectional, H=H,
                                  rounds=a.rounds, steps=a.steps, median_ms=med, round_spread=spread, baseline=base,
                                  fused_over_baseline=med["fused"] / med[base],
                                  every_fused_round_faster=max(round_medians["fused"]) < min(round_medians[base]))), flush=True)


if __name__ == "__main__":
    main()
