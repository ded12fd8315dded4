"""Forward + backward of an attention count head (or DIAMNet) on the config-3 scale batch of tools/si_dual_model_bench.py (512 pairs),
the fused kernels of dn_seg_attn.hip against the composed path (the reference's padded algorithm on the ragged rows).

    python tools/si_attn_bench.py --impl both [--head DIAMNet] [--model] [--steps 20] [--rounds 5]

Without --model: the head alone (graph_adj.attn_head_ragged) on random rows at the model's widths, once on the node rows and once
on the edge rows of the DMPNN edge head (is_dummy | is_reversed edges skipped).  With --model: the whole DMPNN step with the head
attached by set_pred_net.  The two paths alternate round by round in one process; per path the median over the rounds' medians
and their spread (min .. max) are printed as one JSON line per measurement."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import si_dual_model_bench as B  # noqa: E402
from dummynode4graphlearning_amd import ops  # noqa: E402
from dummynode4graphlearning_amd import subgraph_isomorphism as si  # noqa: E402
from dummynode4graphlearning_amd.subgraph_isomorphism.attn_pred import build_attn_pred_net  # noqa: E402
from dummynode4graphlearning_amd.subgraph_isomorphism.graph_adj import attn_head_ragged  # noqa: E402

DEV = B.DEV


def _alternate(step, impls, steps, warmup, rounds):
    med = {i: [] for i in impls}
    for r in range(rounds):
        for impl in impls:
            with ops.attn_fused(impl == "fused"):
                t = B.timed(step, steps, warmup if r == 0 else 1)
            med[impl].append(statistics.median(t))
    return {i: dict(median_ms=statistics.median(m), min_ms=min(m), max_ms=max(m), rounds=m) for i, m in med.items()}


def _side(aug, kind):
    if kind == "v":
        ptr, skip = aug["node_ptr"], aug["is_dummy_node"].bool()
    else:
        ptr, skip = aug["edge_ptr"], aug["is_dummy_edge"].bool() | aug["is_reversed"].bool()
    ptr = ptr.to(torch.int32)
    lens = (ptr[1:] - ptr[:-1]).long()
    seg = torch.repeat_interleave(torch.arange(lens.numel(), device=DEV), lens)
    count = torch.zeros(lens.numel(), device=DEV).index_add_(0, seg, (~skip).float())
    return ptr, skip, int(lens.max()), count


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--impl", choices=["fused", "composed", "both"], default="both")
    ap.add_argument("--head", default="MeanAttnPredictNet", choices=["MeanAttnPredictNet", "SumAttnPredictNet", "MaxAttnPredictNet", "DIAMNet"])
    ap.add_argument("--model", action="store_true")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--infer-steps", type=int, default=1)
    a = ap.parse_args()
    impls = ["fused", "composed"] if a.impl == "both" else [a.impl]
    pa, ga, nel = B.scale_batches()
    kw = dict(pred_hid_dim=64, pred_num_heads=4, pred_infer_steps=a.infer_steps)
    torch.manual_seed(21)
    if a.model:
        cfg = B.config("DMPNN", nel)
        model = si.DMPNN(**cfg)
        model.set_pred_net(a.head, **{k: v for k, v in dict(cfg, **kw).items() if k != "pred_net"})
        model = B.perturb(model).to(DEV).train()
        pg, gg = B.graph_of(pa), B.graph_of(ga)
        coef = (torch.arange(1, 513, dtype=torch.float32, device=DEV) / 512).view(-1, 1)

        def step():
            model.zero_grad(set_to_none=True)
            (model(pg, gg)["pred_c"].float() * coef).sum().backward()
        res = _alternate(step, impls, a.steps, a.warmup, a.rounds)
        print(json.dumps(dict(tool="si_attn_bench", what="DMPNN model step", head=a.head, infer_steps=a.infer_steps,
                              nodes=gg.number_of_nodes(), edges=gg.number_of_edges(), **res)))
        return
    for kind in ("v", "e"):
        D = 64
        net = B.perturb(build_attn_pred_net(a.head, D, False, **kw)).to(DEV).train()
        pp, ps, Lp, pc = _side(pa, kind)
        gp, gs, Lg, gc = _side(ga, kind)
        p_rows = torch.randn(ps.numel(), D, device=DEV)
        g_rows = torch.randn(gs.numel(), D, device=DEV)

        def step():
            net.zero_grad(set_to_none=True)
            pr, gr = p_rows.clone().requires_grad_(True), g_rows.clone().requires_grad_(True)
            attn_head_ragged(net, pr, pp, ps, Lp, pc, gr, gp, gs, Lg, gc).sum().backward()
        res = _alternate(step, impls, a.steps, a.warmup, a.rounds)
        print(json.dumps(dict(tool="si_attn_bench", what="%s head" % ("node" if kind == "v" else "edge"), head=a.head,
                              infer_steps=a.infer_steps, pattern_rows=int(ps.numel()), graph_rows=int(gs.numel()), max_pattern=Lp,
                              max_graph=Lg, **res)), flush=True)


if __name__ == "__main__":
    main()
