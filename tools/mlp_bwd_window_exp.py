"""Launch A of the MLP backward (ops.mlp_bwd_fused with both masks) alone, twice: on a config-5-sized row set with the MLP's own
chunk table (256 chunks of 128 tiles), and with every chunk folded onto the SAME 2,048 rows (a 1 MiB window per operand: after the
first touch every read is an L2 hit, so what is left is the workgroup's own instruction stream).  us per launch and ns per tile.

usage: python tools/mlp_bwd_window_exp.py [--rows N] [--slope S] [--iters K]"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from dummynode4graphlearning_amd import ops  # noqa: E402


def timed(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    t = sorted(a.elapsed_time(b) * 1e3 for a, b in ev)
    return t[len(t) // 2], t[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=2 ** 20)
    ap.add_argument("--slope", type=float, default=0.0)
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    n, H = args.rows, 256
    gen = torch.Generator(device=dev).manual_seed(9)
    g = torch.randn(n, H, device=dev, generator=gen).to(torch.bfloat16)
    a = torch.randn(n, H, device=dev, generator=gen).to(torch.bfloat16)
    w = (torch.randn(H, H, device=dev, generator=gen) / 16).to(torch.bfloat16)
    bits_in = torch.randint(0, 256, (n, H // 8), device=dev, generator=gen, dtype=torch.uint8)
    bits_out = torch.randint(0, 256, (n, H // 8), device=dev, generator=gen, dtype=torch.uint8)
    real = ops._dense_table(n, dev)[1]
    nch = real[2]
    tiles_real = -(-int(real[0][0, 2] - real[0][0, 1]) // 32)
    win = 2048
    fold = (torch.tensor([(0, 0, win, 0)] * nch, dtype=torch.int32, device=dev), torch.tensor([0, nch], dtype=torch.int32, device=dev), nch)
    for name, table, tiles in (("own table", real, tiles_real), ("folded onto %d rows" % win, fold, win // 32)):
        with torch.no_grad():
            med, best = timed(lambda: ops.mlp_bwd_fused(g, a, w, table, mask_in_bits=bits_in, mask_out_bits=bits_out, slope=args.slope),
                              args.iters)
        print("%-24s %d chunks x %3d tiles: median %.1f us, min %.1f us (incl. the reduce launch); %.0f ns per tile (min)"
              % (name, nch, tiles, med, best, best * 1e3 / tiles))


if __name__ == "__main__":
    main()
