#!/usr/bin/env python3
"""Durations of BatchNorm's forward launches (dn_batchnorm_rows_*: colreduce -> colstats -> colapply;
builds before the chunked statistics call the second one colfinal) from a rocprofv3 kernel trace:
    python tools/bn_stats_bench.py [--dtype f32|bf16] [N C ...]          (default: 20181 256 5000 128)
The statistics are the first two launches; the third (apply) is printed beside them as a control that no change to the statistics
touches.  For two builds of the library on ONE box, alternate them:  DN_HIP_LIB=/path/libdn_hip.so python tools/bn_stats_bench.py
(as tools/ab_lib.sh does for bench.py).  The parent only starts the traced child and reads its CSV: it never opens the GPU."""
import collections
import csv
import glob
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPS = 200


def child(dtype, shapes):
    sys.path.insert(0, ROOT)
    import torch
    from dummynode4graphlearning_amd import ops
    dt = torch.float32 if dtype == "f32" else torch.bfloat16
    for N, C in shapes:
        x = (torch.randn(N, C, device="cuda") * 2 + 30).to(dt)
        w, b = torch.ones(C, device="cuda"), torch.zeros(C, device="cuda")
        for _ in range(REPS):
            ops.batch_norm_rows(x, w, b, 1e-5)
        torch.cuda.synchronize()


def main():
    args = sys.argv[1:]
    dtype = "f32"
    if "--dtype" in args:
        i = args.index("--dtype")
        dtype = args[i + 1]
        del args[i:i + 2]
    if args and args[0] == "--child":
        vals = [int(v) for v in args[1:]]
        return child(dtype, list(zip(vals[::2], vals[1::2])))
    vals = [int(v) for v in args] or [20181, 256, 5000, 128]
    shapes = list(zip(vals[::2], vals[1::2]))
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "-o", "k", "--", sys.executable, os.path.abspath(__file__),
               "--dtype", dtype, "--child"] + [str(v) for v in vals]
        r = subprocess.run(cmd, cwd=d, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=280)
        files = sorted(glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True))
        if r.returncode != 0 or not files:
            sys.stdout.write(r.stdout.decode(errors="replace")[-2000:])
            sys.exit("rocprofv3 run failed (exit %d)" % r.returncode)
        rows = sorted(csv.DictReader(open(files[-1])), key=lambda q: int(q["Start_Timestamp"]))
    by = collections.defaultdict(list)
    for q in rows:
        n = q["Kernel_Name"]
        for key, name in (("colreduce_kernel", "colreduce_kernel"), ("colfinal_kernel", "colstats_kernel"), ("colstats_kernel", "colstats_kernel"),
                          ("colapply_kernel", "colapply_kernel")):
            if key in n:
                by[name].append((int(q["End_Timestamp"]) - int(q["Start_Timestamp"])) / 1e3)
    lib = os.environ.get("DN_HIP_LIB", "(in-tree build)")
    for i, (N, C) in enumerate(shapes):                                # launches are in shape order, REPS of each
        med = {}
        for key, v in by.items():
            part = sorted(v[i * REPS + REPS // 4:(i + 1) * REPS])       # (the first quarter warms the caches and clocks)
            med[key] = part[len(part) // 2] if part else float("nan")
        print("%s %s N=%d C=%d: colreduce %.2f us + colstats %.2f us = statistics %.2f us; colapply %.2f us" % (
            lib, dtype, N, C, med.get("colreduce_kernel", 0), med.get("colstats_kernel", 0),
            med.get("colreduce_kernel", 0) + med.get("colstats_kernel", 0), med.get("colapply_kernel", 0)))


if __name__ == "__main__":
    main()
