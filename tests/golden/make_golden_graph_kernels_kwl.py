"""Golden vectors for the 2-WL graph kernels (tests/test_graph_kernels_kwl_host.py, tests/test_gpu_graph_kernels_kwl.py), written by
the reference's OWN binary (graph_classification/graph_kernels/gram.out).

Run on the authoring box only (needs the reference checkout), like the other make_golden_*.py:
    python tests/golden/make_golden_graph_kernels_kwl.py --gram-binary <reference>/graph_classification/graph_kernels/gram.out
Writes graph_kernels_kwl.json (data only): the text of `<ds>__<kernel>2_<h>.gram`, h = 0 .. 2, for `--k 2 --kernel WL | DWL | LWL |
LWLC --n_iters 2` on the five toy datasets of make_golden_graph_kernels.py (their arrays live in graph_kernels.json and are not
repeated) and, with its raw arrays, on

  TWOS    a one-node graph, a two-node graph with its edge, a two-node graph without it, a triangle with a pendant and an isolated
          node, and a five-leaf star with one chord (a name outside the binary's table: flags (true, true))
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden_graph_kernels import datasets as wl_datasets, write_tu  # noqa: E402
import kwl_ref  # noqa: E402
import wl_ref  # noqa: E402

N_ITERS = 2
KERNELS = ("WL", "DWL", "LWL", "LWLC")


def datasets():
    graphs = [(1, {}, [2]),
              (2, {(0, 1): 2}, [1, 2]),
              (2, {}, [1, 2]),
              (5, {(0, 1): 1, (1, 2): 2, (0, 2): 1, (2, 3): 3}, [1, 2, 2, 1, 3]),
              (6, {(0, 1): 1, (0, 2): 2, (0, 3): 1, (0, 4): 2, (0, 5): 1, (2, 3): 1}, [3, 1, 1, 2, 2, 1])]
    gi, A, nl, el, off = [], [], [], [], 0
    for g, (n, lab, labels) in enumerate(graphs, 1):
        for v, w in sorted([(v, w) for v, w in lab] + [(w, v) for v, w in lab]):
            A.append([off + v + 1, off + w + 1])
            el.append(lab[(min(v, w), max(v, w))])
        gi += [g] * n
        nl += labels
        off += n
    return [dict(name="TWOS", graph_indicator=gi, A=A, node_labels=nl, edge_labels=el, graph_labels=[0, 1, 1, 0, 1])]


def _assert_big_is_hard(ds):
    """DUMMY_BIG must wrap around 2^64 and make a new colour numerically below an old one at k = 2 as well."""
    graphs = wl_ref.read_graphs(ds["graph_indicator"], ds["A"], ds["node_labels"], ds["edge_labels"])
    wraps = below = 0

    def counting(a, b):
        nonlocal wraps
        wraps += (a * a + a + b if a >= b else a + b * b) > wl_ref.M64
        return wl_ref.pairing(a, b)

    kwl_ref.pairing = counting                                          # (the restatement's own pairing steps, counted)
    try:
        for G in graphs:
            cols = kwl_ref.colors(G, N_ITERS, "LWL")
            for h in range(1, N_ITERS + 1):
                old = set(x for row in cols[:h] for x in row)
                below += any(x not in old and x < max(old) for x in cols[h])
    finally:
        kwl_ref.pairing = wl_ref.pairing
    assert wraps > 0 and below > 0, (wraps, below)
    return wraps, below


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gram-binary", required=True)
    args = ap.parse_args()
    binary = os.path.abspath(args.gram_binary)
    out = {"n_iters": N_ITERS, "datasets": []}
    with tempfile.TemporaryDirectory() as tmp:
        data, gdir = os.path.join(tmp, "data"), os.path.join(tmp, "gram")
        os.makedirs(gdir)
        for own, ds in [(False, d) for d in wl_datasets()] + [(True, d) for d in datasets()]:
            write_tu(ds, data)
            if ds["name"] == "DUMMY_BIG":
                print("DUMMY_BIG: %d pairing steps wrap, %d graph-iterations make a new colour below an old one" % _assert_big_is_hard(ds))
            grams = {}
            for kernel in KERNELS:
                t0 = time.time()
                subprocess.check_call([binary, "--dataset_dir", data, "--gram_dir", gdir, "--k", "2", "--kernel", kernel,
                                       "--n_iters", str(N_ITERS), "--datasets", ds["name"]], stdout=subprocess.DEVNULL)
                print("%s %s: %.2f s" % (ds["name"], kernel, time.time() - t0))
                for h in range(N_ITERS + 1):
                    key = "%s2_%d" % (kernel, h)
                    with open(os.path.join(gdir, "%s__%s.gram" % (ds["name"], key))) as f:
                        grams[key] = f.read()
            out["datasets"].append(dict(ds, grams=grams) if own else dict(name=ds["name"], grams=grams))
    path = os.path.join(HERE, "graph_kernels_kwl.json")
    with open(path, "w") as f:
        json.dump(out, f, separators=(",", ":"))
    print(path, os.path.getsize(path), "bytes; graph_kernels.json has", os.path.getsize(os.path.join(HERE, "graph_kernels.json")))
    assert os.path.getsize(path) <= os.path.getsize(os.path.join(HERE, "graph_kernels.json"))


if __name__ == "__main__":
    main()
