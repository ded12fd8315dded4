"""Golden vectors for the 3-WL graph kernels (tests/test_graph_kernels_k3wl_host.py, tests/test_gpu_graph_kernels_k3wl.py), written
by the reference's OWN binary (graph_classification/graph_kernels/gram.out).

Run on the authoring box only (needs the reference checkout), like the other make_golden_*.py:
    python tests/golden/make_golden_graph_kernels_k3wl.py --gram-binary <reference>/graph_classification/graph_kernels/gram.out
Writes graph_kernels_k3wl.json (data only): the text of `<ds>__<kernel>3_<h>.gram`, h = 0 .. 2, for `--k 3 --kernel WL | DWL | LWL |
LWLC --n_iters 2` on the five toy datasets of make_golden_graph_kernels.py and TWOS of make_golden_graph_kernels_kwl.py (their arrays
live in graph_kernels.json / graph_kernels_kwl.json and are not repeated) and, with its raw arrays, on

  THREES  a one-node graph, an edgeless three-node graph, a triangle with a pendant, a hub joined to ten nodes with two chords (the
          dummy-node shape), and a six-node path with a chord; node labels near 2^63 and 2^64 - 1 (a name outside the binary's table:
          flags (true, true)) -- asserted below to wrap around 2^64 and to make a new colour below an old one

DUMMY_BIG costs the binary minutes at WL / DWL (an n^3-node tuple graph with 3 n^4 hash-map edges per graph); the text is 24 lines.
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
from make_golden_graph_kernels_kwl import datasets as kwl_datasets  # noqa: E402
import k3wl_ref  # noqa: E402
import wl_ref  # noqa: E402

N_ITERS = 2
KERNELS = ("WL", "DWL", "LWL", "LWLC")
B63, TOP = 1 << 63, (1 << 64) - 1


def datasets():
    hub = {(0, v): 0 for v in range(1, 11)}
    hub.update({(1, 2): 1, (4, 7): 2})
    graphs = [(1, {}, [TOP]),
              (3, {}, [1, B63, 1]),
              (4, {(0, 1): 1, (1, 2): 2, (0, 2): 1, (2, 3): 3}, [B63 - 1, 2, B63 + 1, TOP - 1]),
              (11, hub, [0, 1, 2, 1, 2, B63, 1, 2, TOP, 1, 1]),
              (6, {(0, 1): 1, (1, 2): 1, (2, 3): 2, (3, 4): 1, (4, 5): 1, (1, 4): 2}, [1, 2, TOP, 2, 1, B63])]
    gi, A, nl, el, off = [], [], [], [], 0
    for g, (n, lab, labels) in enumerate(graphs, 1):
        for v, w in sorted([(v, w) for v, w in lab] + [(w, v) for v, w in lab]):
            A.append([off + v + 1, off + w + 1])
            el.append(lab[(min(v, w), max(v, w))])
        gi += [g] * n
        nl += labels
        off += n
    return [dict(name="THREES", graph_indicator=gi, A=A, node_labels=nl, edge_labels=el, graph_labels=[0, 1, 1, 0, 1])]


def _assert_is_hard(ds):
    """THREES must wrap around 2^64 and make a new colour numerically below an old one at k = 3, under every kernel."""
    graphs = wl_ref.read_graphs(ds["graph_indicator"], ds["A"], ds["node_labels"], ds["edge_labels"])
    out = []
    for kernel in KERNELS:
        wraps = below = 0

        def counting(a, b):
            nonlocal wraps
            wraps += (a * a + a + b if a >= b else a + b * b) > wl_ref.M64
            return wl_ref.pairing(a, b)

        k3wl_ref.pairing = counting                                     # (the restatement's own pairing steps, counted)
        try:
            for G in graphs:
                cols = k3wl_ref.colors(G, N_ITERS, kernel)
                for h in range(1, N_ITERS + 1):
                    old = set(x for row in cols[:h] for x in row)
                    below += any(x not in old and x < max(old) for x in cols[h])
        finally:
            k3wl_ref.pairing = wl_ref.pairing
        assert wraps > 0 and below > 0, (kernel, wraps, below)
        out.append((kernel, wraps, below))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gram-binary", required=True)
    args = ap.parse_args()
    binary = os.path.abspath(args.gram_binary)
    out = {"n_iters": N_ITERS, "datasets": []}
    with tempfile.TemporaryDirectory() as tmp:
        data, gdir = os.path.join(tmp, "data"), os.path.join(tmp, "gram")
        os.makedirs(gdir)
        for own, ds in [(True, d) for d in datasets()] + [(False, d) for d in wl_datasets() + kwl_datasets()]:
            write_tu(ds, data)
            if own:
                for kernel, wraps, below in _assert_is_hard(ds):
                    print("%s %s: %d pairing steps wrap, %d graph-iterations make a new colour below an old one"
                          % (ds["name"], kernel, wraps, below))
            grams = {}
            for kernel in KERNELS:
                t0 = time.time()
                subprocess.check_call([binary, "--dataset_dir", data, "--gram_dir", gdir, "--k", "3", "--kernel", kernel,
                                       "--n_iters", str(N_ITERS), "--datasets", ds["name"]], stdout=subprocess.DEVNULL)
                print("%s %s: %.2f s" % (ds["name"], kernel, time.time() - t0), flush=True)
                for h in range(N_ITERS + 1):
                    key = "%s3_%d" % (kernel, h)
                    with open(os.path.join(gdir, "%s__%s.gram" % (ds["name"], key))) as f:
                        grams[key] = f.read()
            out["datasets"].append(dict(ds, grams=grams) if own else dict(name=ds["name"], grams=grams))
    path = os.path.join(HERE, "graph_kernels_k3wl.json")
    with open(path, "w") as f:
        json.dump(out, f, separators=(",", ":"))
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) <= (1 << 20)


if __name__ == "__main__":
    main()
