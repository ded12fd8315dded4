"""Golden vectors for the SP and GR graph kernels (tests/test_graph_kernels_spgr_host.py, tests/test_gpu_graph_kernels_spgr.py),
written by the reference's OWN binary (graph_classification/graph_kernels/gram.out).

Run on the authoring box only (needs the reference checkout), like the other make_golden_*.py:
    python tests/golden/make_golden_graph_kernels_spgr.py --gram-binary <reference>/graph_classification/graph_kernels/gram.out
Writes graph_kernels_spgr.json (data only): the text of `<ds>__SP_0.gram` and `<ds>__GR_0.gram` for the five toy datasets of
make_golden_graph_kernels.py (their arrays live in graph_kernels.json and are not repeated) and, with their raw arrays, for

  EDGES    a 300-node path, a 2-node graph, a 1-node graph, an edgeless 3-node graph, random graphs of 63, 64 and 65 nodes,
           dummy-augmented graphs of 65 and 128 nodes (dummy label 0, dummy edges labelled 0), a 70-node star with chords (hub
           degree 69, triangles at the hub) and a K4 with mixed node and edge labels
  LABELS   small graphs with node labels drawn from {0, 1, 2147483647, 2^32, 2^32 + 1, 2^63, 2^64 - 1}

Both names are outside the binary's table, so their flags are (true, true).
"""
import argparse
import json
import os
import random
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden_graph_kernels import datasets as wl_datasets, write_tu  # noqa: E402

SPECIAL = [0, 1, 2147483647, 1 << 32, (1 << 32) + 1, 1 << 63, (1 << 64) - 1]


def _pack(name, graphs, classes):
    """graphs: (n, {(v, w): edge label} with v < w, node labels) -> the raw TU arrays, both directions of every edge in sorted order."""
    gi, A, nl, el, off = [], [], [], [], 0
    for g, (n, lab, labels) in enumerate(graphs, 1):
        for v, w in sorted([(v, w) for v, w in lab] + [(w, v) for v, w in lab]):
            A.append([off + v + 1, off + w + 1])
            el.append(lab[(min(v, w), max(v, w))])
        gi += [g] * n
        nl += labels
        off += n
    return dict(name=name, graph_indicator=gi, A=A, node_labels=nl, edge_labels=el, graph_labels=classes)


def _random(rng, n, p, node_vocab, edge_vocab, dummy=False):
    m = n - 1 if dummy else n
    lab = {(v, w): rng.randint(1, edge_vocab) for v in range(m) for w in range(v + 1, m) if rng.random() < p}
    labels = [rng.randint(1, node_vocab) for _ in range(m)]
    if dummy:
        lab.update({(v, m): 0 for v in range(m)})
        labels.append(0)
    return n, lab, labels


def datasets():
    rng = random.Random(20240702)
    g = []
    g.append((300, {(v, v + 1): 1 + v % 2 for v in range(299)}, [1 + v % 3 for v in range(300)]))
    g.append((2, {(0, 1): 1}, [1, 2]))
    g.append((1, {}, [2]))
    g.append((3, {}, [1, 1, 3]))
    for n in (63, 64, 65):
        g.append(_random(rng, n, 0.06, 3, 2))
    g.append(_random(rng, 65, 0.06, 3, 2, dummy=True))
    g.append(_random(rng, 128, 0.04, 3, 2, dummy=True))
    star = {(0, v): 1 + v % 2 for v in range(1, 70)}
    star.update({(3, 4): 1, (4, 5): 2, (3, 5): 1, (10, 40): 1, (68, 69): 2})
    g.append((70, star, [2] + [1 + v % 3 for v in range(1, 70)]))
    g.append((4, {(0, 1): 1, (0, 2): 2, (0, 3): 3, (1, 2): 1, (1, 3): 2, (2, 3): 1}, [1, 2, 2, 3]))
    out = [_pack("EDGES", g, [i % 2 for i in range(len(g))])]
    g = []
    for n in (3, 4, 5, 6, 7, 5, 6, 4, 7, 3):
        m, lab, _ = _random(rng, n, 0.55, 1, 2)
        g.append((m, lab, [rng.choice(SPECIAL) for _ in range(n)]))
    out.append(_pack("LABELS", g, [i % 2 for i in range(len(g))]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gram-binary", required=True)
    args = ap.parse_args()
    binary = os.path.abspath(args.gram_binary)
    out = {"datasets": []}
    with tempfile.TemporaryDirectory() as tmp:
        data, gdir = os.path.join(tmp, "data"), os.path.join(tmp, "gram")
        os.makedirs(gdir)
        for own, ds in [(False, d) for d in wl_datasets()] + [(True, d) for d in datasets()]:
            write_tu(ds, data)
            grams = {}
            for kernel in ("SP", "GR"):
                subprocess.check_call([binary, "--dataset_dir", data, "--gram_dir", gdir, "--k", "1", "--kernel", kernel,
                                       "--n_iters", "3", "--datasets", ds["name"]])
                with open(os.path.join(gdir, "%s__%s_0.gram" % (ds["name"], kernel))) as f:
                    grams[kernel + "_0"] = f.read()
            out["datasets"].append(dict(ds, grams=grams) if own else dict(name=ds["name"], grams=grams))
    path = os.path.join(HERE, "graph_kernels_spgr.json")
    with open(path, "w") as f:
        json.dump(out, f, separators=(",", ":"))
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
