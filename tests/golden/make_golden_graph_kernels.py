"""Golden vectors for the WL / WLOA graph kernels (tests/test_graph_kernels_host.py, tests/test_gpu_graph_kernels.py), written by
the reference's OWN binary (graph_classification/graph_kernels/gram.out).

Run on the authoring box only (needs the reference checkout), like the other make_golden_*.py:
    python tests/golden/make_golden_graph_kernels.py --gram-binary <reference>/graph_classification/graph_kernels/gram.out
Writes graph_kernels.json (data only): per seeded toy TU dataset its raw arrays and the text of every .gram file the binary wrote
for `--k 1 --kernel WL` and `--kernel WLOA` at `--n_iters 4`.

  TOYA            six graphs of 3..6 nodes, node and edge labels (a name outside the binary's table: flags (true, true))
  DUMMY_BIG       24 random graphs of 2..40 nodes with node and edge labels, each with a dummy node (label 0) joined to every other
                  node by edges labelled 0 -- asserted below to wrap around 2^64 and to make a new colour below an old one
  NCI1            a table name with flags (true, false): node labels only
  REDDIT-BINARY   a table name with flags (false, false): no label files at all
  QUIRKS          an isolated node, a one-node graph, a repeated `A` line, a pair whose two directions carry different labels
"""
import argparse
import json
import os
import random
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import wl_ref  # noqa: E402

N_ITERS = 4


def _random_graphs(rng, sizes, p, node_vocab, edge_vocab, dummy=False):
    gi, A, nl, el, off = [], [], [], [], 0
    for g, n in enumerate(sizes, 1):
        pairs = [(v, w) for v in range(n) for w in range(v + 1, n) if rng.random() < p]
        if not pairs and n > 1:
            pairs = [(0, 1)]
        labels = [rng.randint(1, node_vocab) for _ in range(n)]
        lab = {e: rng.randint(1, edge_vocab) for e in pairs}
        if dummy:
            for v in range(n):
                lab[(v, n)] = 0
            pairs = pairs + [(v, n) for v in range(n)]
            labels.append(0)
            n += 1
        directed = sorted([(v, w) for v, w in pairs] + [(w, v) for v, w in pairs])
        for v, w in directed:
            A.append([off + v + 1, off + w + 1])
            el.append(lab[(min(v, w), max(v, w))])
        gi += [g] * n
        nl += labels
        off += n
    return gi, A, nl, el


def datasets():
    rng = random.Random(20240611)
    out = []
    gi, A, nl, el = _random_graphs(rng, [3, 4, 5, 6, 4, 6], 0.6, 3, 2)
    out.append(dict(name="TOYA", graph_indicator=gi, A=A, node_labels=nl, edge_labels=el, graph_labels=[1, 0, 1, 1, 0, 0]))
    sizes = [2, 40] + [rng.randint(2, 40) for _ in range(22)]
    gi, A, nl, el = _random_graphs(rng, sizes, 0.15, 4, 3, dummy=True)
    out.append(dict(name="DUMMY_BIG", graph_indicator=gi, A=A, node_labels=nl, edge_labels=el,
                    graph_labels=[rng.randint(0, 1) for _ in sizes]))
    gi, A, nl, el = _random_graphs(rng, [5, 7, 9, 6, 8, 12, 4, 10], 0.35, 5, 1)
    out.append(dict(name="NCI1", graph_indicator=gi, A=A, node_labels=nl, edge_labels=None, graph_labels=[0, 1, 1, 0, 1, 0, 0, 1]))
    gi, A, nl, el = _random_graphs(rng, [6, 9, 5, 11, 7, 8, 10], 0.4, 1, 1)
    out.append(dict(name="REDDIT-BINARY", graph_indicator=gi, A=A, node_labels=None, edge_labels=None,
                    graph_labels=[1, -1, 1, -1, -1, 1, 1]))
    # QUIRKS, nodes 1-based: graph 1 = {1,2,3,4} with 4 isolated, the line 1,2 repeated and 2,1 / 2,3 / 3,2 labelled differently;
    # graph 2 = {5} alone; graph 3 = {6,7,8} a path given in one direction only; graph 4 = {9,10} whose two directions disagree
    A = [[1, 2], [2, 1], [1, 2], [2, 3], [3, 2], [6, 7], [7, 8], [9, 10], [10, 9]]
    el = [1, 2, 3, 2, 1, 1, 2, 2, 1]
    out.append(dict(name="QUIRKS", graph_indicator=[1, 1, 1, 1, 2, 3, 3, 3, 4, 4], A=A, node_labels=[1, 2, 1, 3, 2, 1, 1, 2, 3, 3],
                    edge_labels=el, graph_labels=[0, 1, 0, 1]))
    return out


def write_tu(ds, root):
    d = os.path.join(root, ds["name"])
    os.makedirs(d, exist_ok=True)

    def put(kind, lines):
        with open(os.path.join(d, "%s_%s.txt" % (ds["name"], kind)), "w") as f:
            f.write("".join("%s\n" % ln for ln in lines))

    put("graph_indicator", ds["graph_indicator"])
    put("A", ["%d, %d" % (v, w) for v, w in ds["A"]])
    put("graph_labels", ds["graph_labels"])
    if ds["node_labels"] is not None:
        put("node_labels", ds["node_labels"])
    if ds["edge_labels"] is not None:
        put("edge_labels", ds["edge_labels"])


def _assert_big_is_hard(ds):
    """DUMMY_BIG must exercise wrap-around and the ordering quirk (a new colour numerically below an old one)."""
    graphs = wl_ref.read_graphs(ds["graph_indicator"], ds["A"], ds["node_labels"], ds["edge_labels"])
    wraps = below = 0
    for G in graphs:
        cols = wl_ref.colors(G, N_ITERS)
        for h in range(1, N_ITERS + 1):
            for v in range(G["n"]):
                c = cols[h - 1][v]
                ent = []
                for w in G["nbrs"][v]:
                    a, b = cols[h - 1][w], G["elabel"][(v, w)]
                    wraps += (a * a + a + b if a >= b else a + b * b) > wl_ref.M64
                    ent += [wl_ref.pairing(a, b), a]
                for e in sorted(ent):
                    wraps += (c * c + c + e if c >= e else c + e * e) > wl_ref.M64
                    c = wl_ref.pairing(c, e)
            old = set(x for row in cols[:h] for x in row)
            below += any(x not in old and x < max(old) for x in cols[h])
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
        for ds in datasets():
            write_tu(ds, data)
            if ds["name"] == "DUMMY_BIG":
                print("DUMMY_BIG: %d pairing steps wrap, %d graph-iterations make a new colour below an old one" % _assert_big_is_hard(ds))
            grams = {}
            for kernel, stem in (("WL", "WL1"), ("WLOA", "WLOA")):
                subprocess.check_call([binary, "--dataset_dir", data, "--gram_dir", gdir, "--k", "1", "--kernel", kernel,
                                       "--n_iters", str(N_ITERS), "--datasets", ds["name"]])
                for h in range(N_ITERS + 1):
                    key = "%s_%d" % (stem, h)
                    with open(os.path.join(gdir, "%s__%s.gram" % (ds["name"], key))) as f:
                        grams[key] = f.read()
            out["datasets"].append(dict(ds, grams=grams))
    path = os.path.join(HERE, "graph_kernels.json")
    with open(path, "w") as f:
        json.dump(out, f, separators=(",", ":"))
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
