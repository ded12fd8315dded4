"""Datasets shared by the graph-kernel tests: the goldens (tests/golden/graph_kernels.json, written by the reference's binary), a
TU-format writer, and seeded raw arrays in the goldens' layout {name, graph_indicator, A, node_labels, edge_labels, graph_labels}.
The restatement's results are computed once per dataset and flags and shared (tests/wl_ref.py)."""
import functools
import json
import os
import random

import wl_ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "graph_kernels.json")
BIG_LABELS = [1, 2, 3, (1 << 63) - 1, 1 << 63, (1 << 63) + 1, (1 << 64) - 2, (1 << 64) - 1]


@functools.lru_cache(maxsize=None)
def golden():
    with open(GOLDEN) as f:
        g = json.load(f)
    return g["n_iters"], {d["name"]: d for d in g["datasets"]}


def write_tu(ds, root, raw=False):
    d = os.path.join(root, ds["name"], "raw") if raw else os.path.join(root, ds["name"])
    os.makedirs(d, exist_ok=True)
    cols = {"graph_indicator": ds["graph_indicator"], "A": ["%d, %d" % (v, w) for v, w in ds["A"]], "graph_labels": ds["graph_labels"],
            "node_labels": ds["node_labels"], "edge_labels": ds["edge_labels"]}
    for kind, lines in cols.items():
        if lines is not None:
            with open(os.path.join(d, "%s_%s.txt" % (ds["name"], kind)), "w") as f:
                f.write("".join("%s\n" % ln for ln in lines))


def assemble(name, graphs):
    """graphs: [(n, [(v, w), ...] undirected pairs, node labels, {pair: edge label})] -> raw arrays (both directions, sorted)."""
    gi, A, nl, el, off = [], [], [], [], 0
    for g, (n, pairs, labels, elab) in enumerate(graphs, 1):
        for v, w in sorted([(v, w) for v, w in pairs] + [(w, v) for v, w in pairs]):
            A.append([off + v + 1, off + w + 1])
            el.append(elab[(min(v, w), max(v, w))])
        gi += [g] * n
        nl += list(labels)
        off += n
    return dict(name=name, graph_indicator=gi, A=A, node_labels=nl, edge_labels=el, graph_labels=[g % 2 for g in range(len(graphs))])


def random_graph(rng, n, p, node_labels, edge_labels):
    pairs = [(v, w) for v in range(n) for w in range(v + 1, n) if rng.random() < p]
    return n, pairs, [rng.choice(node_labels) for _ in range(n)], {e: rng.choice(edge_labels) for e in pairs}


def star(rng, deg, node_labels, edge_labels):
    """A centre (node 0) with `deg` leaves and a few chords among the first leaves: the centre's entry list has deg entries (2 deg
    with edge labels)."""
    pairs = [(0, v) for v in range(1, deg + 1)]
    k = min(deg, 10)
    pairs += [(v, w) for v in range(1, k + 1) for w in range(v + 1, k + 1) if rng.random() < 0.3]
    return deg + 1, pairs, [rng.choice(node_labels) for _ in range(deg + 1)], {e: rng.choice(edge_labels) for e in pairs}


def stars(cap):
    """Centre degrees at the sort's boundaries.  Without edge labels the entry count is the degree: 0, 1, 63, 64, 65, 127, 128, 129,
    cap - 1, cap, cap + 1.  With edge labels it is 2 deg, which is always even: 64, 128 and cap are reached exactly (deg 32, 64,
    cap / 2) and every odd boundary is bracketed by its two even neighbours (0 and 2; 62 and 66; 126 and 130; cap - 2 and cap + 2).
    Labels near 2^63 and 2^64 - 1 make the order unsigned and the very first pairing wrap."""
    rng = random.Random(77)
    degs = [0, 1, 31, 32, 33, 63, 64, 65, 127, 128, 129, cap // 2 - 1, cap // 2, cap // 2 + 1, cap - 1, cap, cap + 1]
    return assemble("STARS", [star(rng, d, BIG_LABELS, [0, 1, 5, (1 << 32) - 1]) for d in degs])


def mixed(count, seed=5, lo=1, hi=14):
    """`count` small random graphs (node labels from a small vocabulary so that graphs share colours, with two huge ones mixed in)."""
    rng = random.Random(seed)
    return assemble("MIXED%d" % count, [random_graph(rng, rng.randint(lo, hi), 0.3, [1, 2, 3, (1 << 63) + 5, (1 << 64) - 1], [1, 2])
                                        for _ in range(count)])


def take(ds, count):
    """The first `count` graphs of a dataset."""
    gi = ds["graph_indicator"]
    n = sum(1 for g in gi if g <= count)
    keep = [i for i, (v, w) in enumerate(ds["A"]) if v <= n]
    pick = lambda col: None if col is None else [col[i] for i in keep]  # noqa: E731
    return dict(name="%s_%d" % (ds["name"], count), graph_indicator=gi[:n], A=[ds["A"][i] for i in keep],
                node_labels=None if ds["node_labels"] is None else ds["node_labels"][:n], edge_labels=pick(ds["edge_labels"]),
                graph_labels=ds["graph_labels"][:count])


_REF = {}


def ref(ds, H, use_nl, use_el):
    """The restatement on a dataset: (graphs, colours per graph, features per graph), computed once per (name, H, flags)."""
    key = (ds["name"], H, use_nl, use_el)
    if key not in _REF:
        if ds["name"] not in _REF:
            _REF[ds["name"]] = wl_ref.read_graphs(ds["graph_indicator"], ds["A"], ds["node_labels"], ds["edge_labels"])
        graphs = _REF[ds["name"]]
        cols = [wl_ref.colors(G, H, use_nl, use_el) for G in graphs]
        _REF[key] = (graphs, cols, [wl_ref.features(c) for c in cols])
    return _REF[key]
