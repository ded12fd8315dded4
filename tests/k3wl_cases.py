"""Datasets shared by the 3-WL graph-kernel tests: the goldens (tests/golden/graph_kernels_k3wl.json, written by the reference's
binary; the arrays of the five k = 1 toy datasets come from graph_kernels.json, those of TWOS from graph_kernels_kwl.json) and seeded
graphs at the boundaries of the kernels' classes.  The restatement's colours (tests/k3wl_ref.py) are computed once per dataset, kernel
and flags and shared."""
import functools
import json
import os
import random

import k3wl_ref
import kwl_cases
import wl_cases
import wl_ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "graph_kernels_k3wl.json")
KERNELS = k3wl_ref.KERNELS
flags = kwl_cases.flags                                                    # gram.cpp:17-36; a name outside the table: (True, True)
SMALL_GOLDENS = ["TOYA", "NCI1", "REDDIT-BINARY", "QUIRKS", "TWOS", "THREES"]


@functools.lru_cache(maxsize=None)
def golden():
    """(n_iters, {name: dataset with its raw arrays and its `grams` {"<kernel>3_<h>": text}})."""
    with open(GOLDEN) as f:
        g = json.load(f)
    arrays = dict(wl_cases.golden()[1])
    arrays["TWOS"] = kwl_cases.golden()[1]["TWOS"]
    out = {}
    for d in g["datasets"]:
        out[d["name"]] = d if "graph_indicator" in d else dict(arrays[d["name"]], grams=d["grams"])
    return g["n_iters"], out


_REF = {}


def graphs_of(ds):
    if ds["name"] not in _REF:
        _REF[ds["name"]] = wl_ref.read_graphs(ds["graph_indicator"], ds["A"], ds["node_labels"], ds["edge_labels"])
    return _REF[ds["name"]]


def ref(ds, H, kernel, use_nl=True, use_el=True):
    """(graphs, [colours [H + 1][items] per graph]) of the restatement, computed once."""
    key = (ds["name"], H, kernel, use_nl, use_el)
    if key not in _REF:
        graphs = graphs_of(ds)
        _REF[key] = (graphs, [k3wl_ref.colors(G, H, kernel, use_nl, use_el) for G in graphs])
    return _REF[key]


def flat(cols, h):
    """The colours of iteration h of all graphs, graph after graph."""
    return [x for c in cols for x in c[h]]


def _hub(rng, n, chords=8):
    """A hub (node 0) joined to all n - 1 others, and a few chords among the first leaves."""
    pairs = [(0, v) for v in range(1, n)]
    k = min(n - 1, chords)
    pairs += [(v, w) for v in range(1, k + 1) for w in range(v + 1, k + 1) if rng.random() < 0.3]
    return n, pairs, [rng.choice([1, 2, (1 << 63) + 1]) for _ in range(n)], {e: rng.choice([0, 1, 2]) for e in pairs}


@functools.lru_cache(maxsize=None)
def small_bounds():
    """Graphs of 1, 2, 8 and 9 nodes (either side of the 8-lane fibres of the WL / DWL kernel), random and sparse, with labels near
    2^63 and 2^64 - 1, an edgeless graph, and hubs of degree 7, 8 and 9 (either side of the 8-lane lists of LWL; LWLC's merged list
    of a hub item is about twice the degree, so these also cross into the wavefront class)."""
    rng = random.Random(3024)
    g = [wl_cases.random_graph(rng, n, 0.3, wl_cases.BIG_LABELS, [0, 1, (1 << 32) - 1]) for n in (1, 2, 8, 9)]
    g.append((3, [], [1, 1, 2], {}))
    g += [_hub(rng, n) for n in (8, 9, 10)]
    return wl_cases.assemble("K3WL_SMALL", g)


@functools.lru_cache(maxsize=None)
def mid_bounds():
    """16 and 17 nodes: the last graph of the 16-lane fibres and the first of the 32-lane ones."""
    rng = random.Random(3025)
    return wl_cases.assemble("K3WL_MID", [wl_cases.random_graph(rng, n, 0.25, wl_cases.BIG_LABELS, [1]) for n in (16, 17)])


@functools.lru_cache(maxsize=None)
def wave_bounds():
    """Hubs of degree 63, 64 and 65: 64, 65 and 66 nodes -- either side of the wavefront lists of LWL / LWLC and of the largest graph
    of the WL / DWL kernel -- and a random 33-node graph (the first size of the 64-lane fibres)."""
    rng = random.Random(3026)
    g = [_hub(rng, n) for n in (64, 65, 66)]
    g.append(wl_cases.random_graph(rng, 33, 0.1, [1, 2, 3], [1, 2]))
    return wl_cases.assemble("K3WL_WAVE", g)


@functools.lru_cache(maxsize=None)
def limit_bounds(max_nodes):
    """Sparse random graphs of max_nodes and max_nodes + 1 nodes between two small ones: the WL / DWL kernel's largest graph and the
    first one that takes the composed path, inside one dataset."""
    rng = random.Random(3027)
    g = [wl_cases.random_graph(rng, n, p, [1, 2, 3], [1, 2]) for n, p in ((5, 0.5), (max_nodes, 0.04), (max_nodes + 1, 0.04), (7, 0.4))]
    return wl_cases.assemble("K3WL_LIMIT", g)


@functools.lru_cache(maxsize=None)
def hub_bounds(max_entries):
    """LWLC only (n^3 triples would pass the MAXNUMCOLOR bound): hubs of degree max_entries - 1, max_entries and max_entries + 1 --
    the largest degree of the workgroup kernel and the first graph that takes the composed path -- next to a small graph."""
    rng = random.Random(3028)
    g = [_hub(rng, max_entries + d, chords=4) for d in (0, 1, 2)]
    g.append(wl_cases.random_graph(rng, 6, 0.5, [1, 2], [1]))
    return wl_cases.assemble("K3WL_HUB", g)
