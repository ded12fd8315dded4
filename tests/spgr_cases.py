"""Datasets and reference results shared by the SP / GR graph-kernel tests: the goldens (tests/golden/graph_kernels_spgr.json, whose
first five datasets take their arrays from graph_kernels.json), seeded datasets at the kernels' class boundaries, the restatement's
results computed once per dataset and flags (tests/spgr_ref.py), and readers of a feature CSR."""
import functools
import json
import os
import random

import spgr_ref
import wl_cases as C
import wl_ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "graph_kernels_spgr.json")
# what the binary's table says about the goldens' names (gram.cpp:17-36; names outside it get (true, true))
FLAGS = {"TOYA": (True, True), "DUMMY_BIG": (True, True), "NCI1": (True, False), "REDDIT-BINARY": (False, False), "QUIRKS": (True, True),
         "EDGES": (True, True), "LABELS": (True, True)}
M64 = (1 << 64) - 1
M32 = (1 << 32) - 1
# EDGES, graph by graph (tests/golden/make_golden_graph_kernels_spgr.py)
EDGES_PATH, EDGES_PAIR, EDGES_SINGLE, EDGES_EDGELESS, EDGES_STAR, EDGES_K4 = 0, 1, 2, 3, 9, 10
EDGES_SIZES = [300, 2, 1, 3, 63, 64, 65, 65, 128, 70, 4]


@functools.lru_cache(maxsize=None)
def golden():
    with open(GOLDEN) as f:
        g = json.load(f)
    wl = C.golden()[1]
    return {d["name"]: (d if "A" in d else dict(wl[d["name"]], grams=d["grams"])) for d in g["datasets"]}


def gr_degrees():
    """Stars with chords whose centre degrees sit at the boundaries of the GR launches: 8 pairs lie between degrees 4 (6 pairs) and 5
    (10), 64 pairs between 11 (55) and 12 (66), and a hub's rows are cut into work items of about 2048 pairs: degree 64 (2016 pairs)
    is one item, 65 (2080) two, 100 (4950) three."""
    rng = random.Random(91)
    degs = [0, 1, 2, 3, 4, 5, 6, 10, 11, 12, 13, 64, 65, 100]
    return C.assemble("DEGREES", [C.star(rng, d, [1, 2, 3, (1 << 63) + 5, (1 << 64) - 1], [0, 1, 5, (1 << 32) - 1]) for d in degs])


def sp_sizes(sizes, name):
    """Sparse random graphs of the given sizes (about three neighbours per node: a giant component of a dozen levels, small ones
    and isolated nodes beside it)."""
    rng = random.Random(sum(sizes))
    graphs = []
    for n in sizes:
        pairs = sorted(set((min(v, w), max(v, w)) for v, w in ((rng.randrange(n), rng.randrange(n)) for _ in range(3 * n // 2)) if v != w))
        graphs.append((n, pairs, [rng.choice([0, 1, 2, 3]) for _ in range(n)], {e: 1 for e in pairs}))
    return C.assemble(name, graphs)


_REF = {}


def graphs(ds):
    if ds["name"] not in _REF:
        _REF[ds["name"]] = wl_ref.read_graphs(ds["graph_indicator"], ds["A"], ds["node_labels"], ds["edge_labels"])
    return _REF[ds["name"]]


def ref_sp(ds, use_nl):
    """(per-graph {(lo32(l_a), l_b, d): count}, gram matrix) of the restatement, computed once."""
    key = (ds["name"], "SP", use_nl)
    if key not in _REF:
        feats = [spgr_ref.sp_features(G, use_nl) for G in graphs(ds)]
        _REF[key] = (feats, spgr_ref.gram(feats))
    return _REF[key]


def ref_gr(ds, use_nl, use_el):
    key = (ds["name"], "GR", use_nl, use_el)
    if key not in _REF:
        feats = [spgr_ref.gr_features(G, use_nl, use_el) for G in graphs(ds)]
        _REF[key] = (feats, spgr_ref.gram(feats))
    return _REF[key]


def rows(f):
    """A feature CSR as one list of (unsigned key, count) per graph, after checking its shape: keys strictly ascending, one step."""
    ptr, col, cnt, step = f.ptr.cpu().tolist(), [x & M64 for x in f.color.cpu().tolist()], f.count.cpu().tolist(), f.step.cpu().tolist()
    assert f.num_steps == 1 and not any(step) and ptr[0] == 0 and ptr[-1] == len(col) == len(cnt)
    out = []
    for a, b in zip(ptr, ptr[1:]):
        assert all(x < y for x, y in zip(col[a:b], col[a + 1:b])) and all(c > 0 for c in cnt[a:b])
        out.append(list(zip(col[a:b], cnt[a:b])))
    assert f.max_row == max(len(r) for r in out)
    return out


def sp_decode(ds, use_nl, f):
    """The SP feature CSR as per-graph {(lo32(l_a), l_b, d): count}: a key's high half is rank(lo32(l_a)) * #labels + rank(l_b)."""
    labels = [int(x) & M64 for x in ds["node_labels"]] if use_nl else [1]
    ua, ub = sorted(set(x & M32 for x in labels)), sorted(set(labels))
    return [{(ua[(k >> 32) // len(ub)], ub[(k >> 32) % len(ub)], k & M32): c for k, c in r} for r in rows(f)]
