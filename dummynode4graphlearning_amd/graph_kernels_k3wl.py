"""The 3-WL graph kernels, computed on the device: the counterpart of the reference's graph-kernel tool at `gram --k 3 --kernel WL |
DWL | LWL | LWLC` (graph_classification/graph_kernels), for the datasets graph_kernels.GraphKernelData reads.

  tuple graphs           src/GenerateThree.cpp:835, :987, :1229, :1376                never built: gathers from a graph's own colour
                                                                                       cube, selected by the dataset CSR
  initial colours        the same (the tuple graph's node labels)                      dn_k3wl.hip: dn_k3wl_init_u64
  refinement             GenerateThree::compute_colors_simple, :477-833                k3wl_colors (dn_k3wl_local_u64 / dn_k3wl_global_u64
                                                                                       + dn_k3wl_close_u64)
  colour maps, matrices  :65-137, gram.cpp:252-308                                     k3wl_features / k3wl_gram_matrices (the k = 1 WL
                                                                                       feature build and dn_wl_gram_i64)
  command line           gram.cpp:38-104                                               python -m dummynode4graphlearning_amd.graph_kernels_k3wl

The items are node triples (i, j, k) of one graph: all n^3 of them, row-major (WL, DWL, LWL), or, for LWLC, (i, i, i) for every i, then
(i, i, j) for every adjacent ordered pair, then the pairwise distinct (i, j, k) with at least two of the three pairs adjacent.  A
triple (v, w, u) has up to six neighbour multisets of the previous colours C: exchange 1 gives C[x, w, u], exchange 2 C[v, x, u],
exchange 3 C[v, w, x]; LWL / LWLC let x run over the neighbours of the exchanged node (local; LWLC keeps the x for which the triple is
an item and puts exchanges 1 and 2 into ONE multiset), WL over all nodes (local), DWL over all nodes with the neighbours local and the
rest global.  As at k = 2 the reference's tuple graph is undirected and its add_edge pushes both ends: every neighbour colour enters
its multiset TWICE, and in WL / DWL all three exchange loops reach the triple itself, the edge-type map keeps the first insertion and
each of the three self add_edge calls pushes twice, so the triple's own colour enters multiset 1 SIX times (DWL: the global one).  A
multiset is sorted ascending (unsigned) and folded with the pairing function starting from its maximum; the new colour is the old one
folded over the sorted local folds, then the sorted global folds.  Edge labels enter nowhere: the flag is accepted and ignored.
tests/k3wl_ref.py restates all of this in plain Python and tests/golden/graph_kernels_k3wl.json holds the text the reference's own
binary wrote.

Paths.  The fused kernels (ops.k3wl_fused(True)) take every graph within their limits: ops.k3wl_max_nodes() nodes for WL / DWL (a
group of lanes per fibre of the colour cube), ops.k3wl_max_entries() for the largest degree of a graph for LWL / LWLC.  Larger graphs,
and every graph under ops.k3wl_fused(False), take the composed path: the multiset entries of a run of triples are built with torch
device ops, sorted device-wide by (multiset, colour) and folded by dn_wl_fold_u64, at most `workspace_keys` entries at a time.  Item
lists, classes and chunks are built once per dataset on the host; a refinement reads nothing back.

The plan, the checks, the composed step and the drivers are graph_kernels_kwl's engine at k = 3; this module holds what is k = 3's own
(_K3): the LWLC item enumeration, the pair-code initial colours, and the arrays and launches of the dn_k3wl_* kernels.

Refused with ValueError: what graph_kernels refuses, a graph whose item count times (H + 1) reaches 1,000,000 (the reference's
MAXNUMCOLOR early stop, `color_nums[h - 1] < MAXNUMCOLOR` here, is not built), and a dataset with 2^31 - 1 items or more.  The kernels
LWLP / LWLPC are not built: the reference dereferences color_map_1 / _2 / _3.find(...) on maps that are empty or keyed by other values
(GenerateThree.cpp:641-645, 702-729), so their output is whatever lies behind end().  GenerateThreeSampling and `simple = false`
cannot be reached from gram.cpp and are not built.
"""
import os
import sys

import numpy as np
import torch

from . import graph_kernels as gk
from . import graph_kernels_kwl as engine
from . import ops
from .graph_kernels import MAXNUMCOLOR, GraphKernelData, WLFeatures, dataset_flags, write_libsvm  # noqa: F401
from .graph_kernels_kwl import KERNELS, _member

K3WL_WORKSPACE_KEYS = 1 << 24         # multiset entries of one composed chunk (a handful of int64 arrays of that length live at once)


def _ragged(count):
    """(owner of every item, its position within its owner) for count.sum() items (numpy)."""
    owner = np.repeat(np.arange(count.size), count)
    start = np.cumsum(count) - count
    return owner, np.arange(int(count.sum())) - start[owner]


class _K3:
    """What is k = 3's own (see "The engine" in graph_kernels_kwl)."""
    k, noun, cache, keyed = 3, "items", "_k3wl_plans", ("triple", "(a N + b) N + c")
    multisets = {False: (0, 1, 2), True: (0, 0, 1)}                         # the multiset of every exchange; LWLC: 1 and 2 share one
    max_nodes, max_entries = staticmethod(lambda: ops.k3wl_max_nodes()), staticmethod(lambda: ops.k3wl_max_entries())
    fused_enabled = staticmethod(lambda kernel: ops.k3wl_fused_enabled(kernel))

    @staticmethod
    def too_many(p, count, H):
        if count * (H + 1) >= MAXNUMCOLOR:
            return "%s%d items, times (H + 1) = %d that reaches %d" % ("at least " if p.lower_bound else "", count, H + 1, MAXNUMCOLOR)

    @staticmethod
    def connected_items(p, g):
        """LWLC: per graph (i, i, i), then (i, i, j) for adjacent (i, j), then the distinct triples with two adjacent pairs, each family
        by key.  (count, None, True) where a lower bound on the count is refused already, before any item is built."""
        N, B, ptr, nbr, deg, sizes, node_graph = g.N, g.B, g.ptr, g.nbr, g.deg, g.sizes, g.node_graph
        edges_of = ptr[g.node_ptr[1:]] - ptr[g.node_ptr[:-1]]
        wedges = np.zeros(B, dtype=np.int64)
        np.add.at(wedges, node_graph, deg * (deg - 1))                      # (centre, ordered pair of its neighbours)
        lower = sizes + edges_of + (wedges + 2) // 3                        # an item of the third family has at most three centres
        if int(lower.max()) >= MAXNUMCOLOR or int(lower.sum()) >= (1 << 31) - 1:
            return lower, None, True
        # the third family: every placement of a centre among an ordered pair of its neighbours; a triangle comes from 3 centres
        c, pos = _ragged(deg * deg)
        a, b = nbr[ptr[c] + pos // np.maximum(deg[c], 1)], nbr[ptr[c] + pos % np.maximum(deg[c], 1)]
        keep = a != b
        c, a, b = c[keep], a[keep], b[keep]
        slot_node = np.repeat(np.arange(N), deg)
        fam = np.concatenate([np.zeros(N, np.int64), np.ones(nbr.size, np.int64), np.full(3 * c.size, 2, np.int64)])
        v = np.concatenate([np.arange(N), slot_node, c, a, a])
        w = np.concatenate([np.arange(N), slot_node, a, c, b])
        u = np.concatenate([np.arange(N), nbr, b, b, c])
        gr, n_i, f_i = node_graph[v], sizes[node_graph[v]], g.first[v]
        lk = ((v - f_i) * n_i + (w - f_i)) * n_i + (u - f_i)
        order = np.lexsort((lk, fam, gr))
        gr, fam, lk, v, w, u = gr[order], fam[order], lk[order], v[order], w[order], u[order]
        new = np.ones(gr.size, dtype=bool)
        new[1:] = (gr[1:] != gr[:-1]) | (fam[1:] != fam[:-1]) | (lk[1:] != lk[:-1])
        gr, lk = gr[new], lk[new]
        by_key = np.lexsort((lk, gr))                                       # per graph ascending keys, and the item behind each
        p._item_key_h, p._item_slot_h = lk[by_key], by_key
        return np.bincount(gr, minlength=B).astype(np.int64), [v[new], w[new], u[new]], False

    @staticmethod
    def graph_class(group, graphs, g):
        """WL / DWL: the fibres of a class of graphs, 3 n^2 each."""
        fib_ptr = np.concatenate([[0], np.cumsum(3 * g.sizes[graphs] * g.sizes[graphs])])
        return group, g.to(graphs, np.int32), g.to(fib_ptr, np.int32), int(fib_ptr[-1])

    @staticmethod
    def launch_arrays(p, g):
        p.node_graph = g.to(g.node_graph, np.int32)
        p.item_key = p.item_slot = None
        if p.connected:                                                      # the lookup of dn_k3wl_local_u64: keys and the item behind each
            p.item_key, p.item_slot = g.to(p._item_key_h, np.int64), g.to(p._item_slot_h, np.int32)
        if p.is_global:                                                      # DWL: a 64-bit adjacency row per node of a fused graph
            bits = np.zeros(g.N, dtype=np.uint64)
            if p.malkin:
                slot_node = np.repeat(np.arange(g.N), g.deg)
                ok = p.fused_graph[g.node_graph[slot_node]]
                np.bitwise_or.at(bits, slot_node[ok], np.uint64(1) << (g.nbr[ok] - g.first[slot_node[ok]]).astype(np.uint64))
            p.adj_bits = g.to(bits.view(np.int64), np.int64)

    @staticmethod
    def init_fused(data, p, nl, el, out):
        ops.k3wl_init(data.num_nodes, p.connected, p.tup_v, p.tup_w, p.tup_u, data.ptr, data.nbr, nl, out)

    @staticmethod
    def init_composed(data, p, nl, el, out):
        s, N = p.device_side(), data.num_nodes
        v, w, u = s["tup"]
        one = torch.ones_like(v)
        ci, cj, ck = one, 2 * one, 3 * one
        if nl is not None:
            ci, cj, ck = ops.wl_pairing(nl[v] + 1, ci), ops.wl_pairing(nl[w] + 1, cj), ops.wl_pairing(nl[u] + 1, ck)

        def code(a, b):
            adj = _member(s["ekey"], a * N + b)[1]
            if p.connected:
                return torch.where(adj, 3 * one, torch.where(a == b, one, 2 * one))
            return torch.where(adj, one, 2 * one)

        pair = ops.wl_pairing
        out.copy_(pair(pair(pair(code(v, w), code(v, u)), code(w, u)), pair(pair(ci, cj), ck)))

    @staticmethod
    def step_fused(data, p, cin, cout):
        if p.is_global:
            for group, graphs, fib_ptr, fibres in p.graph_classes:
                ops.k3wl_global(data.num_graphs, graphs, fib_ptr, fibres, group, p.malkin, data.node_ptr, p.tuple_ptr, p.adj_bits, cin, p.work)
            if p.graph_classes:
                ops.k3wl_close(data.num_nodes, p.malkin, p.tup_v, p.tup_w, p.tup_u, p.node_graph, data.node_ptr, data.ptr, cin, p.work, cout)
        else:
            for group, lds, items in p.tuple_classes:
                ops.k3wl_local(data.num_nodes, items, group, lds, p.connected, p.tup_v, p.tup_w, p.tup_u, p.node_graph, data.node_ptr,
                               p.tuple_ptr, data.ptr, data.nbr, p.item_key, p.item_slot, cin, cout)


def _plan(data, kernel):
    return engine._plan_of(_K3, data, kernel)


def _check(data, num_iterations, kernel, use_node_labels, use_edge_labels):
    return engine._check_of(_K3, data, num_iterations, kernel, use_node_labels, use_edge_labels)


def k3wl_colors(data, num_iterations, kernel, use_node_labels=True, use_edge_labels=True, workspace_keys=K3WL_WORKSPACE_KEYS):
    """([H + 1, T] int64 (unsigned bit patterns): every item's colour after every iteration, tuple_ptr [B + 1] int32: where every
    graph's items start).  Launches only -- nothing is read back (classes and chunks were built with the plan).  use_edge_labels is
    checked like everywhere and then ignored, as the reference ignores it at k = 3."""
    return engine._colors_of(_K3, data, num_iterations, kernel, use_node_labels, use_edge_labels, workspace_keys)


def k3wl_features(data, num_iterations, kernel, use_node_labels=True, use_edge_labels=True, colors=None):
    """The feature CSR of the item colours (graph_kernels.WLFeatures): one map per graph over the colours of all iterations, with
    the position slices of the k = 1 WL kernel."""
    return engine._features_of(_K3, data, num_iterations, kernel, use_node_labels, use_edge_labels, colors)


def k3wl_gram_matrices(data, num_iterations, kernel, use_node_labels=True, use_edge_labels=True, features=None):
    """The H + 1 un-normalised matrices [B, B] (int64), exactly the reference's.  With `features` given: one launch, nothing read back."""
    return engine._gram_matrices_of(_K3, data, num_iterations, kernel, use_node_labels, use_edge_labels, features)


# ------------------------------------------------------------------------------------------------ command line
def gram_file(gram_dir, dataset, kernel, h):
    """gram.cpp:299-304: <gram_dir>/<ds>__<kernel>3_<h>.gram."""
    return os.path.join(gram_dir, "%s__%s3_%d.gram" % (dataset, kernel, h))


def main(argv=None):
    argv = sys.argv[1:] if argv is None else list(argv)
    ap = gk.cli_parser("graph_kernels_k3wl", "3-WL gram matrices (--k 3: WL, DWL, LWL, LWLC) in the reference's libsvm text; --k 1 and "
                                             "--k 2 are handed to graph_kernels_kwl")
    args = ap.parse_args(argv)
    if args.k in (1, 2):
        return engine.main(argv)
    if args.k != 3 or args.kernel not in KERNELS:
        ap.exit(2, "--k %d --kernel %s is not built: --k 3 takes --kernel WL, DWL, LWL or LWLC (as --k 2 does; --k 1 WL, WLOA, SP or GR).  "
                   "LWLP and LWLPC are left out because the reference reads behind the end of its own colour maps there "
                   "(GenerateThree.cpp:641-645, 702-729): there is no defined output to reproduce.\n" % (args.k, args.kernel))
    return gk.cli_run(args, gk.cli_per_iteration(args, gram_file, k3wl_gram_matrices))


if __name__ == "__main__":
    sys.exit(main())
