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

Refused with ValueError: what graph_kernels refuses, a graph whose item count times (H + 1) reaches 1,000,000 (the reference's
MAXNUMCOLOR early stop, `color_nums[h - 1] < MAXNUMCOLOR` here, is not built), and a dataset with 2^31 - 1 items or more.  The kernels
LWLP / LWLPC are not built: the reference dereferences color_map_1 / _2 / _3.find(...) on maps that are empty or keyed by other values
(GenerateThree.cpp:641-645, 702-729), so their output is whatever lies behind end().  GenerateThreeSampling and `simple = false`
cannot be reached from gram.cpp and are not built.
"""
import os
import sys
import time

import numpy as np
import torch

from . import graph_kernels as gk
from . import ops
from .graph_kernels import MAXNUMCOLOR, GraphKernelData, WLFeatures, dataset_flags, write_libsvm  # noqa: F401
from .graph_kernels_kwl import _expand, _member                # (ragged expansion and sorted-key membership, as at k = 2)

KERNELS = ("WL", "DWL", "LWL", "LWLC")
K3WL_WORKSPACE_KEYS = 1 << 24         # multiset entries of one composed chunk (a handful of int64 arrays of that length live at once)
_I64_MAX = (1 << 63) - 1
_KEY_NODES = 1 << 21                  # (a N + b) N + c stays below 2^63 for N below this


def _ragged(count):
    """(owner of every item, its position within its owner) for count.sum() items (numpy)."""
    owner = np.repeat(np.arange(count.size), count)
    start = np.cumsum(count) - count
    return owner, np.arange(int(count.sum())) - start[owner]


class _Plan:
    """The items of a dataset under one kernel and everything the launches need, built once on the host."""

    def __init__(self, data, kernel):
        dev = data.device
        to = lambda a, dt: torch.from_numpy(np.ascontiguousarray(np.asarray(a).astype(dt))).to(dev)  # noqa: E731
        node_ptr = data.node_ptr.cpu().numpy().astype(np.int64)
        ptr, N, B = data._ptr_h, data.num_nodes, data.num_graphs
        sizes, deg = np.diff(node_ptr), np.diff(ptr)
        node_graph = np.repeat(np.arange(B), sizes)
        first = node_ptr[:-1][node_graph]
        self.kernel, self.connected, self.malkin, self.is_global = kernel, kernel == "LWLC", kernel == "DWL", kernel in ("WL", "DWL")
        self.lower_bound = False
        if self.connected:
            nbr = data.nbr.cpu().numpy().astype(np.int64)
            edges_of = ptr[node_ptr[1:]] - ptr[node_ptr[:-1]]
            wedges = np.zeros(B, dtype=np.int64)
            np.add.at(wedges, node_graph, deg * (deg - 1))                  # (centre, ordered pair of its neighbours)
            lower = sizes + edges_of + (wedges + 2) // 3                    # an item of the third family has at most three centres
            if int(lower.max()) >= MAXNUMCOLOR or int(lower.sum()) >= (1 << 31) - 1:
                self.count, self.largest, self.num_tuples, self.lower_bound = lower, int(lower.argmax()), int(lower.sum()), True
                return                                                      # (refused by _check before anything is built)
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
            g, n_i, f_i = node_graph[v], sizes[node_graph[v]], first[v]
            lk = ((v - f_i) * n_i + (w - f_i)) * n_i + (u - f_i)
            order = np.lexsort((lk, fam, g))
            g, fam, lk, v, w, u = g[order], fam[order], lk[order], v[order], w[order], u[order]
            new = np.ones(g.size, dtype=bool)
            new[1:] = (g[1:] != g[:-1]) | (fam[1:] != fam[:-1]) | (lk[1:] != lk[:-1])
            g, lk, tup_v, tup_w, tup_u = g[new], lk[new], v[new], w[new], u[new]
            count = np.bincount(g, minlength=B).astype(np.int64)
            by_key = np.lexsort((lk, g))                                    # per graph ascending keys, and the item behind each
            self._item_key_h, self._item_slot_h = lk[by_key], by_key
        else:
            count = sizes * sizes * sizes
        tuple_ptr = np.concatenate([[0], np.cumsum(count)])
        T = int(tuple_ptr[-1])
        self.count, self.tuple_ptr_h, self.num_tuples = count, tuple_ptr, T
        self.largest = int(count.argmax())
        if T >= (1 << 31) - 1:
            return                                                          # (refused by _check before anything is used)
        if not self.connected:
            local = np.arange(T) - np.repeat(tuple_ptr[:-1], count)
            n_t, base_t = np.repeat(sizes, count), np.repeat(node_ptr[:-1], count)
            tup_v, tup_w, tup_u = base_t + local // (n_t * n_t), base_t + (local // n_t) % n_t, base_t + local % n_t
            self.item_key = self.item_slot = None
        else:
            self.item_key, self.item_slot = to(self._item_key_h, np.int64), to(self._item_slot_h, np.int32)
        self.tup_v, self.tup_w, self.tup_u = to(tup_v, np.int32), to(tup_w, np.int32), to(tup_u, np.int32)
        self.tuple_ptr = to(tuple_ptr, np.int32)
        self.node_graph = to(node_graph, np.int32)
        self.tuple_graph = to(np.repeat(np.arange(B), count), np.int64)
        self._tup_graph_h = node_graph[tup_v]
        dv, dw, du = deg[tup_v], deg[tup_w], deg[tup_u]
        # the fused launches: graph classes by the power of two above the size (WL / DWL), item classes by the longest list (LWL / LWLC)
        if self.is_global:
            fused_graph = sizes <= ops.k3wl_max_nodes()
            n2 = np.maximum(8, 1 << np.ceil(np.log2(np.maximum(sizes, 1))).astype(np.int64))
            self.graph_classes = []
            for c in np.unique(n2[fused_graph]):
                graphs = np.nonzero(fused_graph & (n2 == c))[0]
                fib_ptr = np.concatenate([[0], np.cumsum(3 * sizes[graphs] * sizes[graphs])])
                self.graph_classes.append((int(c), to(graphs, np.int32), to(fib_ptr, np.int32), int(fib_ptr[-1])))
            bits = np.zeros(N, dtype=np.uint64)
            if self.malkin:
                slot_node = np.repeat(np.arange(N), deg)
                nbr = data.nbr.cpu().numpy().astype(np.int64)
                ok = fused_graph[node_graph[slot_node]]
                np.bitwise_or.at(bits, slot_node[ok], np.uint64(1) << (nbr[ok] - first[slot_node[ok]]).astype(np.uint64))
            self.adj_bits = to(bits.view(np.int64), np.int64)
            self.work = torch.empty((6 if self.malkin else 3) * T, dtype=torch.int64, device=dev)
            n_t = sizes[self._tup_graph_h]
            self._cand = [n_t, n_t, n_t]
            self._phys = 6 * n_t + 4
        else:
            cap = ops.k3wl_max_entries()
            gmax = np.zeros(B, dtype=np.int64)
            np.maximum.at(gmax, node_graph, deg)
            fused_graph = gmax <= cap
            longest = np.maximum(dv + dw, du) if self.connected else np.maximum(np.maximum(dv, dw), du)
            ok = fused_graph[self._tup_graph_h]
            pick = lambda m: to(np.nonzero(m & ok)[0], np.int32)  # noqa: E731
            block = (longest > 64) & ok
            lds = 1 << int(longest[block].max() - 1).bit_length() if block.any() else 0
            self.tuple_classes = [(grp, l, t) for grp, l, t in ((8, 0, pick(longest <= 8)), (64, 0, pick((longest > 8) & (longest <= 64))),
                                                                (0, lds, pick(longest > 64))) if t.numel()]
            self._cand = [dv, dw, du]
            self._phys = 2 * (dv + dw + du)
        self.fused_graph = fused_graph
        self._chunks = {}
        self._dev = None
        self._data = data

    def device_side(self):
        """Arrays only the composed path needs (built on its first use)."""
        if self._dev is None:
            d, N = self._data, self._data.num_nodes
            dev = d.device
            if N >= _KEY_NODES:
                raise ValueError("%s: %d nodes: the composed path keys a triple as (a N + b) N + c and takes fewer than %d"
                                 % (d.source, N, _KEY_NODES))
            sizes = (d.node_ptr[1:] - d.node_ptr[:-1]).long()
            big = torch.full((1,), _I64_MAX, dtype=torch.int64, device=dev)
            v, w, u = self.tup_v.long(), self.tup_w.long(), self.tup_u.long()
            s = dict(ekey=torch.cat([d.slot_node * N + d.nbr_long, big]), gsize=sizes[d.node_graph], first=d.node_ptr.long()[d.node_graph],
                     t0=self.tuple_ptr.long()[d.node_graph], ptr=d.ptr.long(), deg=(d.ptr[1:] - d.ptr[:-1]).long(), tup=(v, w, u))
            if self.connected:
                slot = self.item_slot.long()
                s["slot"] = slot
                s["tkey"] = torch.cat([((v * N + w) * N + u)[slot], big])   # ascending: graphs are runs of nodes, keys ascend within one
            self._dev = s
        return self._dev

    def chunks(self, everything, workspace_keys):
        """Runs of items of at most workspace_keys entries each (a single item with more is a run of its own): of every graph, or of
        the graphs the fused kernels leave out.  [(item ids int64, candidates of exchanges 1, 2, 3, entries)]."""
        key = (bool(everything), int(workspace_keys))
        if key not in self._chunks:
            ids = np.arange(self.num_tuples) if everything else np.nonzero(~self.fused_graph[self._tup_graph_h])[0]
            out, a = [], 0
            if ids.size:
                run = np.cumsum(self._phys[ids])
                while a < ids.size:
                    b = int(np.searchsorted(run, (run[a - 1] if a else 0) + workspace_keys, side="right"))
                    b = min(max(b, a + 1), a + workspace_keys)               # (items without entries: bounded by their number)
                    t = ids[a:b]
                    out.append((torch.from_numpy(t.astype(np.int64)).to(self._data.device), [int(c[t].sum()) for c in self._cand],
                                int(self._phys[t].sum())))
                    a = b
            self._chunks[key] = out
        return self._chunks[key]


def _plan(data, kernel):
    plans = data.__dict__.setdefault("_k3wl_plans", {})
    if kernel not in plans:
        plans[kernel] = _Plan(data, kernel)
    return plans[kernel]


def _check(data, num_iterations, kernel, use_node_labels, use_edge_labels):
    if kernel not in KERNELS:
        raise ValueError("kernel %r is not built at k = 3: WL, DWL, LWL and LWLC are (LWLP / LWLPC read behind the end of the reference's "
                         "own colour maps, so there is nothing to reproduce)" % (kernel,))
    H = int(num_iterations)
    if H < 0:
        raise ValueError("num_iterations must be >= 0 (got %d)" % H)
    if use_node_labels and data.node_label is None:
        raise ValueError("%s: use_node_labels without node labels (no node-label file)"
                         % data.missing.get("node_labels", data.source + "[node_labels]"))
    if use_edge_labels and data.edge_label is None:
        raise ValueError("%s: use_edge_labels without edge labels (no edge-label file; the reference dereferences end() here)"
                         % data.missing.get("edge_labels", data.source + "[edge_labels]"))
    p = _plan(data, kernel)
    if int(p.count.max()) * (H + 1) >= MAXNUMCOLOR:
        raise ValueError("%s: graph %d has %s%d items, times (H + 1) = %d that reaches %d: the reference's MAXNUMCOLOR early stop is not built"
                         % (data.source, p.largest + 1, "at least " if p.lower_bound else "", int(p.count.max()), H + 1, MAXNUMCOLOR))
    if p.num_tuples >= (1 << 31) - 1:
        raise ValueError("%s: %d items, more than 2^31 - 2" % (data.source, p.num_tuples))
    return H, p


# ------------------------------------------------------------------------------------------------ composed path
def _init_composed(data, p, nl, out):
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


def _sort3(f, h):
    """Three folds per item [t, 3] with presence flags: present before absent, ascending (unsigned) among the present."""
    f, h = list(f.unbind(1)), list(h.unbind(1))
    for a, b in ((0, 1), (1, 2), (0, 1)):
        swap = (~h[a] & h[b]) | (h[a] & h[b] & ((f[a] ^ ops._WL_SIGN) > (f[b] ^ ops._WL_SIGN)))
        f[a], f[b] = torch.where(swap, f[b], f[a]), torch.where(swap, f[a], f[b])
        h[a], h[b] = torch.where(swap, h[b], h[a]), torch.where(swap, h[a], h[b])
    return f, h


def _combine(own, fold, has):
    """own [t], fold / has [t, 6] in the order (local 1, 2, 3, global 1, 2, 3)."""
    acc = own
    for lo in (0, 3):
        for f, ok in zip(*_sort3(fold[:, lo:lo + 3], has[:, lo:lo + 3])):
            acc = torch.where(ok, ops.wl_pairing(acc, f), acc)
    return acc


def _step_composed(data, p, chunks, cin, cout):
    s, N = p.device_side(), data.num_nodes
    for tids, cand, phys in chunks:
        tri = [c[tids] for c in s["tup"]]
        Tc = int(tids.numel())
        trash = 6 * Tc
        segs, idxs, mults = [], [], []
        for ex, total in enumerate(cand):
            if total == 0:
                continue
            moved = tri[ex]                                                  # the component that is exchanged
            if p.is_global:
                ti, j = _expand(s["gsize"][moved], total)
                x = s["first"][moved][ti] + j
            else:
                ti, j = _expand(s["deg"][moved], total)
                x = data.nbr_long[s["ptr"][moved][ti] + j]
            a, b, c = [x if e == ex else tri[e][ti] for e in range(3)]       # the triple whose colour is gathered
            drop = torch.zeros_like(x, dtype=torch.bool)
            if p.connected:
                pos, hit = _member(s["tkey"], (a * N + b) * N + c)
                drop = ~hit
                idx = s["slot"][pos.clamp(max=p.num_tuples - 1)]
            else:
                f, n = s["first"][a], s["gsize"][a]
                idx = s["t0"][a] + ((a - f) * n + (b - f)) * n + (c - f)
            mult = torch.full_like(x, 2)
            glob = torch.zeros_like(x)
            if p.is_global:
                own = x == moved[ti]
                if ex:
                    drop = own                                               # exchanges 2 and 3 leave the triple itself out
                else:
                    mult = torch.where(own, 3 * mult, mult)                  # exchange 1 holds it six times
                if p.malkin:
                    adj = _member(s["ekey"], moved[ti] * N + x)[1]
                    glob = (own | ~adj).long()
            mset = (0, 0, 1)[ex] if p.connected else ex                      # LWLC: exchanges 1 and 2 share a multiset
            segs.append(torch.where(drop, torch.full_like(x, trash), ti * 6 + mset + 3 * glob))
            idxs.append(idx)
            mults.append(mult)
        if not segs:
            cout[tids] = cin[tids]
            continue
        mult = torch.cat(mults)
        rep = torch.repeat_interleave(torch.arange(mult.numel(), device=mult.device), mult, output_size=phys)
        fold, size = ops.kwl_fold_from_max(torch.cat(segs)[rep], cin[torch.cat(idxs)][rep], trash)
        cout[tids] = _combine(cin[tids], fold.view(Tc, 6), size.view(Tc, 6) > 0)


# ------------------------------------------------------------------------------------------------ colours
def _step(data, p, cin, cout, workspace_keys):
    if not ops.k3wl_fused_enabled(p.kernel):
        _step_composed(data, p, p.chunks(True, workspace_keys), cin, cout)
        return
    if p.is_global:
        for group, graphs, fib_ptr, fibres in p.graph_classes:
            ops.k3wl_global(data.num_graphs, graphs, fib_ptr, fibres, group, p.malkin, data.node_ptr, p.tuple_ptr, p.adj_bits, cin, p.work)
        if p.graph_classes:
            ops.k3wl_close(data.num_nodes, p.malkin, p.tup_v, p.tup_w, p.tup_u, p.node_graph, data.node_ptr, data.ptr, cin, p.work, cout)
    else:
        for group, lds, items in p.tuple_classes:
            ops.k3wl_local(data.num_nodes, items, group, lds, p.connected, p.tup_v, p.tup_w, p.tup_u, p.node_graph, data.node_ptr,
                           p.tuple_ptr, data.ptr, data.nbr, p.item_key, p.item_slot, cin, cout)
    if not p.fused_graph.all():
        _step_composed(data, p, p.chunks(False, workspace_keys), cin, cout)


def k3wl_colors(data, num_iterations, kernel, use_node_labels=True, use_edge_labels=True, workspace_keys=K3WL_WORKSPACE_KEYS):
    """([H + 1, T] int64 (unsigned bit patterns): every item's colour after every iteration, tuple_ptr [B + 1] int32: where every
    graph's items start).  Launches only -- nothing is read back (classes and chunks were built with the plan).  use_edge_labels is
    checked like everywhere and then ignored, as the reference ignores it at k = 3."""
    H, p = _check(data, num_iterations, kernel, use_node_labels, use_edge_labels)
    workspace_keys = int(workspace_keys)
    if workspace_keys < 1:
        raise ValueError("workspace_keys must be positive (got %d)" % workspace_keys)
    nl = data.node_label if use_node_labels else None
    c = torch.empty((H + 1, p.num_tuples), dtype=torch.int64, device=data.device)
    if ops.k3wl_fused_enabled(kernel):
        ops.k3wl_init(data.num_nodes, p.connected, p.tup_v, p.tup_w, p.tup_u, data.ptr, data.nbr, nl, c[0])
    else:
        _init_composed(data, p, nl, c[0])
    for h in range(1, H + 1):
        _step(data, p, c[h - 1], c[h], workspace_keys)
    return c, p.tuple_ptr


# ------------------------------------------------------------------------------------------------ features and matrices
def k3wl_features(data, num_iterations, kernel, use_node_labels=True, use_edge_labels=True, colors=None):
    """The feature CSR of the item colours (graph_kernels.WLFeatures): one map per graph over the colours of all iterations, with
    the position slices of the k = 1 WL kernel."""
    H, p = _check(data, num_iterations, kernel, use_node_labels, use_edge_labels)
    c = k3wl_colors(data, H, kernel, use_node_labels, use_edge_labels)[0] if colors is None else colors
    return gk.features_of_colors(p.tuple_graph, c, data.num_graphs)


def k3wl_gram_matrices(data, num_iterations, kernel, use_node_labels=True, use_edge_labels=True, features=None):
    """The H + 1 un-normalised matrices [B, B] (int64), exactly the reference's.  With `features` given: one launch, nothing read back."""
    H, _ = _check(data, num_iterations, kernel, use_node_labels, use_edge_labels)
    if H + 1 > ops.wl_max_steps():
        raise ValueError("num_iterations + 1 = %d exceeds the gram kernel's %d steps" % (H + 1, ops.wl_max_steps()))
    f = k3wl_features(data, H, kernel, use_node_labels, use_edge_labels) if features is None else features
    if f.num_steps != H + 1:
        raise ValueError("features were built for %d iterations, not %d" % (f.num_steps - 1, H))
    return list(ops.wl_gram(f.ptr, f.color, f.count, f.step, f.num_graphs, f.num_steps, False).unbind(0))


# ------------------------------------------------------------------------------------------------ command line
def gram_file(gram_dir, dataset, kernel, h):
    """gram.cpp:299-304: <gram_dir>/<ds>__<kernel>3_<h>.gram."""
    return os.path.join(gram_dir, "%s__%s3_%d.gram" % (dataset, kernel, h))


def main(argv=None):
    import argparse
    argv = sys.argv[1:] if argv is None else list(argv)
    ap = argparse.ArgumentParser(prog="python -m dummynode4graphlearning_amd.graph_kernels_k3wl",
                                 description="3-WL gram matrices (--k 3: WL, DWL, LWL, LWLC) in the reference's libsvm text; --k 1 and "
                                             "--k 2 are handed to graph_kernels_kwl")
    ap.add_argument("--dataset_dir", default="./datasets")
    ap.add_argument("--gram_dir", default="./svm/GM/EXP")
    ap.add_argument("--k", type=int, default=1)
    ap.add_argument("--kernel", default="WL")
    ap.add_argument("--n_iters", type=int, default=1)
    ap.add_argument("--datasets", nargs="*", default=[])
    ap.add_argument("--device", default="cuda")
    args = ap.parse_args(argv)
    if args.k in (1, 2):
        from . import graph_kernels_kwl
        return graph_kernels_kwl.main(argv)
    if args.k != 3 or args.kernel not in KERNELS:
        ap.exit(2, "--k %d --kernel %s is not built: --k 3 takes --kernel WL, DWL, LWL or LWLC (as --k 2 does; --k 1 WL, WLOA, SP or GR).  "
                   "LWLP and LWLPC are left out because the reference reads behind the end of its own colour maps there "
                   "(GenerateThree.cpp:641-645, 702-729): there is no defined output to reproduce.\n" % (args.k, args.kernel))
    jobs = []
    for name in args.datasets:
        if name not in gk.DATASET_FLAGS:
            print("Warning: %s is not a valid dataset." % name)
        jobs.append((name, GraphKernelData.from_dir(args.dataset_dir, name, device=args.device)) + dataset_flags(name))
    for name, data, use_nl, use_el in jobs:
        t0 = time.time()
        for h, G in enumerate(k3wl_gram_matrices(data, args.n_iters, args.kernel, use_nl, use_el)):
            write_libsvm(G, data.classes, gram_file(args.gram_dir, name, args.kernel, h))
        print("%s-%d\t%s\t%d seconds" % (args.kernel, args.n_iters, name, int(time.time() - t0)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
