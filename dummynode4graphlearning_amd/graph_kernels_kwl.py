"""The 2-WL graph kernels, computed on the device: the counterpart of the reference's graph-kernel tool at `gram --k 2 --kernel WL |
DWL | LWL | LWLC` (graph_classification/graph_kernels), for the datasets graph_kernels.GraphKernelData reads -- and the host engine of
the k-WL kernels at every k that is built (graph_kernels_k3wl binds it at k = 3).

  tuple graphs           src/GenerateTwo.cpp:752 on (generate_global_graph, _malkin,   never built: gathers from a graph's own colour
                         generate_local_graph, _connected)                             matrix, selected by the dataset CSR
  initial colours        the same (the tuple graph's node labels)                      dn_kwl.hip: dn_kwl_init_u64
  refinement             GenerateTwo::compute_colors_simple, :450-750                  kwl_colors (dn_kwl_local_u64 / dn_kwl_global_u64)
  colour maps, matrices  :583-594, :722-736, gram.cpp:195-250                          kwl_features / kwl_gram_matrices (the k = 1 WL
                                                                                       feature build and dn_wl_gram_i64)
  command line           gram.cpp:38-104                                               python -m dummynode4graphlearning_amd.graph_kernels_kwl

The items are node pairs ("tuples") (i, j) of one graph: all n^2 of them, row-major (WL, DWL, LWL), or only i == j and adjacent pairs
(LWLC).  A tuple (v, w) has up to four neighbour multisets of the previous colours C: type 1 exchanges the first component (C[x, w]),
type 2 the second (C[v, x]); LWL / LWLC let x run over the neighbours of the exchanged node (local), WL over all nodes (local), DWL
over all nodes with the neighbours local and the rest global.  The reference's tuple graph is undirected and its add_edge pushes both
ends, so every neighbour colour enters its multiset TWICE; in WL / DWL both exchange loops reach the tuple itself, the edge-type map
keeps the first insertion (type 1) and each of the two self add_edge calls pushes twice: the tuple's own colour enters type 1 FOUR
times (DWL: global 1, has_edge(v, v) being false).  A multiset is sorted ascending (unsigned) and folded with the pairing function
starting from its maximum; the new colour is the old one folded over the sorted local folds, then the sorted global folds.  Edge
labels enter the initial colours only.  tests/kwl_ref.py restates all of this in plain Python and tests/golden/graph_kernels_kwl.json
holds the text the reference's own binary wrote.

Paths.  The fused kernels (ops.kwl_fused(True)) take every graph within their limits: ops.kwl_max_nodes() nodes for WL / DWL (a
workgroup per graph, colour matrix in LDS), ops.kwl_max_entries() for the largest degree of a graph for LWL / LWLC.  Larger graphs,
and every graph under ops.kwl_fused(False), take the composed path: the multiset entries of a run of tuples are built with torch
device ops, sorted device-wide by (multiset, colour) and folded by dn_wl_fold_u64, at most `workspace_keys` entries at a time.  Tuple
classes, graph classes and chunks are built once per dataset on the host; a refinement reads nothing back.

The engine.  What is the same at every k -- the plan (all-tuples enumeration, graph and item classes, chunks), the checks, the
composed step, the colour / feature / matrix drivers -- is written once below and takes k from a description (_K2 here, _K3 in
graph_kernels_k3wl): k enters through arithmetic and loop bounds (a k-digit key to base n, 2 k multisets per item, k copies of the own
colour's pair), and the description holds what is genuinely one k's: the noun, the MAXNUMCOLOR predicate and its message, the LWLC
item enumeration, the arrays and launches of its fused kernels, its initial colours, its switch and its limits.

Refused with ValueError: what graph_kernels refuses, a graph with more than 1,000,000 / (H + 1) tuples (the reference's MAXNUMCOLOR
early stop is not built), and a dataset with 2^31 - 1 tuples or more.  `--k 3` is graph_kernels_k3wl's.  The kernels LWLP / LWLPC are
not built: the reference's LWLP / LWLPC dereference color_map_1.find(...) / color_map_2.find(...) on maps that are empty or keyed by
other values (GenerateTwo.cpp:579-580, 638, 650), so their output is whatever lies behind end().
"""
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

from . import graph_kernels as gk
from . import ops
from .graph_kernels import MAXNUMCOLOR, GraphKernelData, WLFeatures, dataset_flags, write_libsvm  # noqa: F401

KERNELS = ("WL", "DWL", "LWL", "LWLC")
KWL_WORKSPACE_KEYS = 1 << 24          # multiset entries of one composed chunk (a handful of int64 arrays of that length live at once)
_I64_MAX = (1 << 63) - 1


# ------------------------------------------------------------------------------------------------ the engine: plan and checks
class _Plan:
    """The items (k-tuples of nodes) of a dataset under one kernel and everything the launches need, built once on the host."""

    def __init__(self, K, data, kernel):
        k, dev = K.k, data.device
        to = lambda a, dt: torch.from_numpy(np.ascontiguousarray(np.asarray(a).astype(dt))).to(dev)  # noqa: E731
        node_ptr = data.node_ptr.cpu().numpy().astype(np.int64)
        ptr, N, B = data._ptr_h, data.num_nodes, data.num_graphs
        sizes, deg = np.diff(node_ptr), np.diff(ptr)
        node_graph = np.repeat(np.arange(B), sizes)
        g = SimpleNamespace(to=to, node_ptr=node_ptr, ptr=ptr, N=N, B=B, sizes=sizes, deg=deg, node_graph=node_graph,
                            first=node_ptr[:-1][node_graph], nbr=data.nbr.cpu().numpy().astype(np.int64))
        self.K, self.kernel, self.connected, self.malkin, self.is_global = K, kernel, kernel == "LWLC", kernel == "DWL", kernel in ("WL", "DWL")
        count, tup, self.lower_bound = K.connected_items(self, g) if self.connected else (sizes ** k, None, False)
        tuple_ptr = np.concatenate([[0], np.cumsum(count)])
        T = int(tuple_ptr[-1])
        self.count, self.tuple_ptr_h, self.num_tuples = count, tuple_ptr, T
        self.largest = int(count.argmax())
        if self.lower_bound or T >= (1 << 31) - 1:
            return                                                          # (refused by _check before anything is used)
        if not self.connected:                                              # all of them, row-major: the k base-n digits of the position
            local = np.arange(T) - np.repeat(tuple_ptr[:-1], count)
            n_t, base_t = np.repeat(sizes, count), np.repeat(node_ptr[:-1], count)
            tup = [base_t + (local // n_t ** (k - 1 - e)) % n_t for e in range(k)]
        self.tup = [to(t, np.int32) for t in tup]
        for name, t in zip(("tup_v", "tup_w", "tup_u"), self.tup):
            setattr(self, name, t)
        self.tuple_ptr = to(tuple_ptr, np.int32)
        self.tuple_graph = to(np.repeat(np.arange(B), count), np.int64)
        self._tup_graph_h = node_graph[tup[0]]
        # the fused launches: graph classes by the power of two above the size (WL / DWL), item classes by the longest list (LWL / LWLC)
        if self.is_global:
            fused_graph = sizes <= K.max_nodes()
            n2 = np.maximum(8, 1 << np.ceil(np.log2(np.maximum(sizes, 1))).astype(np.int64))
            self.graph_classes = [K.graph_class(int(c), np.nonzero(fused_graph & (n2 == c))[0], g) for c in np.unique(n2[fused_graph])]
            self.work = torch.empty((2 * k if self.malkin else k) * T, dtype=torch.int64, device=dev)
            n_t = sizes[self._tup_graph_h]
            # the composed path's per-item costs: candidates per exchange (before the copies) and entries (with them)
            self._cand = [n_t] * k
            self._phys = 2 * k * n_t + 2 * k - 2                            # every candidate twice, the own colour 2 k times in all
        else:
            gmax = np.zeros(B, dtype=np.int64)
            np.maximum.at(gmax, node_graph, deg)
            fused_graph = gmax <= K.max_entries()
            self._cand = [deg[t] for t in tup]
            mset = K.multisets[self.connected]
            longest = np.maximum.reduce([sum(c for c, m in zip(self._cand, mset) if m == i) for i in sorted(set(mset))])
            ok = fused_graph[self._tup_graph_h]
            pick = lambda m: to(np.nonzero(m & ok)[0], np.int32)  # noqa: E731
            block = (longest > 64) & ok
            lds = 1 << int(longest[block].max() - 1).bit_length() if block.any() else 0
            self.tuple_classes = [(grp, l, t) for grp, l, t in ((8, 0, pick(longest <= 8)), (64, 0, pick((longest > 8) & (longest <= 64))),
                                                                (0, lds, pick(longest > 64))) if t.numel()]
            self._phys = 2 * sum(self._cand)
        self.fused_graph = fused_graph
        K.launch_arrays(self, g)
        self._chunks = {}
        self._dev = None
        self._data = data

    def device_side(self):
        """Arrays only the composed path needs (built on its first use)."""
        if self._dev is None:
            d, N, K = self._data, self._data.num_nodes, self.K
            if N ** K.k > _I64_MAX:
                raise ValueError("%s: %d nodes: the composed path keys a %s as %s and takes fewer than %d"
                                 % ((d.source, N) + K.keyed + (1 << -(-63 // K.k),)))
            n = (d.node_ptr[1:] - d.node_ptr[:-1]).long()[d.node_graph]
            first = d.node_ptr.long()[d.node_graph]
            tup = [t.long() for t in self.tup]
            # item (a, b, ..) of an all-tuples kernel sits at off[a] + its digits to base gsize[a]
            s = dict(ekey=torch.cat([d.slot_node * N + d.nbr_long, d.nbr_long.new_full((1,), _I64_MAX)]), gsize=n, first=first,
                     off=self.tuple_ptr.long()[d.node_graph] - first * sum(n ** e for e in range(K.k)), ptr=d.ptr.long(),
                     deg=(d.ptr[1:] - d.ptr[:-1]).long(), tup=tup)
            if self.connected:             # the items by ascending key, then a sentinel above every query (its slot: any item, dropped)
                tkey, slot = torch.sort(_key(tup, N))
                s["tkey"] = torch.cat([tkey, tkey.new_full((1,), _I64_MAX)])
                s["slot"] = torch.cat([slot, slot.new_full((1,), self.num_tuples - 1)])
            self._dev = s
        return self._dev

    def chunks(self, everything, workspace_keys):
        """Runs of items of at most workspace_keys entries each (a single item with more is a run of its own): of every graph, or of
        the graphs the fused kernels leave out.  [(item ids int64, candidates of exchanges 1 .. k, entries)]."""
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


def _plan_of(K, data, kernel):
    plans = data.__dict__.setdefault(K.cache, {})
    if kernel not in plans:
        plans[kernel] = _Plan(K, data, kernel)
    return plans[kernel]


def _check_of(K, data, num_iterations, kernel, use_node_labels, use_edge_labels):
    if kernel not in KERNELS:
        raise ValueError("kernel %r is not built at k = %d: WL, DWL, LWL and LWLC are (LWLP / LWLPC read behind the end of the reference's "
                         "own colour maps, so there is nothing to reproduce)" % (kernel, K.k))
    H = int(num_iterations)
    if H < 0:
        raise ValueError("num_iterations must be >= 0 (got %d)" % H)
    if use_node_labels and data.node_label is None:
        raise ValueError("%s: use_node_labels without node labels (no node-label file)"
                         % data.missing.get("node_labels", data.source + "[node_labels]"))
    if use_edge_labels and data.edge_label is None:
        raise ValueError("%s: use_edge_labels without edge labels (no edge-label file; the reference dereferences end() here)"
                         % data.missing.get("edge_labels", data.source + "[edge_labels]"))
    p = _plan_of(K, data, kernel)
    too_many = K.too_many(p, int(p.count.max()), H)
    if too_many:
        raise ValueError("%s: graph %d has %s: the reference's MAXNUMCOLOR early stop is not built" % (data.source, p.largest + 1, too_many))
    if p.num_tuples >= (1 << 31) - 1:
        raise ValueError("%s: %d %s, more than 2^31 - 2" % (data.source, p.num_tuples, K.noun))
    return H, p


# ------------------------------------------------------------------------------------------------ the engine: composed path
def _member(sorted_keys, q):
    """(position, is q in the ascending keys?); sorted_keys ends with a sentinel above every query."""
    pos = torch.searchsorted(sorted_keys, q)
    return pos, sorted_keys[pos] == q


def _expand(count, total):
    """Ragged expansion: (owner of every item, its position within its owner) for `total` = count.sum() items (known on the host)."""
    owner = torch.repeat_interleave(torch.arange(count.numel(), device=count.device), count, output_size=total)
    start = torch.cumsum(count, 0) - count
    return owner, torch.arange(total, device=count.device) - start[owner]


def _key(digits, base):
    """(d0 base + d1) base + d2 ..: the digits of an item to one number."""
    acc = digits[0]
    for d in digits[1:]:
        acc = acc * base + d
    return acc


def _combine(k, malkin, own, fold, has):
    """own [t], fold / has [t, 2 k] in the order (local 1 .. k, global 1 .. k): own folded over the local folds that are present, in
    ascending (unsigned) order, then over the global ones (DWL only has any).  The compare-exchanges bring the present folds before
    the absent ones, ascending among themselves."""
    acc = own
    for lo in (0, k) if malkin else (0,):
        f, h = list(fold[:, lo:lo + k].unbind(1)), list(has[:, lo:lo + k].unbind(1))
        for a, b in ((a, a + 1) for last in range(k - 1, 0, -1) for a in range(last)):
            swap = h[b] & (~h[a] | ((f[a] ^ ops._WL_SIGN) > (f[b] ^ ops._WL_SIGN)))
            f[a], f[b] = torch.where(swap, f[b], f[a]), torch.where(swap, f[a], f[b])
            h[a], h[b] = h[a] | h[b], h[a] & h[b]
        for fi, ok in zip(f, h):
            acc = torch.where(ok, ops.wl_pairing(acc, fi), acc)
    return acc


def _step_composed(K, data, p, chunks, cin, cout):
    s, N, k = p.device_side(), data.num_nodes, K.k
    mset = K.multisets[p.connected]
    for tids, cand, phys in chunks:
        tup = [c[tids] for c in s["tup"]]
        Tc = int(tids.numel())
        trash = 2 * k * Tc                                                   # the segment of what is dropped
        segs, idxs, mults = [], [], []
        for ex, total in enumerate(cand):
            if total == 0:
                continue
            moved = tup[ex]                                                  # the component that is exchanged
            if p.is_global:
                ti, j = _expand(s["gsize"][moved], total)
                x = s["first"][moved][ti] + j
            else:
                ti, j = _expand(s["deg"][moved], total)
                x = data.nbr_long[s["ptr"][moved][ti] + j]
            item = [x if e == ex else tup[e][ti] for e in range(k)]          # the item whose colour is gathered
            seg = ti * (2 * k) + mset[ex]
            mult = torch.full_like(x, 2)
            drop = None
            if p.connected:
                pos, hit = _member(s["tkey"], _key(item, N))
                drop = ~hit
                idx = s["slot"][pos]
            else:
                idx = s["off"][item[0]] + _key(item, s["gsize"][item[0]])
            if p.is_global:
                own = x == moved[ti]
                if ex:
                    drop = own                                               # the later exchanges leave the item itself out
                else:
                    mult = torch.where(own, k * mult, mult)                  # exchange 1 holds it 2 k times
                if p.malkin:
                    adj = _member(s["ekey"], moved[ti] * N + x)[1]
                    seg = seg + k * (own | ~adj)
            segs.append(seg if drop is None else torch.where(drop, torch.full_like(x, trash), seg))
            idxs.append(idx)
            mults.append(mult)
        if not segs:
            cout[tids] = cin[tids]
            continue
        mult = torch.cat(mults)
        rep = torch.repeat_interleave(torch.arange(mult.numel(), device=mult.device), mult, output_size=phys)
        fold, size = ops.kwl_fold_from_max(torch.cat(segs)[rep], cin[torch.cat(idxs)][rep], trash)
        cout[tids] = _combine(k, p.malkin, cin[tids], fold.view(Tc, 2 * k), size.view(Tc, 2 * k) > 0)


# ------------------------------------------------------------------------------------------------ the engine: colours, features, matrices
def _colors_of(K, data, num_iterations, kernel, use_node_labels, use_edge_labels, workspace_keys):
    H, p = _check_of(K, data, num_iterations, kernel, use_node_labels, use_edge_labels)
    workspace_keys = int(workspace_keys)
    if workspace_keys < 1:
        raise ValueError("workspace_keys must be positive (got %d)" % workspace_keys)
    nl = data.node_label if use_node_labels else None
    el = data.edge_label if use_edge_labels else None
    c = torch.empty((H + 1, p.num_tuples), dtype=torch.int64, device=data.device)
    (K.init_fused if K.fused_enabled(kernel) else K.init_composed)(data, p, nl, el, c[0])
    for h in range(1, H + 1):
        if not K.fused_enabled(kernel):
            _step_composed(K, data, p, p.chunks(True, workspace_keys), c[h - 1], c[h])
            continue
        K.step_fused(data, p, c[h - 1], c[h])
        if not p.fused_graph.all():
            _step_composed(K, data, p, p.chunks(False, workspace_keys), c[h - 1], c[h])
    return c, p.tuple_ptr


def _features_of(K, data, num_iterations, kernel, use_node_labels, use_edge_labels, colors):
    H, p = _check_of(K, data, num_iterations, kernel, use_node_labels, use_edge_labels)
    c = _colors_of(K, data, H, kernel, use_node_labels, use_edge_labels, KWL_WORKSPACE_KEYS)[0] if colors is None else colors
    return gk.features_of_colors(p.tuple_graph, c, data.num_graphs)


def _gram_matrices_of(K, data, num_iterations, kernel, use_node_labels, use_edge_labels, features):
    H, _ = _check_of(K, data, num_iterations, kernel, use_node_labels, use_edge_labels)
    if H + 1 > ops.wl_max_steps():
        raise ValueError("num_iterations + 1 = %d exceeds the gram kernel's %d steps" % (H + 1, ops.wl_max_steps()))
    f = _features_of(K, data, H, kernel, use_node_labels, use_edge_labels, None) if features is None else features
    if f.num_steps != H + 1:
        raise ValueError("features were built for %d iterations, not %d" % (f.num_steps - 1, H))
    return list(ops.wl_gram(f.ptr, f.color, f.count, f.step, f.num_graphs, f.num_steps, False).unbind(0))


# ------------------------------------------------------------------------------------------------ k = 2
class _K2:
    """What is k = 2's own (see "The engine" above)."""
    k, noun, cache, keyed = 2, "tuples", "_kwl_plans", ("pair", "a N + b")
    multisets = {False: (0, 1), True: (0, 1)}                               # the multiset of every exchange: one each, LWLC too
    max_nodes, max_entries = staticmethod(lambda: ops.kwl_max_nodes()), staticmethod(lambda: ops.kwl_max_entries())
    fused_enabled = staticmethod(lambda kernel: ops.kwl_fused_enabled())

    @staticmethod
    def too_many(p, count, H):
        if count > MAXNUMCOLOR // (H + 1):
            return "%d tuples, more than %d / (H + 1) = %d" % (count, MAXNUMCOLOR, MAXNUMCOLOR // (H + 1))

    @staticmethod
    def connected_items(p, g):
        """LWLC: (i, i) and the adjacent (i, j), by (i, j)."""
        v = np.concatenate([np.repeat(np.arange(g.N), g.deg), np.arange(g.N)])
        w = np.concatenate([g.nbr, np.arange(g.N)])
        order = np.lexsort((w, v))
        return g.sizes + (g.ptr[g.node_ptr[1:]] - g.ptr[g.node_ptr[:-1]]), [v[order], w[order]], False

    @staticmethod
    def graph_class(n2, graphs, g):
        return n2, g.to(graphs, np.int32)

    @staticmethod
    def launch_arrays(p, g):
        """row_ptr[a], the first tuple of row a: all pairs: the tuples of the earlier graphs + (a - first) n; LWLC: ptr[a] + a."""
        nodes = np.arange(g.N)
        row_ptr = g.ptr[:-1] + nodes if p.connected else p.tuple_ptr_h[:-1][g.node_graph] + (nodes - g.first) * g.sizes[g.node_graph]
        p.row_ptr, p.node_first = g.to(row_ptr, np.int32), g.to(g.first, np.int32)

    @staticmethod
    def init_fused(data, p, nl, el, out):
        ops.kwl_init(data.num_nodes, p.tup_v, p.tup_w, data.ptr, data.nbr, nl, el, out)

    @staticmethod
    def init_composed(data, p, nl, el, out):
        s, N = p.device_side(), data.num_nodes
        v, w = s["tup"]
        one = torch.ones_like(v)
        ci = ops.wl_pairing(nl[v] + 1, one) if nl is not None else one
        cj = ops.wl_pairing(nl[w] + 1, 2 * one) if nl is not None else 2 * one
        pos, adj = _member(s["ekey"], v * N + w)
        c = torch.where(v == w, one, 2 * one)
        if el is not None:
            lab = ops.wl_pairing(3 * one, el[pos.clamp(max=max(int(el.numel()) - 1, 0))]) if el.numel() else 3 * one
        else:
            lab = 3 * one
        out.copy_(ops.wl_pairing(ops.wl_pairing(ci, cj), torch.where(adj, lab, c)))

    @staticmethod
    def step_fused(data, p, cin, cout):
        if p.is_global:
            for n2, graphs in p.graph_classes:
                ops.kwl_global(data.num_graphs, graphs, n2, p.malkin, data.node_ptr, p.tuple_ptr, data.ptr, data.nbr, cin, cout, p.work)
        else:
            for group, lds, tuples in p.tuple_classes:
                ops.kwl_local(data.num_nodes, tuples, group, lds, p.connected, p.tup_v, p.tup_w, p.row_ptr, p.node_first, data.ptr,
                              data.nbr, cin, cout)


def _plan(data, kernel):
    return _plan_of(_K2, data, kernel)


def _check(data, num_iterations, kernel, use_node_labels, use_edge_labels):
    return _check_of(_K2, data, num_iterations, kernel, use_node_labels, use_edge_labels)


def kwl_colors(data, num_iterations, kernel, use_node_labels=True, use_edge_labels=True, workspace_keys=KWL_WORKSPACE_KEYS):
    """([H + 1, T] int64 (unsigned bit patterns): every tuple's colour after every iteration, tuple_ptr [B + 1] int32: where every
    graph's tuples start).  Launches only -- nothing is read back (classes and chunks were built with the plan)."""
    return _colors_of(_K2, data, num_iterations, kernel, use_node_labels, use_edge_labels, workspace_keys)


def kwl_features(data, num_iterations, kernel, use_node_labels=True, use_edge_labels=True, colors=None):
    """The feature CSR of the tuple colours (graph_kernels.WLFeatures): one map per graph over the colours of all iterations, with
    the position slices of the k = 1 WL kernel."""
    return _features_of(_K2, data, num_iterations, kernel, use_node_labels, use_edge_labels, colors)


def kwl_gram_matrices(data, num_iterations, kernel, use_node_labels=True, use_edge_labels=True, features=None):
    """The H + 1 un-normalised matrices [B, B] (int64), exactly the reference's.  With `features` given: one launch, nothing read back."""
    return _gram_matrices_of(_K2, data, num_iterations, kernel, use_node_labels, use_edge_labels, features)


# ------------------------------------------------------------------------------------------------ command line
def gram_file(gram_dir, dataset, kernel, h):
    """gram.cpp:195-250: <gram_dir>/<ds>__<kernel>2_<h>.gram."""
    return os.path.join(gram_dir, "%s__%s2_%d.gram" % (dataset, kernel, h))


def main(argv=None):
    argv = sys.argv[1:] if argv is None else list(argv)
    ap = gk.cli_parser("graph_kernels_kwl", "2-WL gram matrices (--k 2: WL, DWL, LWL, LWLC) in the reference's libsvm text; --k 1 is "
                                            "handed to graph_kernels_spgr")
    args = ap.parse_args(argv)
    if args.k == 1:
        from . import graph_kernels_spgr
        return graph_kernels_spgr.main(argv)
    if args.k != 2 or args.kernel not in KERNELS:
        ap.exit(2, "--k %d --kernel %s is not built: --k 2 takes --kernel WL, DWL, LWL or LWLC (and --k 1 WL, WLOA, SP or GR).  LWLP and "
                   "LWLPC are left out because the reference reads behind the end of its own colour maps there (GenerateTwo.cpp:579-580, "
                   "638, 650): there is no defined output to reproduce.  The k = 3 generators are not built either.\n"
                % (args.k, args.kernel))
    return gk.cli_run(args, gk.cli_per_iteration(args, gram_file, kwl_gram_matrices))


if __name__ == "__main__":
    sys.exit(main())
