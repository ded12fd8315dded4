"""The 2-WL graph kernels, computed on the device: the counterpart of the reference's graph-kernel tool at `gram --k 2 --kernel WL |
DWL | LWL | LWLC` (graph_classification/graph_kernels), for the datasets graph_kernels.GraphKernelData reads.

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

Refused with ValueError: what graph_kernels refuses, a graph with more than 1,000,000 / (H + 1) tuples (the reference's MAXNUMCOLOR
early stop is not built), and a dataset with 2^31 - 1 tuples or more.  `--k 3` and the kernels LWLP / LWLPC are not built: the
reference's LWLP / LWLPC dereference color_map_1.find(...) / color_map_2.find(...) on maps that are empty or keyed by other values
(GenerateTwo.cpp:579-580, 638, 650), so their output is whatever lies behind end().
"""
import os
import sys
import time

import numpy as np
import torch

from . import graph_kernels as gk
from . import ops
from .graph_kernels import MAXNUMCOLOR, GraphKernelData, WLFeatures, dataset_flags, write_libsvm  # noqa: F401

KERNELS = ("WL", "DWL", "LWL", "LWLC")
KWL_WORKSPACE_KEYS = 1 << 24          # multiset entries of one composed chunk (a handful of int64 arrays of that length live at once)
_I64_MAX = (1 << 63) - 1


class _Plan:
    """The tuples of a dataset under one kernel and everything the launches need, built once on the host."""

    def __init__(self, data, kernel):
        dev = data.device
        to = lambda a, dt: torch.from_numpy(np.ascontiguousarray(np.asarray(a).astype(dt))).to(dev)  # noqa: E731
        node_ptr = data.node_ptr.cpu().numpy().astype(np.int64)
        ptr, N, B = data._ptr_h, data.num_nodes, data.num_graphs
        sizes, deg = np.diff(node_ptr), np.diff(ptr)
        node_graph = np.repeat(np.arange(B), sizes)
        first = node_ptr[:-1][node_graph]
        self.kernel, self.connected, self.malkin, self.is_global = kernel, kernel == "LWLC", kernel == "DWL", kernel in ("WL", "DWL")
        if self.connected:
            nbr = data.nbr.cpu().numpy().astype(np.int64)
            v = np.concatenate([np.repeat(np.arange(N), deg), np.arange(N)])
            w = np.concatenate([nbr, np.arange(N)])
            order = np.lexsort((w, v))
            tup_v, tup_w = v[order], w[order]
            count = sizes + (ptr[node_ptr[1:]] - ptr[node_ptr[:-1]])
            row_ptr = ptr[:-1] + np.arange(N)
        else:
            count = sizes * sizes
        tuple_ptr = np.concatenate([[0], np.cumsum(count)])
        T = int(tuple_ptr[-1])
        self.count, self.tuple_ptr_h, self.num_tuples = count, tuple_ptr, T
        self.largest = int(count.argmax())
        if T >= (1 << 31) - 1:
            return                                                          # (refused by _check before anything is used)
        if not self.connected:
            local = np.arange(T) - np.repeat(tuple_ptr[:-1], count)
            n_t, base_t = np.repeat(sizes, count), np.repeat(node_ptr[:-1], count)
            tup_v, tup_w = base_t + local // n_t, base_t + local % n_t
            row_ptr = tuple_ptr[:-1][node_graph] + (np.arange(N) - first) * sizes[node_graph]
        self.tup_v, self.tup_w = to(tup_v, np.int32), to(tup_w, np.int32)
        self.row_ptr, self.node_first = to(row_ptr, np.int32), to(first, np.int32)
        self.tuple_ptr = to(tuple_ptr, np.int32)
        self.tuple_graph = to(np.repeat(np.arange(B), count), np.int64)
        # the fused launches: graph classes by the power of two above the size (WL / DWL), tuple classes by the longer list (LWL / LWLC)
        if self.is_global:
            fused_graph = sizes <= ops.kwl_max_nodes()
            n2 = np.maximum(8, 1 << np.ceil(np.log2(np.maximum(sizes, 1))).astype(np.int64))
            self.graph_classes = [(int(c), to(np.nonzero(fused_graph & (n2 == c))[0], np.int32)) for c in np.unique(n2[fused_graph])]
            self.work = torch.empty((2 if self.malkin else 1) * T, dtype=torch.int64, device=dev)
        else:
            cap = ops.kwl_max_entries()
            gmax = np.zeros(B, dtype=np.int64)
            np.maximum.at(gmax, node_graph, deg)
            fused_graph = gmax <= cap
            longer = np.maximum(deg[tup_v], deg[tup_w])
            ok = fused_graph[node_graph[tup_v]]
            pick = lambda m: to(np.nonzero(m & ok)[0], np.int32)  # noqa: E731
            block = (longer > 64) & ok
            lds = 1 << int(longer[block].max() - 1).bit_length() if block.any() else 0
            self.tuple_classes = [(grp, l, t) for grp, l, t in ((8, 0, pick(longer <= 8)), (64, 0, pick((longer > 8) & (longer <= 64))),
                                                                (0, lds, pick(longer > 64))) if t.numel()]
        self.fused_graph = fused_graph
        # the composed path's per-tuple costs: candidates (before the copies) and entries (with them)
        self._tup_graph_h = node_graph[tup_v]
        if self.is_global:
            n_t = sizes[self._tup_graph_h]
            self._cand, self._phys = 2 * n_t, 4 * n_t + 2
        else:
            self._cand = deg[tup_v] + deg[tup_w]
            self._phys = 2 * self._cand
        self._deg1_h = deg[tup_v]
        self._chunks = {}
        self._dev = None
        self._data = data

    def device_side(self):
        """Arrays only the composed path needs (built on its first use)."""
        if self._dev is None:
            d, N = self._data, self._data.num_nodes
            dev = d.device
            sizes = (d.node_ptr[1:] - d.node_ptr[:-1]).long()
            ekey = torch.cat([d.slot_node * N + d.nbr_long, torch.full((1,), _I64_MAX, dtype=torch.int64, device=dev)])
            tkey = torch.cat([self.tup_v.long() * N + self.tup_w.long(), torch.full((1,), _I64_MAX, dtype=torch.int64, device=dev)])
            self._dev = dict(ekey=ekey, tkey=tkey, gsize=sizes[d.node_graph], first=self.node_first.long(), row_ptr=self.row_ptr.long(),
                             ptr=d.ptr.long(), deg=(d.ptr[1:] - d.ptr[:-1]).long(), tup_v=self.tup_v.long(), tup_w=self.tup_w.long())
        return self._dev

    def chunks(self, everything, workspace_keys):
        """Runs of tuples of at most workspace_keys entries each (a single tuple with more is a run of its own): of every graph, or of
        the graphs the fused kernels leave out.  [(tuple ids int64, candidates of type 1, candidates of type 2, entries)]."""
        key = (bool(everything), int(workspace_keys))
        if key not in self._chunks:
            ids = np.arange(self.num_tuples) if everything else np.nonzero(~self.fused_graph[self._tup_graph_h])[0]
            out, a = [], 0
            if ids.size:
                run = np.cumsum(self._phys[ids])
                while a < ids.size:
                    b = int(np.searchsorted(run, (run[a - 1] if a else 0) + workspace_keys, side="right"))
                    b = min(max(b, a + 1), a + workspace_keys)               # (tuples without entries: bounded by their number)
                    t = ids[a:b]
                    if self.is_global:
                        c1 = c2 = int(self._cand[t].sum()) // 2
                    else:
                        c1 = int(self._deg1_h[t].sum())
                        c2 = int(self._cand[t].sum()) - c1
                    out.append((torch.from_numpy(t.astype(np.int64)).to(self._data.device), c1, c2, int(self._phys[t].sum())))
                    a = b
            self._chunks[key] = out
        return self._chunks[key]


def _plan(data, kernel):
    plans = data.__dict__.setdefault("_kwl_plans", {})
    if kernel not in plans:
        plans[kernel] = _Plan(data, kernel)
    return plans[kernel]


def _check(data, num_iterations, kernel, use_node_labels, use_edge_labels):
    if kernel not in KERNELS:
        raise ValueError("kernel %r is not built at k = 2: WL, DWL, LWL and LWLC are (LWLP / LWLPC read behind the end of the reference's "
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
    if int(p.count.max()) > MAXNUMCOLOR // (H + 1):
        raise ValueError("%s: graph %d has %d tuples, more than %d / (H + 1) = %d: the reference's MAXNUMCOLOR early stop is not built"
                         % (data.source, p.largest + 1, int(p.count.max()), MAXNUMCOLOR, MAXNUMCOLOR // (H + 1)))
    if p.num_tuples >= (1 << 31) - 1:
        raise ValueError("%s: %d tuples, more than 2^31 - 2" % (data.source, p.num_tuples))
    return H, p


# ------------------------------------------------------------------------------------------------ composed path
def _member(sorted_keys, q):
    """(position, is q in the ascending keys?); sorted_keys ends with a sentinel above every query."""
    pos = torch.searchsorted(sorted_keys, q)
    return pos, sorted_keys[pos] == q


def _expand(count, total):
    """Ragged expansion: (owner of every item, its position within its owner) for `total` = count.sum() items (known on the host)."""
    owner = torch.repeat_interleave(torch.arange(count.numel(), device=count.device), count, output_size=total)
    start = torch.cumsum(count, 0) - count
    return owner, torch.arange(total, device=count.device) - start[owner]


def _init_composed(data, p, nl, el, out):
    s, N = p.device_side(), data.num_nodes
    v, w = s["tup_v"], s["tup_w"]
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


def _combine(own, fold, has):
    """own [t], fold / has [t, 4] in the order (local 1, local 2, global 1, global 2)."""
    l1, l2, g1, g2 = fold.unbind(1)
    h = has.unbind(1)
    swap_l = h[0] & h[1] & ((l1 ^ ops._WL_SIGN) > (l2 ^ ops._WL_SIGN))
    swap_g = h[2] & h[3] & ((g1 ^ ops._WL_SIGN) > (g2 ^ ops._WL_SIGN))
    l1, l2 = torch.where(swap_l, l2, l1), torch.where(swap_l, l1, l2)
    g1, g2 = torch.where(swap_g, g2, g1), torch.where(swap_g, g1, g2)
    acc = own
    for f, ok in ((l1, h[0]), (l2, h[1]), (g1, h[2]), (g2, h[3])):
        acc = torch.where(ok, ops.wl_pairing(acc, f), acc)
    return acc


def _step_composed(data, p, chunks, cin, cout):
    s, N = p.device_side(), data.num_nodes
    for tids, c1, c2, phys in chunks:
        v, w = s["tup_v"][tids], s["tup_w"][tids]
        Tc = int(tids.numel())
        trash = 4 * Tc
        segs, idxs, mults = [], [], []
        for typ, total in ((0, c1), (1, c2)):
            if total == 0:
                continue
            moved = w if typ else v                                          # the component that is exchanged
            if p.is_global:
                ti, j = _expand(s["gsize"][v], total)
                x = s["first"][v][ti] + j
            else:
                ti, j = _expand(s["deg"][moved], total)
                x = data.nbr_long[s["ptr"][moved][ti] + j]
            a, b = (v[ti], x) if typ else (x, w[ti])                        # the tuple whose colour is gathered
            drop = torch.zeros_like(x, dtype=torch.bool)
            if p.connected:
                idx, hit = _member(s["tkey"], a * N + b)
                drop = ~hit
                idx = idx.clamp(max=p.num_tuples - 1)
            else:
                idx = s["row_ptr"][a] + (b - s["first"][a])
            mult = torch.full_like(x, 2)
            glob = torch.zeros_like(x)
            if p.is_global:
                own = x == moved[ti]
                if typ:
                    drop = own                                               # type 2 leaves the tuple itself out
                else:
                    mult = torch.where(own, 2 * mult, mult)                  # type 1 holds it four times
                if p.malkin:
                    adj = _member(s["ekey"], moved[ti] * N + x)[1]
                    glob = (own | ~adj).long()
            segs.append(torch.where(drop, torch.full_like(x, trash), ti * 4 + typ + 2 * glob))
            idxs.append(idx)
            mults.append(mult)
        if not segs:
            cout[tids] = cin[tids]
            continue
        mult = torch.cat(mults)
        rep = torch.repeat_interleave(torch.arange(mult.numel(), device=mult.device), mult, output_size=phys)
        fold, size = ops.kwl_fold_from_max(torch.cat(segs)[rep], cin[torch.cat(idxs)][rep], trash)
        cout[tids] = _combine(cin[tids], fold.view(Tc, 4), size.view(Tc, 4) > 0)


# ------------------------------------------------------------------------------------------------ colours
def _step(data, p, cin, cout, workspace_keys):
    if not ops.kwl_fused_enabled():
        _step_composed(data, p, p.chunks(True, workspace_keys), cin, cout)
        return
    if p.is_global:
        for n2, graphs in p.graph_classes:
            ops.kwl_global(data.num_graphs, graphs, n2, p.malkin, data.node_ptr, p.tuple_ptr, data.ptr, data.nbr, cin, cout, p.work)
    else:
        for group, lds, tuples in p.tuple_classes:
            ops.kwl_local(data.num_nodes, tuples, group, lds, p.connected, p.tup_v, p.tup_w, p.row_ptr, p.node_first, data.ptr, data.nbr,
                          cin, cout)
    if not p.fused_graph.all():
        _step_composed(data, p, p.chunks(False, workspace_keys), cin, cout)


def kwl_colors(data, num_iterations, kernel, use_node_labels=True, use_edge_labels=True, workspace_keys=KWL_WORKSPACE_KEYS):
    """([H + 1, T] int64 (unsigned bit patterns): every tuple's colour after every iteration, tuple_ptr [B + 1] int32: where every
    graph's tuples start).  Launches only -- nothing is read back (classes and chunks were built with the plan)."""
    H, p = _check(data, num_iterations, kernel, use_node_labels, use_edge_labels)
    workspace_keys = int(workspace_keys)
    if workspace_keys < 1:
        raise ValueError("workspace_keys must be positive (got %d)" % workspace_keys)
    nl = data.node_label if use_node_labels else None
    el = data.edge_label if use_edge_labels else None
    c = torch.empty((H + 1, p.num_tuples), dtype=torch.int64, device=data.device)
    if ops.kwl_fused_enabled():
        ops.kwl_init(data.num_nodes, p.tup_v, p.tup_w, data.ptr, data.nbr, nl, el, c[0])
    else:
        _init_composed(data, p, nl, el, c[0])
    for h in range(1, H + 1):
        _step(data, p, c[h - 1], c[h], workspace_keys)
    return c, p.tuple_ptr


# ------------------------------------------------------------------------------------------------ features and matrices
def kwl_features(data, num_iterations, kernel, use_node_labels=True, use_edge_labels=True, colors=None):
    """The feature CSR of the tuple colours (graph_kernels.WLFeatures): one map per graph over the colours of all iterations, with
    the position slices of the k = 1 WL kernel."""
    H, p = _check(data, num_iterations, kernel, use_node_labels, use_edge_labels)
    c = kwl_colors(data, H, kernel, use_node_labels, use_edge_labels)[0] if colors is None else colors
    return gk.features_of_colors(p.tuple_graph, c, data.num_graphs)


def kwl_gram_matrices(data, num_iterations, kernel, use_node_labels=True, use_edge_labels=True, features=None):
    """The H + 1 un-normalised matrices [B, B] (int64), exactly the reference's.  With `features` given: one launch, nothing read back."""
    H, _ = _check(data, num_iterations, kernel, use_node_labels, use_edge_labels)
    if H + 1 > ops.wl_max_steps():
        raise ValueError("num_iterations + 1 = %d exceeds the gram kernel's %d steps" % (H + 1, ops.wl_max_steps()))
    f = kwl_features(data, H, kernel, use_node_labels, use_edge_labels) if features is None else features
    if f.num_steps != H + 1:
        raise ValueError("features were built for %d iterations, not %d" % (f.num_steps - 1, H))
    return list(ops.wl_gram(f.ptr, f.color, f.count, f.step, f.num_graphs, f.num_steps, False).unbind(0))


# ------------------------------------------------------------------------------------------------ command line
def gram_file(gram_dir, dataset, kernel, h):
    """gram.cpp:195-250: <gram_dir>/<ds>__<kernel>2_<h>.gram."""
    return os.path.join(gram_dir, "%s__%s2_%d.gram" % (dataset, kernel, h))


def main(argv=None):
    import argparse
    argv = sys.argv[1:] if argv is None else list(argv)
    ap = argparse.ArgumentParser(prog="python -m dummynode4graphlearning_amd.graph_kernels_kwl",
                                 description="2-WL gram matrices (--k 2: WL, DWL, LWL, LWLC) in the reference's libsvm text; --k 1 is "
                                             "handed to graph_kernels_spgr")
    ap.add_argument("--dataset_dir", default="./datasets")
    ap.add_argument("--gram_dir", default="./svm/GM/EXP")
    ap.add_argument("--k", type=int, default=1)
    ap.add_argument("--kernel", default="WL")
    ap.add_argument("--n_iters", type=int, default=1)
    ap.add_argument("--datasets", nargs="*", default=[])
    ap.add_argument("--device", default="cuda")
    args = ap.parse_args(argv)
    if args.k == 1:
        from . import graph_kernels_spgr
        return graph_kernels_spgr.main(argv)
    if args.k != 2 or args.kernel not in KERNELS:
        ap.exit(2, "--k %d --kernel %s is not built: --k 2 takes --kernel WL, DWL, LWL or LWLC (and --k 1 WL, WLOA, SP or GR).  LWLP and "
                   "LWLPC are left out because the reference reads behind the end of its own colour maps there (GenerateTwo.cpp:579-580, "
                   "638, 650): there is no defined output to reproduce.  The k = 3 generators are not built either.\n"
                % (args.k, args.kernel))
    jobs = []
    for name in args.datasets:
        if name not in gk.DATASET_FLAGS:
            print("Warning: %s is not a valid dataset." % name)
        jobs.append((name, GraphKernelData.from_dir(args.dataset_dir, name, device=args.device)) + dataset_flags(name))
    for name, data, use_nl, use_el in jobs:
        t0 = time.time()
        for h, G in enumerate(kwl_gram_matrices(data, args.n_iters, args.kernel, use_nl, use_el)):
            write_libsvm(G, data.classes, gram_file(args.gram_dir, name, args.kernel, h))
        print("%s-%d\t%s\t%d seconds" % (args.kernel, args.n_iters, name, int(time.time() - t0)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
