"""The shortest-path (SP) and 3-node graphlet (GR) graph kernels, computed on the device: the other half of the reference's
graph-kernel tool at k = 1 (graph_classification/graph_kernels: `gram --kernel SP | GR`, driven by run.py) beside graph_kernels.py.

  reader, flags, text    as for WL                                            graph_kernels.GraphKernelData / dataset_flags / write_libsvm
  SP features            src/ShortestPathKernel.cpp:10-139                    sp_features   (dn_gk.hip: dn_gk_sp_u64, or composed)
  GR features            src/GraphletKernel.cpp:56-196                        gr_features   (dn_gk.hip: dn_gk_gr_keys_u64, or composed)
  gram matrix            F F^T                                                sp_gram_matrix / gr_gram_matrix (dn_wl_gram_i64, one step)
  command line           gram.cpp:176-193                                     python -m dummynode4graphlearning_amd.graph_kernels_spgr

Both feature builds end in graph_kernels.WLFeatures (one step, keys ascending unsigned per graph), so the gram matrix is the WL
kernel's launch.  Everything is exact integer arithmetic: the matrices equal the reference's entry for entry and the files byte for
byte (tests/spgr_ref.py restates the rules, tests/golden/graph_kernels_spgr.json holds the reference binary's text).

SP, the quirks.  d(a, b) is the hop distance, INT_MAX = 2147483647 where b cannot be reached -- a distance like any other, counted,
not dropped.  d(a, a) is 2 where a has a neighbour and INT_MAX where it has none (the reference's Floyd-Warshall runs in place over
j >= i).  Every ordered pair (a, b), a != b, adds 1 to the triple (lo32(l_a), l_b, d); a == b adds 2.  The first component is the
label truncated to 32 bits (the tuple's type), and the reference's filter reads IT, not the distance: a triple is dropped where
lo32(l_a) is 0 or INT_MAX, so a dummy node labelled 0 counts as b, never as a.  Edge labels are never used.  A key here is
(rank of lo32(l_a) * #labels + rank of l_b) in the high 32 bits and d in the low 32: only equality and a consistent order matter.

GR, the quirks.  Every unordered wedge u - v - w and every unordered triangle counts 1 (the reference counts ordered walks and divides
by 6).  The feature key is ONE unsigned 64-bit value: a wedge whose key equals a triangle's is the same feature.  Without node
labels the keys are 2 (wedge) and 3 (triangle) and edge labels are ignored; with them P(list) = the pairing fold started at the
list's length: wedge min(P[l_u, l_v, l_w], P[l_w, l_v, l_u]) or, with edge labels, min(P[l_u, e_uv, l_v, e_vw, l_w], P[reversed]);
triangle P(sorted labels) or the minimum over its six walks (GraphletKernel.cpp:108-113).

Fused and composed.  ops.gk_fused(on) picks the dn_gk_* kernels or the composed torch-op path (SP: padded dense adjacency per chunk
of graphs, levels by boolean products; GR: pair enumeration with repeat_interleave, searchsorted and ops.wl_pairing).  The composed
path also runs on CPU tensors, is the A/B partner, and takes the SP graphs above the fused classes (ops.gk_sp_lds_max_nodes()).

Refused with ValueError: node labels wanted without a node-label file, edge labels wanted (GR with node labels) without an
edge-label file, for SP a graph of more than 32,767 nodes (2 n^2 must fit the feature CSR's int32 count) or label ranks whose
product does not fit 32 bits, for GR a key workspace smaller than one work item.  The k >= 2 generators of the tool are not built.
"""
import os
import sys

import numpy as np
import torch

from . import graph_kernels as gk
from . import ops
from .graph_kernels import GraphKernelData, WLFeatures, dataset_flags, write_libsvm  # noqa: F401

INT_MAX = 2147483647
SP_MAX_NODES = 32767
GR_WORKSPACE_KEYS = 1 << 24          # 16 M pair slots: 128 MiB of keys and 64 MiB of graph ids per chunk
_GR_ITEM_PAIRS = 2048                # a hub's rows are grouped into work items of about this many pairs
_SP_COMPOSED_ELEMS = 1 << 22         # padded adjacency elements (graphs x nmax^2) per chunk of the composed SP path
KERNELS = ("SP", "GR")
_SIGN = ops._WL_SIGN


def _need_node_labels(data):
    if data.node_label is None:
        raise ValueError("%s: use_node_labels without node labels (no node-label file)"
                         % data.missing.get("node_labels", data.source + "[node_labels]"))


def _dev(data, a, dt):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a).astype(dt))).to(data.device)


def _reduce(g, key, w):
    """(graph, key, weight) entries in any order -> the distinct (graph, key) ascending by graph, then unsigned key, with summed
    weights.  Reads back the number of distinct entries."""
    if g.numel() == 0:
        return g, key, w
    k, o1 = torch.sort(key ^ _SIGN, stable=True)
    g2, o2 = torch.sort(g[o1], stable=True)
    k, w = k[o2], w[o1][o2]
    new = torch.ones_like(g2, dtype=torch.bool)
    new[1:] = (g2[1:] != g2[:-1]) | (k[1:] != k[:-1])
    uid = torch.cumsum(new, 0) - 1
    cnt = torch.zeros(int(uid[-1]) + 1, dtype=torch.int64, device=g.device).index_add_(0, uid, w)
    return g2[new], k[new] ^ _SIGN, cnt


def _features(data, g, key, cnt):
    rows = torch.bincount(g, minlength=data.num_graphs)
    ptr = torch.cat([rows.new_zeros(1), torch.cumsum(rows, 0)])
    return WLFeatures(ptr.to(torch.int32), key.contiguous(), cnt.to(torch.int32), torch.zeros_like(cnt, dtype=torch.int32), 1,
                      int(rows.max()))


def _gram(f):
    """[B, B] int64 = F F^T.  On the device this is dn_wl_gram_i64 (one launch, nothing read back); CPU tensors -- the composed
    path's host runs -- take a dense integer product."""
    B = f.num_graphs
    if f.color.numel() == 0:
        return torch.zeros((B, B), dtype=torch.int64, device=f.ptr.device)
    if f.color.is_cuda:
        return ops.wl_gram(f.ptr, f.color, f.count, f.step, B, 1, False)[0]
    col = torch.unique(f.color, return_inverse=True)[1]
    row = torch.repeat_interleave(torch.arange(B), torch.diff(f.ptr.long()))
    F = torch.zeros((B, int(col.max()) + 1), dtype=torch.int64)
    F[row, col] = f.count.long()
    return F @ F.t()


# ------------------------------------------------------------------------------------------------ SP
class _SPPlan:
    """Label ranks, the graphs' local label classes and the graph classes of one dataset, built once on the host."""

    def __init__(self, data, use_node_labels, lds_max_nodes):
        N, B = data.num_nodes, data.num_graphs
        if data.max_nodes > SP_MAX_NODES:
            raise ValueError("%s: graph %d has %d nodes, more than %d: 2 n^2 would not fit the feature CSR's int32 count"
                             % (data.source, data.largest_graph + 1, data.max_nodes, SP_MAX_NODES))
        lab = data.node_label.cpu().numpy().view(np.uint64) if use_node_labels else np.ones(N, dtype=np.uint64)
        lo32 = lab & np.uint64(0xffffffff)
        ua, ra = np.unique(lo32, return_inverse=True)
        ub, rb = np.unique(lab, return_inverse=True)
        if ua.size * ub.size > (1 << 32):
            raise ValueError("%s: %d distinct 32-bit source labels x %d distinct labels do not fit the key's 32 bits (rank overflow)"
                             % (data.source, ua.size, ub.size))
        base = ra.astype(np.int64) * ub.size
        base[(lo32 == 0) | (lo32 == INT_MAX)] = -1
        node_ptr = data.node_ptr.cpu().numpy().astype(np.int64)
        sizes = np.diff(node_ptr)
        node_graph = np.repeat(np.arange(B), sizes)
        uniq, inv = np.unique(node_graph * ub.size + rb, return_inverse=True)
        cls_ptr = np.concatenate([[0], np.cumsum(np.bincount(uniq // ub.size, minlength=B))])
        self.sizes, self.node_ptr_h = sizes, node_ptr
        self.src_base, self.rank_b = _dev(data, base, np.int64), _dev(data, rb, np.int64)
        self.local_class = _dev(data, inv - cls_ptr[node_graph], np.int32)
        self.class_ptr, self.class_rank = _dev(data, cls_ptr, np.int32), _dev(data, uniq % ub.size, np.int32)
        self.wave = np.nonzero(sizes <= 64)[0]
        self.block = np.nonzero((sizes > 64) & (sizes <= lds_max_nodes))[0]
        self.large = np.nonzero(sizes > max(64, lds_max_nodes))[0]
        self.block_nodes = int(sizes[self.block].max()) if self.block.size else 0
        self.wave_d, self.block_d = _dev(data, self.wave, np.int32), _dev(data, self.block, np.int32)


def _sp_plan(data, use_node_labels, lds_max_nodes):
    cache = data.__dict__.setdefault("_sp_plans", {})
    k = (bool(use_node_labels), int(lds_max_nodes))
    if k not in cache:
        cache[k] = _SPPlan(data, *k)
    return cache[k]


def _sp_composed(data, p, graphs):
    """(graph, key, weight) of the listed graphs by dense level-synchronous BFS: chunks of graphs of similar size, padded to the
    chunk's largest; level d + 1 = (frontier x adjacency > 0) and not yet seen."""
    dev, out = data.device, []
    order = graphs[np.argsort(p.sizes[graphs], kind="stable")]
    slot_graph = data.node_graph[data.slot_node]
    i = 0
    while i < order.size:
        j = i + 1
        while j < order.size and (j + 1 - i) * int(p.sizes[order[j]]) ** 2 <= _SP_COMPOSED_ELEMS:
            j += 1
        gl = order[i:j]
        i = j
        C, nmax = gl.size, int(p.sizes[gl].max())
        where = torch.full((data.num_graphs,), -1, dtype=torch.int64, device=dev)
        where[_dev(data, gl, np.int64)] = torch.arange(C, device=dev)
        first = _dev(data, p.node_ptr_h[gl], np.int64)
        size = _dev(data, p.sizes[gl], np.int64)
        slot = torch.nonzero(where[slot_graph] >= 0).squeeze(1)
        c = where[slot_graph[slot]]
        adj = torch.zeros((C, nmax, nmax), dtype=torch.bool, device=dev)
        adj[c, data.slot_node[slot] - first[c], data.nbr_long[slot] - first[c]] = True
        adjf = adj.to(torch.float32)
        eye = torch.eye(nmax, dtype=torch.bool, device=dev).unsqueeze(0)
        dist = torch.full((C, nmax, nmax), INT_MAX, dtype=torch.int64, device=dev)
        frontier, seen, d = adj & ~eye, adj | eye, 1
        while bool(frontier.any()):
            dist.masked_fill_(frontier, d)
            frontier = (torch.bmm(frontier.to(torch.float32), adjf) > 0) & ~seen
            seen |= frontier
            d += 1
        dist.diagonal(dim1=1, dim2=2).copy_(torch.where(adj.any(2), 2, INT_MAX))
        local = torch.arange(nmax, device=dev).unsqueeze(0)
        valid = local < size.unsqueeze(1)                                        # [C, nmax]
        node = (first.unsqueeze(1) + local).clamp(max=data.num_nodes - 1)
        base = torch.where(valid, p.src_base[node], torch.full_like(node, -1))
        keep = (base >= 0).unsqueeze(2) & valid.unsqueeze(1)
        key = ((base.unsqueeze(2) + p.rank_b[node].unsqueeze(1)) << 32) | dist
        g = _dev(data, gl, np.int64).view(C, 1, 1).expand(C, nmax, nmax)
        w = (1 + eye.to(torch.int64)).expand(C, nmax, nmax)
        out.append((g[keep], key[keep], w[keep]))
    return out


def sp_features(data, use_node_labels=True, lds_max_nodes=None):
    """The SP feature CSR (graph_kernels.WLFeatures, one step).  lds_max_nodes lowers the largest graph the workgroup class takes
    (default and upper bound: ops.gk_sp_lds_max_nodes()); larger graphs take the composed path."""
    if use_node_labels:
        _need_node_labels(data)
    fused = data.device.type == "cuda" and ops.gk_fused_enabled("SP")
    cap = 0
    if fused:
        cap = ops.gk_sp_lds_max_nodes()
        if lds_max_nodes is not None:
            if not 64 <= int(lds_max_nodes) <= cap:
                raise ValueError("lds_max_nodes must be 64 .. %d (got %d)" % (cap, lds_max_nodes))
            cap = int(lds_max_nodes)
    p = _sp_plan(data, use_node_labels, cap)
    parts = []
    if fused:
        launches = [(lst, grp, lds) for lst, grp, lds in ((p.wave_d, 64, 0), (p.block_d, 0, p.block_nodes)) if lst.numel()]
        args = (data.node_ptr, data.ptr, data.nbr, p.src_base, p.local_class, p.class_ptr, p.class_rank)
        counts = torch.zeros(data.num_nodes, dtype=torch.int32, device=data.device)
        for lst, grp, lds in launches:
            ops.gk_sp(data.num_graphs, lst, grp, lds, *args, counts=counts)
        cl = counts.long()
        ends = torch.cumsum(cl, 0)
        total = int(ends[-1])
        if total:
            key = torch.empty(total, dtype=torch.int64, device=data.device)
            cnt = torch.empty(total, dtype=torch.int32, device=data.device)
            offsets = (ends - cl).contiguous()
            for lst, grp, lds in launches:
                ops.gk_sp(data.num_graphs, lst, grp, lds, *args, offsets=offsets, out_key=key, out_count=cnt)
            parts.append((torch.repeat_interleave(data.node_graph, cl), key, cnt.long()))
        rest = p.large
    else:
        rest = np.arange(data.num_graphs)
    if rest.size:
        parts += _sp_composed(data, p, rest)
    if not parts:
        e = torch.zeros(0, dtype=torch.int64, device=data.device)
        return _features(data, e, e, e)
    return _features(data, *_reduce(*[torch.cat(x) for x in zip(*parts)]))


def sp_gram_matrix(data, use_node_labels=True, features=None):
    """[B, B] int64, exactly the reference's un-normalised SP matrix.  With `features` given: one launch, nothing read back."""
    return _gram(sp_features(data, use_node_labels) if features is None else features)


# ------------------------------------------------------------------------------------------------ GR
class _GRPlan:
    """The work items (centre, row range) of a dataset in node order, cut into chunks of at most workspace_keys pairs; per chunk the
    item lists of the 8-lane, the wavefront and the workgroup class."""

    def __init__(self, data, workspace_keys):
        ptr = data._ptr_h
        deg = np.diff(ptr)
        pairs = deg * (deg - 1) // 2
        whole = np.nonzero((pairs > 0) & (pairs <= 64))[0]
        hubs = np.nonzero(pairs > 64)[0]
        node, r0, r1, size = [whole], [np.zeros(whole.size, np.int64)], [deg[whole]], [pairs[whole]]
        if hubs.size:
            nrows = deg[hubs] - 1
            rep = np.repeat(np.arange(hubs.size), nrows)
            start = np.concatenate([[0], np.cumsum(nrows)])
            row = np.arange(rep.size) - start[rep]
            rsize = deg[hubs][rep] - 1 - row
            cum = np.cumsum(rsize) - rsize
            grp = (cum - cum[start[:-1]][rep]) // _GR_ITEM_PAIRS
            cut = np.nonzero(np.concatenate([[True], (rep[1:] != rep[:-1]) | (grp[1:] != grp[:-1])]))[0]
            last = np.concatenate([cut[1:], [rep.size]]) - 1
            node.append(hubs[rep[cut]])
            r0.append(row[cut])
            r1.append(row[last] + 1)
            size.append(np.add.reduceat(rsize, cut))
        node, r0, r1, size = (np.concatenate(x).astype(np.int64) for x in (node, r0, r1, size))
        order = np.lexsort((r0, node))
        node, r0, r1, size = node[order], r0[order], r1[order], size[order]
        group = np.where(pairs[node] <= 8, 8, np.where(pairs[node] <= 64, 64, 0))
        if size.size and int(size.max()) > workspace_keys:
            raise ValueError("%s: workspace_keys = %d is smaller than one work item (%d pairs)" % (data.source, workspace_keys, int(size.max())))
        ends = np.cumsum(size)
        self.chunks, self.pairs, i = [], int(ends[-1]) if size.size else 0, 0
        while i < size.size:
            j = int(np.searchsorted(ends, (ends[i - 1] if i else 0) + workspace_keys, side="right"))
            off = ends[i:j] - size[i:j] - (ends[i - 1] if i else 0)
            lists = []
            for grp_id in (8, 64, 0):
                m = group[i:j] == grp_id
                if m.any():
                    lists.append((grp_id, _dev(data, node[i:j][m], np.int32), _dev(data, r0[i:j][m], np.int32),
                                  _dev(data, r1[i:j][m], np.int32), _dev(data, off[m], np.int64)))
            # the composed path's rows: slot of u and the number of later slots, in workspace order
            nr = r1[i:j] - r0[i:j]
            rstart = np.concatenate([[0], np.cumsum(nr)])
            it = np.repeat(np.arange(j - i), nr)
            eu = ptr[node[i:j]][it] + r0[i:j][it] + (np.arange(it.size) - rstart[it])
            self.chunks.append(dict(used=int(ends[j - 1] - (ends[i - 1] if i else 0)), lists=lists, row_slot=_dev(data, eu, np.int64),
                                    row_size=_dev(data, ptr[node[i:j] + 1][it] - 1 - eu, np.int64)))
            i = j
        self.node_graph32 = data.node_graph.to(torch.int32)
        self.adj_key = data.slot_node * data.num_nodes + data.nbr_long


def _gr_plan(data, workspace_keys):
    cache = data.__dict__.setdefault("_gr_plans", {})
    if workspace_keys not in cache:
        cache[workspace_keys] = _GRPlan(data, workspace_keys)
    return cache[workspace_keys]


def _umin(a, b):
    return torch.where((a ^ _SIGN) < (b ^ _SIGN), a, b)


def _P(*xs):
    c = torch.full_like(xs[0], len(xs))
    for x in xs:
        c = ops.wl_pairing(c, x)
    return c


def _gr_composed_chunk(data, p, ch, nl, el):
    """(graph, key) of the counted pairs of one chunk, by torch ops."""
    rs = ch["row_size"]
    eu = torch.repeat_interleave(ch["row_slot"], rs)
    ew = eu + 1 + torch.arange(eu.numel(), device=data.device) - torch.repeat_interleave(torch.cumsum(rs, 0) - rs, rs)
    v, u, w = data.slot_node[eu], data.nbr_long[eu], data.nbr_long[ew]
    q = u * data.num_nodes + w
    pos = torch.searchsorted(p.adj_key, q).clamp(max=p.adj_key.numel() - 1)
    tri = p.adj_key[pos] == q
    if nl is None:
        key = torch.where(tri, torch.full_like(q, 3), torch.full_like(q, 2))
    else:
        lu, lv, lw = nl[u], nl[v], nl[w]
        if el is not None:
            uv, vw, uw = el[eu], el[ew], el[pos]
            wedge = _umin(_P(lu, uv, lv, vw, lw), _P(lw, vw, lv, uv, lu))
            walks = [_P(lu, uv, lv, vw, lw, uw), _P(lu, uw, lw, vw, lv, uv), _P(lv, uv, lu, uw, lw, vw), _P(lv, vw, lw, uw, lu, uv),
                     _P(lw, uw, lu, uv, lv, vw), _P(lw, vw, lv, uv, lu, uw)]
            tria = walks[0]
            for x in walks[1:]:
                tria = _umin(tria, x)
        else:
            wedge = _umin(_P(lu, lv, lw), _P(lw, lv, lu))
            s = torch.sort(torch.stack([lu, lv, lw], 1) ^ _SIGN, dim=1)[0] ^ _SIGN
            tria = _P(s[:, 0], s[:, 1], s[:, 2])
        key = torch.where(tri, tria, wedge)
    keep = ~tri | (v < u)
    return data.node_graph[v][keep], key[keep]


def gr_features(data, use_node_labels=True, use_edge_labels=True, workspace_keys=GR_WORKSPACE_KEYS):
    """The GR feature CSR (graph_kernels.WLFeatures, one step).  The centres' neighbour pairs are processed in chunks of at most
    workspace_keys pairs; every chunk is reduced (sort and run-length) before the next one is enumerated."""
    nl = el = None
    if use_node_labels:
        _need_node_labels(data)
        nl = data.node_label
        if use_edge_labels:
            if data.edge_label is None:
                raise ValueError("%s: use_edge_labels without edge labels (no edge-label file)"
                                 % data.missing.get("edge_labels", data.source + "[edge_labels]"))
            el = data.edge_label
    workspace_keys = int(workspace_keys)
    if workspace_keys < 1:
        raise ValueError("workspace_keys must be positive (got %d)" % workspace_keys)
    p = _gr_plan(data, workspace_keys)
    fused = data.device.type == "cuda" and ops.gk_fused_enabled("GR")
    parts = []
    if fused and p.chunks:
        size = max(ch["used"] for ch in p.chunks)
        ws_key = torch.empty(size, dtype=torch.int64, device=data.device)
        ws_gid = torch.empty(size, dtype=torch.int32, device=data.device)
    for ch in p.chunks:
        if fused:
            ws_gid.fill_(-1)
            for grp, node, r0, r1, off in ch["lists"]:
                ops.gk_gr_keys(data.num_nodes, grp, node, r0, r1, off, data.ptr, data.nbr, nl, el, p.node_graph32, ws_key, ws_gid)
            keep = ws_gid[:ch["used"]] >= 0
            g, key = ws_gid[:ch["used"]][keep].long(), ws_key[:ch["used"]][keep]
        else:
            g, key = _gr_composed_chunk(data, p, ch, nl, el)
        parts.append(_reduce(g, key, torch.ones_like(g)))
    if not parts:
        e = torch.zeros(0, dtype=torch.int64, device=data.device)
        return _features(data, e, e, e)
    if len(parts) == 1:
        return _features(data, *parts[0])
    return _features(data, *_reduce(*[torch.cat(x) for x in zip(*parts)]))


def gr_gram_matrix(data, use_node_labels=True, use_edge_labels=True, features=None, workspace_keys=GR_WORKSPACE_KEYS):
    """[B, B] int64, exactly the reference's un-normalised GR matrix (after its division by 6).  With `features` given: one launch,
    nothing read back."""
    return _gram(gr_features(data, use_node_labels, use_edge_labels, workspace_keys) if features is None else features)


# ------------------------------------------------------------------------------------------------ command line
def gram_file(gram_dir, dataset, kernel):
    """gram.cpp:182 / :191: <gram_dir>/<ds>__SP_0.gram, <gram_dir>/<ds>__GR_0.gram."""
    return os.path.join(gram_dir, "%s__%s_0.gram" % (dataset, kernel))


def main(argv=None):
    argv = sys.argv[1:] if argv is None else list(argv)
    ap = gk.cli_parser("graph_kernels_spgr", "SP / GR gram matrices in the reference's libsvm text (WL / WLOA: graph_kernels)")
    args = ap.parse_args(argv)
    if args.kernel in gk.KERNELS:
        return gk.main(argv)
    if args.k != 1 or args.kernel not in KERNELS:
        ap.exit(2, "--k %d --kernel %s is not built: only --k 1 with --kernel SP, GR, WL or WLOA is "
                   "(the k = 2 / k = 3 generators are not)\n" % (args.k, args.kernel))
    return gk.cli_run(args, lambda name, data, use_nl, use_el: [
        (gram_file(args.gram_dir, name, args.kernel), sp_gram_matrix(data, use_nl) if args.kernel == "SP" else gr_gram_matrix(data, use_nl, use_el))])


if __name__ == "__main__":
    sys.exit(main())
