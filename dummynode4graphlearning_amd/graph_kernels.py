"""WL and WLOA graph kernels at k = 1, computed on the device: the counterpart of the reference's graph-kernel tool
(graph_classification/graph_kernels: `gram --k 1 --kernel WL | WLOA`, driven by run.py) for the datasets tu_io.process_dataset writes.

  reader                 src/AuxiliaryMethods.cpp:41-342, gram.cpp:106-115    GraphKernelData.from_dir / from_arrays (host text -> CSR)
  per-dataset flags      gram.cpp:17-36                                       DATASET_FLAGS / dataset_flags
  colour refinement      src/ColorRefinementKernel.cpp:171-306                wl_colors      (dn_wl.hip: dn_wl_refine_u64 / dn_wl_fold_u64)
  per-graph colour maps  :199-305 (the std::map and the colour numbers)       wl_features    (torch device ops, one-off per dataset)
  gram matrices          :80-169                                              wl_gram_matrices (dn_wl.hip: dn_wl_gram_i64)
  normalised text        AuxiliaryMethods.cpp:437-485                         normalize_gram / write_libsvm
  command line           gram.cpp:38-104, 117-175                             python -m dummynode4graphlearning_amd.graph_kernels

Everything up to the normalisation is exact unsigned 64-bit integer arithmetic that wraps (colours travel as int64 bit patterns),
so the integer matrices equal the reference's entry for entry; tests/wl_ref.py restates the arithmetic in plain Python and
tests/golden/graph_kernels.json holds the text the reference's own binary wrote.

The ordering quirk.  Matrix h does not use "the colours of iterations 0..h": per graph the reference keeps ONE map of all colours of
all iterations, ordered by colour VALUE, and hands matrix h the entries at sorted POSITIONS [nums[h - 1], nums[h]), nums[h] being the
number of distinct colours after iteration h, with each entry's FINAL count.  While new colours are larger than old ones the two
readings agree; once the pairing function wraps around 2^64 (the normal case from the second iteration on) they do not, and the
slice is what is reproduced here: every feature entry carries the step whose slice holds its position.

Refused with ValueError (the reference handles these by accident or by undefined behaviour): a self loop (it would list the node
twice), an `A` line that joins two graphs, edge labels wanted without an edge-label file (it dereferences end()), node labels wanted
without a node-label file, an edge label above 2^32 - 1 (its edge-label map truncates to 32 bits), and a graph with more than
1,000,000 / (H + 1) nodes (its MAXNUMCOLOR early stop is not built).  SP and GR live in graph_kernels_spgr.py (its command line takes all
four kernels), the k = 2 kernels in graph_kernels_kwl.py (on features_of_colors below); this command line keeps refusing both.
"""
import os
import sys
import time

import numpy as np
import torch

from . import ops

MAXNUMCOLOR = 1000000

# gram.cpp:17-36 as data: name -> (use_node_labels, use_edge_labels); any other name gets (True, True) and a warning
DATASET_FLAGS = {
    "ENZYMES": (True, False), "DD": (True, False), "IMDB-BINARY": (True, False), "IMDB-MULTI": (True, False), "MUTAG": (True, True),
    "NCI1": (True, False), "NCI109": (True, False), "PTC_FM": (True, False), "PTC_FR": (True, False), "PROTEINS": (True, False),
    "REDDIT-BINARY": (False, False), "Yeast": (True, True), "YeastH": (True, True), "UACC257": (True, True), "UACC257H": (True, True),
    "OVCAR-8": (True, True), "OVCAR-8H": (True, True),
}
KERNELS = ("WL", "WLOA")


def dataset_flags(name):
    """(use_node_labels, use_edge_labels) of a dataset name; (True, True) for a name outside the table."""
    return DATASET_FLAGS.get(name, (True, True))


# ------------------------------------------------------------------------------------------------ reader
def _read_column(path, what):
    """One unsigned integer per line -> list of Python ints; ValueError names the file and the line."""
    out = []
    with open(path) as f:
        for ln, line in enumerate(f, 1):
            try:
                out.append(int(line.strip()))
            except ValueError:
                raise ValueError("%s:%d: %r is not %s" % (path, ln, line.strip(), what))
    return out


def _find(dataset_dir, name, kind):
    """<dir>/<name>/<name>_<kind>.txt, else <dir>/<name>/raw/<name>_<kind>.txt, else None."""
    for sub in ("", "raw"):
        p = os.path.join(dataset_dir, name, sub, "%s_%s.txt" % (name, kind))
        if os.path.exists(p):
            return p
    return None


class _Plan:
    """The node classes of one refinement flavour (entries = deg, or 2 deg with edge labels), built once on the host: node lists
    for the 8-lane, the 64-lane and the workgroup launches, and for lists above ops.wl_max_entries() the composed path's slots."""

    def __init__(self, ptr_h, mult, device, cap):
        deg = np.diff(ptr_h)
        ent = deg * mult
        dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a.astype(dt))).to(device)  # noqa: E731
        pick = lambda m: dev(np.nonzero(m)[0], np.int32)  # noqa: E731
        self.small, self.wave = pick(ent <= 8), pick((ent > 8) & (ent <= 64))
        big = (ent > 64) & (ent <= cap)
        self.block = pick(big)
        self.block_lds = 1 << int(ent[big].max() - 1).bit_length() if big.any() else 0
        huge = np.nonzero(ent > cap)[0]
        self.huge = dev(huge, np.int32)
        if huge.size:
            slots = np.concatenate([np.arange(ptr_h[v], ptr_h[v + 1]) for v in huge])
            self.huge_slots = dev(slots, np.int64)
            self.huge_seg = dev(np.repeat(np.arange(huge.size), deg[huge]), np.int64)
            self.huge_ptr = dev(np.concatenate([[0], np.cumsum(ent[huge])]), np.int64)
        self.all_ptr = dev(ptr_h.astype(np.int64) * mult, np.int64)


class GraphKernelData:
    """A whole TU dataset as the graph-kernel tool sees it, on one device: simple undirected graphs as one deduplicated CSR over
    global node ids (ptr [N + 1], nbr [2 E] int32, ascending per node), the label of every slot (edge_label [2 E] int64 or None),
    node labels as unsigned 64-bit patterns (node_label [N] int64 or None), node_ptr [B + 1] and the graphs' classes."""

    def __init__(self, node_ptr, ptr, nbr, edge_label, node_label, classes, device, source="<arrays>"):
        self.device = torch.device(device)
        self.source = source
        self.num_graphs, self.num_nodes = int(node_ptr.size - 1), int(node_ptr[-1])
        if self.num_graphs < 1 or self.num_nodes < 1:
            raise ValueError("%s: an empty dataset (%d graphs, %d nodes)" % (source, self.num_graphs, self.num_nodes))
        self.classes = None if classes is None else [int(c) for c in classes]
        if self.classes is not None and len(self.classes) != self.num_graphs:
            raise ValueError("%s: %d graph labels for %d graphs" % (source, len(self.classes), self.num_graphs))
        sizes = np.diff(node_ptr)
        self.max_nodes, self.largest_graph = int(sizes.max()), int(sizes.argmax())
        dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a.astype(dt))).to(self.device)  # noqa: E731
        self._ptr_h = ptr.astype(np.int64)
        self.node_ptr, self.ptr, self.nbr = dev(node_ptr, np.int32), dev(ptr, np.int32), dev(nbr, np.int32)
        self.nbr_long = self.nbr.long()
        self.slot_node = dev(np.repeat(np.arange(self.num_nodes), np.diff(ptr)), np.int64)
        self.node_graph = dev(np.repeat(np.arange(self.num_graphs), sizes), np.int64)
        self.edge_label = None if edge_label is None else dev(edge_label.view(np.int64), np.int64)
        self.node_label = None if node_label is None else dev(node_label.view(np.int64), np.int64)
        self._plans = {}

    def plan(self, use_edge_labels):
        mult = 2 if use_edge_labels else 1
        if mult not in self._plans:
            self._plans[mult] = _Plan(self._ptr_h, mult, self.device, ops.wl_max_entries())
        return self._plans[mult]

    @classmethod
    def from_arrays(cls, graph_indicator=None, A=None, node_labels=None, edge_labels=None, graph_labels=None, device="cuda", batch=None,
                    source="<arrays>", files=None):
        """From the raw TU arrays (graph_indicator [N] 1-based, A [E, 2] 1-based node ids in file order, optional labels), or from
        batch = a tu_io.TUBatch (node_ptr, src, dst, node_label, edge_label; graph_labels separately).  `files` names the files the
        arrays came from, for the messages."""
        files = files or {}
        where = lambda kind, ln: "%s:%d" % (files.get(kind, "%s[%s]" % (source, kind)), ln)  # noqa: E731
        if batch is not None:
            h = {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in batch.items()}
            sizes = np.diff(h["node_ptr"].astype(np.int64))
            graph_indicator = np.repeat(np.arange(1, sizes.size + 1), sizes)
            A = np.stack([h["src"].astype(np.int64) + 1, h["dst"].astype(np.int64) + 1], 1)
            node_labels, edge_labels = h.get("node_label"), h.get("edge_label")
        gi = np.asarray(graph_indicator, dtype=np.int64).reshape(-1)
        A = np.asarray(A, dtype=np.int64).reshape(-1, 2)
        N = gi.size
        if N == 0 or gi[0] < 1 or (np.diff(gi) < 0).any():
            bad = 1 if N == 0 or gi[0] < 1 else int(np.nonzero(np.diff(gi) < 0)[0][0]) + 2
            raise ValueError("%s: graph ids must start at 1 or above and never decrease" % where("graph_indicator", bad))
        B = int(gi[-1])                                                         # the LAST value, as the reference takes it
        node_ptr = np.concatenate([[0], np.cumsum(np.bincount(gi - 1, minlength=B))]).astype(np.int64)

        def u64(values, kind, count):
            if values is None:
                return None
            vals = [int(x) for x in (values.tolist() if isinstance(values, np.ndarray) else values)]
            if len(vals) != count:
                raise ValueError("%s: %d labels for %d %s" % (where(kind, len(vals) + 1), len(vals), count,
                                                              "nodes" if kind == "node_labels" else "lines of A"))
            for ln, x in enumerate(vals, 1):
                if x < 0 or x >= (1 << 64):
                    raise ValueError("%s: label %d is not an unsigned 64-bit value" % (where(kind, ln), x))
                if kind == "edge_labels" and x >= (1 << 32):
                    raise ValueError("%s: edge label %d does not fit the reference's 32-bit edge-label map" % (where(kind, ln), x))
            return np.array(vals, dtype=np.uint64)

        nl, el = u64(node_labels, "node_labels", N), u64(edge_labels, "edge_labels", A.shape[0])
        v, w = A[:, 0] - 1, A[:, 1] - 1
        if A.shape[0]:
            oob = (v < 0) | (v >= N) | (w < 0) | (w >= N)
            if oob.any():
                raise ValueError("%s: node id outside 1..%d" % (where("A", int(np.nonzero(oob)[0][0]) + 1), N))
            loop = v == w
            if loop.any():
                ln = int(np.nonzero(loop)[0][0])
                raise ValueError("%s: self loop on node %d (the reference would list the node twice as its own neighbour)"
                                 % (where("A", ln + 1), int(v[ln]) + 1))
            cross = gi[v] != gi[w]
            if cross.any():
                ln = int(np.nonzero(cross)[0][0])
                raise ValueError("%s: nodes %d and %d belong to different graphs" % (where("A", ln + 1), int(v[ln]) + 1, int(w[ln]) + 1))
        # one undirected edge per unordered pair, labelled by the FIRST line that names it in either order
        key = np.minimum(v, w) * N + np.maximum(v, w)
        _, first = np.unique(key, return_index=True)
        lo, hi = np.minimum(v, w)[first], np.maximum(v, w)[first]
        src, dst = np.concatenate([lo, hi]), np.concatenate([hi, lo])
        order = np.lexsort((dst, src))
        ptr = np.concatenate([[0], np.cumsum(np.bincount(src, minlength=N))]).astype(np.int64)
        if ptr[-1] >= (1 << 31) - 1 or N >= (1 << 31) - 1:
            raise ValueError("%s: more than 2^31 - 2 nodes or adjacency slots" % source)
        slot_label = None if el is None else np.concatenate([el[first], el[first]])[order]
        return cls(node_ptr, ptr, dst[order], slot_label, nl, graph_labels, device, source=source)

    @classmethod
    def from_dir(cls, dataset_dir, name, device="cuda"):
        """The reference's reader: <dir>/<name>/<name>_*.txt, else <dir>/<name>/raw/<name>_*.txt."""
        files = {k: _find(dataset_dir, name, k) for k in ("graph_indicator", "A", "node_labels", "edge_labels", "graph_labels")}
        for k in ("graph_indicator", "A", "graph_labels"):
            if files[k] is None:
                raise FileNotFoundError("%s_%s.txt not found under %s (nor its raw/)" % (name, k, os.path.join(dataset_dir, name)))
        gi = _read_column(files["graph_indicator"], "a graph id")
        A = []
        with open(files["A"]) as f:
            for ln, line in enumerate(f, 1):
                parts = line.replace(",", " ").split()
                try:
                    if len(parts) != 2:
                        raise ValueError
                    A.append((int(parts[0]), int(parts[1])))
                except ValueError:
                    raise ValueError("%s:%d: %r is not a pair of node ids" % (files["A"], ln, line.strip()))
        nl = None if files["node_labels"] is None else _read_column(files["node_labels"], "an unsigned node label")
        el = None if files["edge_labels"] is None else _read_column(files["edge_labels"], "an unsigned edge label")
        data = cls.from_arrays(gi, np.array(A, dtype=np.int64).reshape(-1, 2), nl, el, _read_column(files["graph_labels"], "a class"),
                               device=device, source=os.path.join(dataset_dir, name), files={k: p for k, p in files.items() if p})
        data.missing = {k: os.path.join(dataset_dir, name, "%s_%s.txt" % (name, k)) for k in ("node_labels", "edge_labels")
                        if files[k] is None}
        return data

    missing = {}


def _check(data, num_iterations, use_node_labels, use_edge_labels):
    H = int(num_iterations)
    if H < 0:
        raise ValueError("num_iterations must be >= 0 (got %d)" % H)
    if use_node_labels and data.node_label is None:
        raise ValueError("%s: use_node_labels without node labels (no node-label file)"
                         % data.missing.get("node_labels", data.source + "[node_labels]"))
    if use_edge_labels and data.edge_label is None:
        raise ValueError("%s: use_edge_labels without edge labels (no edge-label file; the reference dereferences end() here)"
                         % data.missing.get("edge_labels", data.source + "[edge_labels]"))
    if data.max_nodes > MAXNUMCOLOR // (H + 1):
        raise ValueError("%s: graph %d has %d nodes, more than %d / (H + 1) = %d: the reference's MAXNUMCOLOR early stop is not built"
                         % (data.source, data.largest_graph + 1, data.max_nodes, MAXNUMCOLOR, MAXNUMCOLOR // (H + 1)))
    return H


# ------------------------------------------------------------------------------------------------ colours
def _refine(data, cin, cout, use_edge_labels):
    p = data.plan(use_edge_labels)
    el = data.edge_label if use_edge_labels else None
    N = data.num_nodes
    if not ops.wl_fused_enabled():
        ops.wl_refine_composed(N, None, None, data.slot_node, p.all_ptr, data.nbr_long, el, cin, cout)
        return
    for nodes, group, lds in ((p.small, 8, 0), (p.wave, 64, 0), (p.block, 0, p.block_lds)):
        if nodes.numel():
            ops.wl_refine_fused(N, nodes, group, lds, data.ptr, data.nbr, el, cin, cout)
    if p.huge.numel():
        ops.wl_refine_composed(N, p.huge, p.huge_slots, p.huge_seg, p.huge_ptr, data.nbr_long, el, cin, cout)


def wl_colors(data, num_iterations, use_node_labels=True, use_edge_labels=True):
    """[H + 1, N] int64 (unsigned bit patterns): every node's colour after every iteration.  Row 0 is the node label (1 without node
    labels).  Launches only -- nothing is read back (the node classes were built with the dataset)."""
    H = _check(data, num_iterations, use_node_labels, use_edge_labels)
    c = torch.empty((H + 1, data.num_nodes), dtype=torch.int64, device=data.device)
    if use_node_labels:
        c[0].copy_(data.node_label)
    else:
        c[0].fill_(1)
    for h in range(1, H + 1):
        _refine(data, c[h - 1], c[h], use_edge_labels)
    return c


# ------------------------------------------------------------------------------------------------ features
class WLFeatures:
    """The feature CSR of a dataset: row g = ptr[g] .. ptr[g + 1] holds graph g's distinct colours of all iterations in ascending
    unsigned order (color, int64 bit patterns), how often each occurs (count, int32) and the step whose position slice holds it
    (step, int32).  max_row is the longest row (read back with the number of entries)."""

    def __init__(self, ptr, color, count, step, num_steps, max_row):
        self.ptr, self.color, self.count, self.step, self.num_steps, self.max_row = ptr, color, count, step, num_steps, max_row

    @property
    def num_graphs(self):
        return int(self.ptr.numel() - 1)


def wl_features(data, num_iterations, use_node_labels=True, use_edge_labels=True, colors=None):
    """One-off per dataset, composed from torch device ops: sort all (graph, colour) pairs, count the runs, take each run's first
    iteration, turn them into the colour numbers nums[g][h] and look every sorted position up in them."""
    H = _check(data, num_iterations, use_node_labels, use_edge_labels)
    c = wl_colors(data, H, use_node_labels, use_edge_labels) if colors is None else colors
    return features_of_colors(data.node_graph, c, data.num_graphs)


def features_of_colors(item_graph, c, num_graphs):
    """The feature CSR of coloured items of any kind: item_graph [N] int64 (the graph of every item, ascending), c [S, N] the colour
    of every item after every iteration.  (The items are nodes at k = 1 and node pairs at k = 2: graph_kernels_kwl.py.)"""
    S, N, B, dev = int(c.shape[0]), int(c.shape[1]), int(num_graphs), c.device
    g = item_graph.repeat(S)
    it = torch.arange(S, device=dev).repeat_interleave(N)
    key, o1 = torch.sort(c.reshape(-1) ^ ops._WL_SIGN, stable=True)
    g2, o2 = torch.sort(g[o1], stable=True)                                  # now ordered by (graph, colour)
    key, it = key[o2], it[o1][o2]
    new = torch.ones(S * N, dtype=torch.bool, device=dev)
    new[1:] = (g2[1:] != g2[:-1]) | (key[1:] != key[:-1])
    uid = torch.cumsum(new, 0) - 1
    fg, color = g2[new], (key[new] ^ ops._WL_SIGN).contiguous()
    F = int(fg.numel())
    count = torch.bincount(uid, minlength=F)
    first = torch.full((F,), S, dtype=torch.int64, device=dev).scatter_reduce_(0, uid, it, "amin")
    nums = torch.bincount(fg * S + first, minlength=B * S).view(B, S).cumsum(1)        # distinct colours of graph g up to iteration h
    rows = torch.bincount(fg, minlength=B)
    ptr = torch.cat([rows.new_zeros(1), torch.cumsum(rows, 0)])
    pos = torch.arange(F, device=dev) - ptr[fg]
    step = (nums[fg] <= pos.unsqueeze(1)).sum(1)
    return WLFeatures(ptr.to(torch.int32), color, count.to(torch.int32), step.to(torch.int32), S, int(rows.max()))


# ------------------------------------------------------------------------------------------------ gram matrices
def wl_gram_matrices(data, num_iterations, kernel="WL", use_node_labels=True, use_edge_labels=True, features=None):
    """The H + 1 un-normalised matrices [B, B] (int64), exactly the reference's: matrix h = Phi_h Phi_h^T (WL) or the sums of
    min(Phi_h[i], Phi_h[j]) with matrix 0 all zero (WLOA).  With `features` given this is one launch and reads nothing back."""
    if kernel not in KERNELS:
        raise ValueError("kernel %r is not built here: WL and WLOA at k = 1 are (SP and GR: graph_kernels_spgr; k >= 2 is not)" % (kernel,))
    H = _check(data, num_iterations, use_node_labels, use_edge_labels)
    if H + 1 > ops.wl_max_steps():
        raise ValueError("num_iterations + 1 = %d exceeds the gram kernel's %d steps" % (H + 1, ops.wl_max_steps()))
    f = wl_features(data, H, use_node_labels, use_edge_labels) if features is None else features
    if f.num_steps != H + 1:
        raise ValueError("features were built for %d iterations, not %d" % (f.num_steps - 1, H))
    out = ops.wl_gram(f.ptr, f.color, f.count, f.step, f.num_graphs, f.num_steps, kernel == "WLOA")
    if kernel == "WLOA":
        out[0].zero_()
    return list(out.unbind(0))


def normalize_gram(G):
    """float64 G_ij / (sqrt(G_ii) * sqrt(G_jj)), 0 where that product is 0 -- the reference's expression and order of operations."""
    G = torch.as_tensor(G)
    Gd = G.to(torch.float64)
    d = torch.sqrt(torch.diagonal(Gd))
    x = d.unsqueeze(1) * d.unsqueeze(0)
    return torch.where(x != 0, Gd / torch.where(x != 0, x, torch.ones_like(x)), torch.zeros_like(x))


def write_libsvm(G, classes, path, normalize=True):
    """The reference's text: `class 0:i 1:v 2:v ...` per row at the stream's default precision (%g).  The normalisation runs on
    the host in IEEE double, as the reference's does."""
    G = torch.as_tensor(G).cpu()
    M = (normalize_gram(G) if normalize else G.to(torch.float64)).tolist()
    if len(classes) != len(M):
        raise ValueError("%d classes for a %d x %d matrix" % (len(classes), len(M), len(M)))
    with open(path, "w") as f:
        for i, (cls, row) in enumerate(zip(classes, M), 1):
            f.write("%d 0:%d %s\n" % (int(cls), i, " ".join("%d:%g" % (j, v) for j, v in enumerate(row, 1))))


# ------------------------------------------------------------------------------------------------ command line
def gram_file(gram_dir, dataset, kernel, h):
    """gram.cpp:147 / :171: <gram_dir>/<ds>__WL1_<h>.gram, <gram_dir>/<ds>__WLOA_<h>.gram."""
    return os.path.join(gram_dir, "%s__%s_%d.gram" % (dataset, "WL1" if kernel == "WL" else kernel, h))


def cli_parser(module, description):
    """The arguments of the reference's tool (gram.cpp:38-104), the same for the command line of every graph-kernel module."""
    import argparse
    ap = argparse.ArgumentParser(prog="python -m dummynode4graphlearning_amd." + module, description=description)
    ap.add_argument("--dataset_dir", default="./datasets")
    ap.add_argument("--gram_dir", default="./svm/GM/EXP")
    ap.add_argument("--k", type=int, default=1)
    ap.add_argument("--kernel", default="WL")
    ap.add_argument("--n_iters", type=int, default=1)
    ap.add_argument("--datasets", nargs="*", default=[])
    ap.add_argument("--device", default="cuda")
    return ap


def cli_run(args, grams):
    """What every command line does once it has accepted (--k, --kernel): read all the datasets named (an unknown name: the reference's
    warning, then the read), then per dataset the matrices `grams(name, data, use_node_labels, use_edge_labels)` -- (file, matrix)
    pairs -- written as libsvm text, and the reference's line with the time."""
    jobs = []
    for name in args.datasets:
        if name not in DATASET_FLAGS:
            print("Warning: %s is not a valid dataset." % name)
        jobs.append((name, GraphKernelData.from_dir(args.dataset_dir, name, device=args.device)) + dataset_flags(name))
    for name, data, use_nl, use_el in jobs:
        t0 = time.time()
        for path, G in grams(name, data, use_nl, use_el):
            write_libsvm(G, data.classes, path)
        print("%s-%d\t%s\t%d seconds" % (args.kernel, args.n_iters, name, int(time.time() - t0)))
    return 0


def cli_per_iteration(args, gram_file, matrices):
    """cli_run's `grams` for a kernel with one matrix per iteration: matrices(data, n_iters, kernel, flags) into gram_file(.., h)."""
    return lambda name, data, use_nl, use_el: [
        (gram_file(args.gram_dir, name, args.kernel, h), G)
        for h, G in enumerate(matrices(data, args.n_iters, args.kernel, use_nl, use_el))]


def main(argv=None):
    ap = cli_parser("graph_kernels", "WL / WLOA gram matrices (k = 1) in the reference's libsvm text")
    args = ap.parse_args(argv)
    if args.k != 1 or args.kernel not in KERNELS:
        ap.exit(2, "--k %d --kernel %s is not built here: only --k 1 with --kernel WL or --kernel WLOA is (SP and GR: "
                   "python -m dummynode4graphlearning_amd.graph_kernels_spgr; the k = 2 / k = 3 generators are not)\n" % (args.k, args.kernel))
    return cli_run(args, cli_per_iteration(args, gram_file, wl_gram_matrices))


if __name__ == "__main__":
    sys.exit(main())
