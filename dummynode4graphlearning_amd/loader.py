"""A device-resident dataset and one-launch mini-batch assembly.

The reference builds every step's batch on the host: ``DataLoader`` + PyG collate
(graph_classification/graph_neural_networks/main.py:245-247), ``batchify`` -> ``dgl.batch``
(subgraph_isomorphism/dataset.py:1321-1328, 1605-1611).  Here the whole dataset is packed once on the device
(``PackedGraphs``: columns of node / edge / graph level, graph-local endpoints, ``node_ptr`` / ``edge_ptr``), a batch is planned on
the host from the host copy of the sizes (``np.cumsum``: no read-back), and one ``dn_batch_assemble`` launch copies the chosen
graphs' rows, re-bases their endpoints and fills the ``batch`` vector.  ``BatchLoader`` is the ``DataLoader`` look-alike on top.

The result of ``assemble(ids)`` equals ``GraphBatch.collate([items[i] for i in ids])`` / ``BatchedGraph.batch([graphs[i] for i
in ids])`` tensor for tensor, with ``ptr`` / ``node_ptr`` / ``edge_ptr`` preset.
"""
import numpy as np
import torch

from . import ops
from ._lib import BatchCol, check, lib, require_gpu, stream_ptr
from .graph import BatchedGraph, GraphBatch

LEVEL_NODE, LEVEL_EDGE, LEVEL_GRAPH = 0, 1, 2             # DN_BATCH_LEVEL_*
REBASE_NONE, REBASE_NODE, REBASE_EDGE = 0, 1, 2           # DN_BATCH_REBASE_*
MAX_COLS = 32                                             # DN_BATCH_MAX_COLS
_LIMIT = 1 << 31                                          # ids and offsets are int32 on the device
I32 = torch.int32


def check_totals(node_sizes, edge_sizes):
    """ValueError when the nodes or the edges of the given graphs do not fit int32 offsets (sums only: nothing is allocated)."""
    n, e = int(np.sum(node_sizes, dtype=np.int64)), int(np.sum(edge_sizes, dtype=np.int64))
    if n >= _LIMIT or e >= _LIMIT:
        raise ValueError("%d nodes / %d edges: totals must stay below 2^31 (int32 offsets on the device)" % (n, e))
    return n, e


def plan_batch(node_sizes, edge_sizes, ids):
    """Host plan of a batch: (ids, out_node_ptr, out_edge_ptr) as int64 numpy arrays ([B], [B + 1], [B + 1]).
    Empty ids -> ValueError, an id outside [0, len(node_sizes)) -> IndexError, totals of 2^31 or more -> ValueError."""
    if isinstance(ids, torch.Tensor):
        ids = ids.detach().cpu().numpy()
    ids = np.asarray(ids).reshape(-1)
    if ids.size == 0:
        raise ValueError("assemble needs at least one graph id")
    if ids.dtype.kind not in "iu":
        raise TypeError("graph ids must be integers, got %s" % ids.dtype)
    ids = ids.astype(np.int64, copy=False)
    G = len(node_sizes)
    if int(ids.min()) < 0 or int(ids.max()) >= G:
        raise IndexError("graph id out of range [0, %d): min %d, max %d" % (G, int(ids.min()), int(ids.max())))
    nn, ne = node_sizes[ids], edge_sizes[ids]
    check_totals(nn, ne)
    onp, oep = np.zeros(ids.size + 1, dtype=np.int64), np.zeros(ids.size + 1, dtype=np.int64)
    np.cumsum(nn, out=onp[1:])
    np.cumsum(ne, out=oep[1:])
    return ids, onp, oep


class _Col:
    """One packed column: rows of graph i = data[ptr[i]:ptr[i + 1]] along dim 0 (ptr by `level`)."""

    def __init__(self, name, data, level, rebase=REBASE_NONE, src_global=False, ptr_tail=False, src_ptr=None, flat=False):
        if src_ptr is None and not data.is_contiguous():
            data = data.contiguous()
        self.name, self.data, self.level, self.rebase, self.flat = name, data, level, rebase, flat
        self.src_global, self.ptr_tail = bool(src_global), bool(ptr_tail)
        self.dtype, self.tail_shape = data.dtype, tuple(data.shape[1:]) if src_ptr is None else ()
        per = 1
        for s in self.tail_shape:
            per *= int(s)
        self.per = per
        self.row_bytes = per * data.element_size()
        self.int_width = data.element_size() if rebase != REBASE_NONE else 0
        self.src_ptr = int(data.data_ptr()) if src_ptr is None else int(src_ptr)
        if self.row_bytes < 1:
            raise ValueError("column %s has empty rows (shape %s)" % (name, tuple(data.shape)))

    def rows(self, N, E, B):
        return N if self.level == LEVEL_NODE else (E if self.level == LEVEL_EDGE else B)

    def alloc(self, N, E, B):
        r = self.rows(N, E, B) + (1 if self.ptr_tail else 0)
        if self.flat:
            return torch.empty(r * self.per, dtype=self.dtype, device=self.data.device)
        return torch.empty((r,) + self.tail_shape, dtype=self.dtype, device=self.data.device)


def _template(cols):
    if len(cols) > MAX_COLS:
        raise ValueError("%d columns: dn_batch_assemble takes at most %d" % (len(cols), MAX_COLS))
    arr = (BatchCol * max(len(cols), 1))()
    for j, c in enumerate(cols):
        arr[j].src, arr[j].dst = c.src_ptr or None, None
        arr[j].row_bytes, arr[j].level, arr[j].rebase, arr[j].int_width = c.row_bytes, c.level, c.rebase, c.int_width
        arr[j].src_global, arr[j].ptr_tail = int(c.src_global), int(c.ptr_tail)
    return arr


_INDEX_NAMES = ("in_ptr", "in_perm", "src_by_dst", "out_ptr", "out_perm", "dst_by_src")


class PackedGraphs:
    """A whole dataset on the device, packed once; ``assemble(ids)`` builds a mini-batch of it in one launch.

    kind "gc": the batch is a GraphBatch (x, edge_index, edge_attr, y, is_dummy_node, is_dummy_edge);
    kind "si": a BatchedGraph (src, dst, ndata, edata).  node_sizes / edge_sizes (numpy, host) plan every batch without a read-back;
    node_ptr / edge_ptr are their int32 prefix sums on the device.
    with_index: whether assemble also emits the batch's CSR by destination / CSC by source (ops.EdgeIndex) from the dataset's own
    (build_edge_index) as six more columns of the same launch.  Off by default: see docs/LAB_NOTES.md, "Batch loader"."""

    with_index = False

    def __init__(self, kind, node_sizes, edge_sizes, cols, device, keys=None):
        assert kind in ("gc", "si")
        self.kind, self.device = kind, torch.device(device)
        self.node_sizes = np.ascontiguousarray(node_sizes, dtype=np.int64).reshape(-1)
        self.edge_sizes = np.ascontiguousarray(edge_sizes, dtype=np.int64).reshape(-1)
        assert self.node_sizes.size == self.edge_sizes.size
        self.num_nodes, self.num_edges = check_totals(self.node_sizes, self.edge_sizes)
        self.node_ptr_host = np.concatenate([[0], np.cumsum(self.node_sizes)]).astype(np.int64)
        self.edge_ptr_host = np.concatenate([[0], np.cumsum(self.edge_sizes)]).astype(np.int64)
        self.node_ptr = torch.from_numpy(self.node_ptr_host.astype(np.int32)).to(self.device)
        self.edge_ptr = torch.from_numpy(self.edge_ptr_host.astype(np.int32)).to(self.device)
        self._cols = list(cols)
        self._keys = keys                                   # si: (ndata keys, edata keys) in dict order
        for c in self._cols:
            want = {LEVEL_NODE: self.num_nodes, LEVEL_EDGE: self.num_edges, LEVEL_GRAPH: len(self)}[c.level]
            have = c.data.shape[1] if c.name in ("src", "dst") and kind == "gc" else c.data.shape[0]
            if have != want:
                raise ValueError("column %s has %d rows, the sizes add up to %d" % (c.name, have, want))
        self._tmpl = _template(self._cols)
        self._index_cols, self._tmpl_index = None, None

    def __len__(self):
        return int(self.node_sizes.size)

    # ---- constructors -------------------------------------------------------------------------------------------------------
    @classmethod
    def _gc(cls, x, edge_index, edge_attr, y, is_dummy_node, is_dummy_edge, node_sizes, edge_sizes):
        if x is None or edge_index is None:
            raise ValueError("a graph-classification dataset needs x and edge_index")
        G = len(node_sizes)
        edge_index = edge_index.contiguous()
        if edge_index.dtype != torch.int64:
            raise ValueError("edge_index must be int64 (got %s)" % edge_index.dtype)
        E = int(edge_index.shape[1])
        cols = [_Col("x", x, LEVEL_NODE),
                _Col("src", edge_index, LEVEL_EDGE, REBASE_NODE, src_ptr=edge_index.data_ptr()),
                _Col("dst", edge_index, LEVEL_EDGE, REBASE_NODE, src_ptr=edge_index.data_ptr() + 8 * E)]
        if edge_attr is not None:
            cols.append(_Col("edge_attr", edge_attr, LEVEL_EDGE))
        if y is not None:
            if y.shape[0] != G:
                raise ValueError("y has %d rows for %d graphs" % (y.shape[0], G))
            cols.append(_Col("y", y.reshape(G, -1), LEVEL_GRAPH, flat=True))
        if is_dummy_node is not None:
            cols.append(_Col("is_dummy_node", is_dummy_node, LEVEL_NODE))
        if is_dummy_edge is not None:
            cols.append(_Col("is_dummy_edge", is_dummy_edge, LEVEL_EDGE))
        return cls("gc", node_sizes, edge_sizes, cols, x.device)

    @classmethod
    def from_pyg_dataset(cls, ds):
        """Zero-copy over a tu_io.PYGDataset's collated tensors (ds.data / ds.slices); assemble(ids) == ds.batch(ids)."""
        d, s = ds.data, ds.slices
        if d.x is None or "x" not in s:
            raise ValueError("the dataset has no node features")
        nptr, eptr = s["x"].detach().cpu().numpy().astype(np.int64), s["edge_index"].detach().cpu().numpy().astype(np.int64)
        return cls._gc(d.x, d.edge_index, d.edge_attr, d.y, getattr(d, "is_dummy_node", None), getattr(d, "is_dummy_edge", None),
                       np.diff(nptr), np.diff(eptr))

    @classmethod
    def from_items(cls, items):
        """From per-graph items (x, edge_index, edge_attr, y, is_dummy_node, is_dummy_edge namespaces, graph-local endpoints):
        assemble(ids) == GraphBatch.collate([items[i] for i in ids]).  An optional field is given by every item or by none; y has the
        same number of elements in every item."""
        items = list(items)
        if not items:
            raise ValueError("no graphs")

        def field(name, dim=0, prep=None):
            vals = [getattr(d, name, None) for d in items]
            if all(v is None for v in vals):
                return None
            if any(v is None for v in vals):
                raise ValueError("%s is given by some graphs only" % name)
            return torch.cat([prep(v) if prep else v for v in vals], dim)

        y = field("y", prep=lambda v: v.reshape(1, -1))
        return cls._gc(field("x"), field("edge_index", 1), field("edge_attr"), y, field("is_dummy_node"), field("is_dummy_edge"),
                       np.array([int(d.x.shape[0]) for d in items], dtype=np.int64),
                       np.array([int(d.edge_index.shape[1]) for d in items], dtype=np.int64))

    @classmethod
    def from_graphs(cls, graphs):
        """From single-graph BatchedGraph objects with their ndata / edata: assemble(ids) == BatchedGraph.batch([graphs[i] ...])."""
        graphs = list(graphs)
        if not graphs:
            raise ValueError("no graphs")
        if any(g.batch_size != 1 for g in graphs):
            raise ValueError("from_graphs takes single graphs (batch_size 1)")
        nkeys, ekeys = list(graphs[0].ndata), list(graphs[0].edata)
        cols = [_Col("src", torch.cat([g._src.long() for g in graphs]), LEVEL_EDGE, REBASE_NODE),
                _Col("dst", torch.cat([g._dst.long() for g in graphs]), LEVEL_EDGE, REBASE_NODE)]
        cols += [_Col("ndata:" + k, torch.cat([g.ndata[k] for g in graphs], 0), LEVEL_NODE) for k in nkeys]
        cols += [_Col("edata:" + k, torch.cat([g.edata[k] for g in graphs], 0), LEVEL_EDGE) for k in ekeys]
        return cls("si", np.array([g.number_of_nodes() for g in graphs], dtype=np.int64),
                   np.array([g.number_of_edges() for g in graphs], dtype=np.int64), cols, graphs[0].device, keys=(nkeys, ekeys))

    # ---- the dataset's own CSR / CSC ------------------------------------------------------------------------------------------
    def _col(self, name):
        for c in self._cols:
            if c.name == name:
                return c
        raise KeyError(name)

    def build_edge_index(self):
        """ops.csr_build once over the whole packed dataset, both directions.  Nodes of a graph are contiguous, so a batch's CSR is the
        concatenation of its graphs' CSRs re-based: assemble(with_index=True) copies it instead of grouping the batch's edges again."""
        if self._index_cols is not None:
            return self
        src_c, dst_c = self._col("src"), self._col("dst")
        E = self.num_edges
        if self.kind == "gc":
            src_l, dst_l = src_c.data[0], src_c.data[1]
        else:
            src_l, dst_l = src_c.data, dst_c.data
        G = len(self)
        gid = torch.repeat_interleave(torch.arange(G, device=self.device), torch.from_numpy(self.edge_sizes).to(self.device),
                                      output_size=E)
        off = self.node_ptr.long()[gid]
        src = (src_l + off).to(I32).contiguous()
        dst = (dst_l + off).to(I32).contiguous()
        in_ptr, in_perm = ops.csr_build(dst, self.num_nodes)
        out_ptr, out_perm = ops.csr_build(src, self.num_nodes)
        src_by_dst, dst_by_src = ops.gather_rows_i32(src, in_perm), ops.gather_rows_i32(dst, out_perm)
        # (pointer columns: one value per NODE, re-based by the EDGE offset; the dataset's closing entry is not a row of any graph)
        self._index_cols = [
            _Col("in_ptr", in_ptr[:-1].contiguous(), LEVEL_NODE, REBASE_EDGE, src_global=True, ptr_tail=True),
            _Col("in_perm", in_perm, LEVEL_EDGE, REBASE_EDGE, src_global=True),
            _Col("src_by_dst", src_by_dst, LEVEL_EDGE, REBASE_NODE, src_global=True),
            _Col("out_ptr", out_ptr[:-1].contiguous(), LEVEL_NODE, REBASE_EDGE, src_global=True, ptr_tail=True),
            _Col("out_perm", out_perm, LEVEL_EDGE, REBASE_EDGE, src_global=True),
            _Col("dst_by_src", dst_by_src, LEVEL_EDGE, REBASE_NODE, src_global=True)]
        self._tmpl_index = _template(self._cols + self._index_cols)
        return self

    # ---- one batch ----------------------------------------------------------------------------------------------------------
    def _stage(self, ids, onp, oep):
        """The id / pointer table (int32: ids, out_node_ptr, out_edge_ptr) and the batch's int64 host-known vectors behind it (gc: ptr;
        si: batch_num_nodes, batch_num_edges) in ONE pinned buffer, copied to the device once."""
        B = ids.size
        n32 = 3 * B + 2
        w32 = n32 + (n32 & 1)
        n64 = B + 1 if self.kind == "gc" else 2 * B
        buf = torch.empty(4 * w32 + 8 * n64, dtype=torch.uint8, pin_memory=self.device.type == "cuda")
        host = buf.numpy()
        t32, t64 = host[:4 * n32].view(np.int32), host[4 * w32:].view(np.int64)
        t32[:B], t32[B:2 * B + 1], t32[2 * B + 1:] = ids, onp, oep
        if self.kind == "gc":
            t64[:] = onp
        else:
            t64[:B], t64[B:] = self.node_sizes[ids], self.edge_sizes[ids]
        dev = buf.to(self.device, non_blocking=True)
        return dev[:4 * n32].view(I32), dev[4 * w32:].view(torch.int64)

    def assemble(self, ids, with_index=None):
        """The batch of the graphs `ids` (host integers: list, numpy or CPU tensor; any order, duplicates allowed): a GraphBatch
        (kind "gc") or a BatchedGraph ("si") equal to what the host-side collate returns.  One pinned host -> device copy, one launch,
        no device -> host read (with_index=True hands the CSR parts to ops.EdgeIndex.from_parts, whose hub split reads one scalar)."""
        ids, onp, oep = plan_batch(self.node_sizes, self.edge_sizes, ids)
        with_index = self.with_index if with_index is None else bool(with_index)
        B, N, E = int(ids.size), int(onp[-1]), int(oep[-1])
        if with_index:
            self.build_edge_index()
        cols = self._cols + (self._index_cols if with_index else [])
        tmpl = self._tmpl_index if with_index else self._tmpl
        require_gpu(self.node_ptr)
        table, extra = self._stage(ids, onp, oep)
        out, arr = {}, type(tmpl).from_buffer_copy(tmpl)
        ei = torch.empty((2, E), dtype=torch.int64, device=self.device) if self.kind == "gc" else None
        for j, c in enumerate(cols):
            if ei is not None and c.name in ("src", "dst"):
                arr[j].dst = (ei.data_ptr() + (8 * E if c.name == "dst" else 0)) or None
                continue
            t = out[c.name] = c.alloc(N, E, B)
            arr[j].dst = t.data_ptr() or None
        bvec = torch.empty(N, dtype=torch.int64, device=self.device) if self.kind == "gc" else None

        def _launch():
            check(lib().dn_batch_assemble(B, table.data_ptr(), self.node_ptr.data_ptr(), self.edge_ptr.data_ptr(), len(self), N, E, arr,
                                          len(cols), None if bvec is None or N == 0 else bvec.data_ptr(), stream_ptr()),
                  "dn_batch_assemble")

        ops.launch_tagged("batch_assemble", _launch)
        node_ptr, edge_ptr = table[B:2 * B + 1], table[2 * B + 1:]
        if self.kind == "gc":
            batch = GraphBatch(out["x"], ei, bvec, out.get("edge_attr"), out.get("y"), out.get("is_dummy_node"),
                               out.get("is_dummy_edge"), ptr=extra)
            batch._dn_ptr_i32 = (extra, extra._version, node_ptr)       # graph.graph_ptr_i32's per-batch conversion, already made
            src, dst = ei[0], ei[1]
        else:
            nkeys, ekeys = self._keys
            batch = BatchedGraph(out["src"], out["dst"], N, extra[:B], extra[B:], {k: out["ndata:" + k] for k in nkeys},
                                 {k: out["edata:" + k] for k in ekeys}, node_ptr=node_ptr, edge_ptr=edge_ptr)
            src, dst = out["src"], out["dst"]
        if with_index:
            batch._cache._edge_index = ops.EdgeIndex.from_parts(src, dst, N, node_ptr, *(out[k] for k in _INDEX_NAMES))
        return batch


class BatchLoader:
    """Re-iterable mini-batch loader over a PackedGraphs (the DataLoader of main.py:245-247 / dataset.py:1605-1611 without worker
    processes: a batch costs one launch).  With shuffle, an epoch's order is torch.randperm(len(dataset), generator=generator) on the
    CPU, drawn anew at every iteration.  batch_sampler: any iterable of index lists (the reference's bucket / curriculum samplers),
    used in place of batch_size / shuffle / drop_last.  fetch(ids) -> batch defaults to dataset.assemble; a loop over several packed
    datasets passes its own, e.g. ``lambda ids: (patterns.assemble(pid[ids]), graphs.assemble(ids), counts[ids])``."""

    def __init__(self, dataset, batch_size=1, shuffle=False, drop_last=False, generator=None, batch_sampler=None, fetch=None):
        if batch_sampler is not None:
            if batch_size != 1 or shuffle or drop_last:
                raise ValueError("batch_sampler excludes batch_size, shuffle and drop_last")
        elif int(batch_size) < 1:
            raise ValueError("batch_size must be positive, got %r" % (batch_size,))
        self.dataset, self.batch_size, self.shuffle, self.drop_last = dataset, int(batch_size), bool(shuffle), bool(drop_last)
        self.generator, self.batch_sampler = generator, batch_sampler
        self.fetch = fetch if fetch is not None else dataset.assemble

    def __len__(self):
        if self.batch_sampler is not None:
            return len(self.batch_sampler)
        n = len(self.dataset)
        return n // self.batch_size if self.drop_last else (n + self.batch_size - 1) // self.batch_size

    def batches(self):
        """The index lists of one epoch (draws the epoch's permutation when shuffling)."""
        if self.batch_sampler is not None:
            yield from self.batch_sampler
            return
        n = len(self.dataset)
        order = torch.randperm(n, generator=self.generator) if self.shuffle else torch.arange(n)
        stop = n - n % self.batch_size if self.drop_last else n
        for a in range(0, stop, self.batch_size):
            yield order[a:min(a + self.batch_size, stop)]

    def __iter__(self):
        for ids in self.batches():
            yield self.fetch(ids)
