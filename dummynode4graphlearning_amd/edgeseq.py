"""EdgeSeq: a batch of edge sequences, the (u, v, ul, el, vl) tuple lists the sequence count models read.

The batched EdgeSeq of the reference's subgraph_isomorphism/dataset.py:111-770 as far as EdgeSeqModel.forward uses it: the five
[B, L] int64 code tensors in `tdata`, left-padded with zeros (pre_pad), `batch_size`, `batch_num_tuples()`, `batch_num_nodes()`,
`number_of_tuples()`, the padded degree tables and `to(device)`.  The lengths live on the HOST (`lens`, a Python list, as the
reference's `_batch_num_tuples`), so a kernel's tile plan never reads the device back.

`EdgeSeq.from_graph(batched_graph)` builds the whole batch from this package's BatchedGraph with torch device ops: per graph the
tuples (id[u], id[v], label[u], elabel, label[v]) sorted by (u, v, ul, el, vl) -- a chain of stable sorts, the graph as the last
key, no Python loop over graphs."""
import torch as th

NODEID, NODELABEL, EDGELABEL = "id", "label", "label"                # constants.py:12-23
REVFLAG, DUMMYFLAG, INDEGREE, OUTDEGREE = "is_reversed", "is_dummy", "in_deg", "out_deg"
CODE_KEYS = ("u", "v", "ul", "el", "vl")


def _pad_left(rows, lens, L, fill=0):
    """Ragged rows (one flat tensor [sum(lens), ...] in batch order) -> [B, L, ...] with every sequence at the END of its row."""
    B = len(lens)
    dev = rows.device
    ln = th.as_tensor(lens, dtype=th.long, device=dev)
    out = th.full((B, L) + tuple(rows.shape[1:]), fill, dtype=rows.dtype, device=dev)
    if rows.shape[0]:
        seq = th.repeat_interleave(th.arange(B, device=dev), ln)
        start = th.cumsum(ln, 0) - ln
        pos = th.arange(rows.shape[0], device=dev) - start[seq] + (L - ln[seq])
        out[seq, pos] = rows
    return out


class EdgeSeq:
    def __init__(self, tdata=None, lens=None):
        """tdata: {"u", "v", "ul", "el", "vl" (, "is_reversed", ...)} as [B, L] tensors (batched, lens = the B lengths) or [n]
        tensors (one sequence, lens None)."""
        if tdata is None:
            tdata = {k: th.zeros((0,), dtype=th.long) for k in CODE_KEYS}
        self.tdata = dict(tdata)
        self.lens = None if lens is None else [int(x) for x in lens]
        self._number_of_tuples = int(self.tdata["u"].shape[0]) if self.lens is None else sum(self.lens)

    # ---- the reference's surface ----
    @property
    def batch_size(self):
        return 1 if self.lens is None else len(self.lens)

    @property
    def device(self):
        return self.tdata["u"].device

    u = src = property(lambda self: self.tdata["u"])
    v = dst = property(lambda self: self.tdata["v"])
    ul = src_label = property(lambda self: self.tdata["ul"])
    el = edge_label = property(lambda self: self.tdata["el"])
    vl = dst_label = property(lambda self: self.tdata["vl"])

    def batch_num_tuples(self):
        return th.tensor([self._number_of_tuples] if self.lens is None else self.lens, device=self.device)

    def number_of_tuples(self):
        return self._number_of_tuples

    def batch_num_nodes(self):
        if self._number_of_tuples == 0:
            return th.zeros((self.batch_size,), dtype=th.long, device=self.device)
        if self.lens is None:
            return th.maximum(self.u.max(), self.v.max()).view(1) + 1
        return th.maximum(self.u.max(dim=1)[0], self.v.max(dim=1)[0]) + 1

    def _degrees(self, of, sized_by):
        """Per sequence bincount(of, minlength = sized_by.max() + 1), left-padded to the widest table (dataset.py:278-326: the
        in-degree table is sized by u, the out-degree table by v -- kept)."""
        if self.lens is None:
            if self._number_of_tuples == 0:
                return th.zeros((0,), dtype=th.long, device=self.device)
            return th.bincount(of, minlength=int(sized_by.max()) + 1)
        B, L = of.shape
        if self._number_of_tuples == 0:
            return th.zeros((B, 0), dtype=th.long, device=self.device)
        dev = self.device
        ln = th.as_tensor(self.lens, dtype=th.long, device=dev)
        live = th.arange(L, device=dev).view(1, L) >= (L - ln).view(B, 1)
        width = th.maximum(sized_by.max(dim=1)[0], th.where(live, of, th.zeros_like(of)).max(dim=1)[0]) + 1      # [B]
        W = int(width.max())
        shift = (W - width).view(B, 1)
        cnt = th.zeros((B, W), dtype=th.long, device=dev)
        cnt.scatter_add_(1, th.where(live, of + shift, th.zeros_like(of)), live.long())
        return cnt

    def in_degrees(self):
        if INDEGREE not in self.tdata:
            self.tdata[INDEGREE] = self._degrees(self.v, self.u)
        return self.tdata[INDEGREE]

    def out_degrees(self):
        if OUTDEGREE not in self.tdata:
            self.tdata[OUTDEGREE] = self._degrees(self.u, self.v)
        return self.tdata[OUTDEGREE]

    def to(self, device):
        if device is None or self.device == th.device(device):
            return self
        return EdgeSeq({k: t.to(device) for k, t in self.tdata.items()}, self.lens)

    def check_codes(self, sizes):
        """Raise unless 0 <= code < size for the five codes (sizes in CODE_KEYS order): the embedding kernels index their tables by
        them.  One read-back per batch and table sizes, kept."""
        done = self.__dict__.setdefault("_checked", set())
        if tuple(sizes) in done or self._number_of_tuples == 0:
            return
        code = th.stack([self.tdata[k].reshape(-1) for k in CODE_KEYS])
        lo, hi = code.min(dim=1)[0].tolist(), code.max(dim=1)[0].tolist()
        for k, a, b, n in zip(CODE_KEYS, lo, hi, sizes):
            if a < 0 or b >= n:
                raise IndexError("EdgeSeq: code %r out of its table [0, %d): min %d, max %d" % (k, n, a, b))
        done.add(tuple(sizes))

    def codes(self):
        """The live tuples of every sequence as one [number_of_tuples, 5] tensor in batch order."""
        code = th.stack([self.tdata[k] for k in CODE_KEYS], dim=-1)
        if self.lens is None:
            return code
        L = code.shape[1]
        ln = th.as_tensor(self.lens, dtype=th.long, device=code.device)
        live = th.arange(L, device=code.device).view(1, L) >= (L - ln).view(-1, 1)
        return code[live]

    def __repr__(self):
        return "EdgeSeq(num_tuples=%d, batch_size=%d, keys=%s)" % (self._number_of_tuples, self.batch_size, list(self.tdata))

    # ---- constructors ----
    @staticmethod
    def batch(data, pre_pad=True):
        """dataset.py:634-709: sequences ([n, 5] codes, or EdgeSeq objects, single or batched) -> one padded batch.  Extra tdata keys
        (REVFLAG) are carried and padded with zeros like the codes; the degree tables are not."""
        assert isinstance(data, list) and len(data) > 0
        seqs = []
        for x in data:
            if not isinstance(x, EdgeSeq):
                code = th.as_tensor(x)
                x = EdgeSeq({k: code[..., i] for i, k in enumerate(CODE_KEYS)})
            seqs.append(x)
        keys = list(CODE_KEYS)
        for x in seqs:
            keys += [k for k in x.tdata if k not in keys and k not in (INDEGREE, OUTDEGREE)]
        lens, rows = [], {k: [] for k in keys}
        for x in seqs:
            one = [(None, x._number_of_tuples)] if x.lens is None else list(enumerate(x.lens))
            for i, n in one:
                lens.append(n)
                for k in keys:
                    if k in x.tdata:
                        t = x.tdata[k] if i is None else x.tdata[k][i, x.tdata[k].shape[1] - n:]
                    else:
                        t = th.zeros((n,), dtype=next(y.tdata[k].dtype for y in seqs if k in y.tdata), device=x.device)
                    rows[k].append(t)
        L = max(lens)
        out = {}
        for k in keys:
            padded = _pad_left(th.cat(rows[k]), lens, L)
            out[k] = padded if pre_pad else th.stack([th.roll(padded[i], lens[i] - L, 0) for i in range(len(lens))])
        return EdgeSeq(out, lens)

    @staticmethod
    def from_graph(graph):
        """dataset.py:507-541 for a BatchedGraph, the whole batch at once (see the module docstring)."""
        src, dst = graph.all_edges()
        src, dst = src.long(), dst.long()
        dev = src.device
        ids, labels, elabels = graph.ndata[NODEID].long(), graph.ndata[NODELABEL].long(), graph.edata[EDGELABEL].long()
        bne = graph.batch_num_edges().long()
        B = int(bne.numel())
        gid = th.repeat_interleave(th.arange(B, device=dev), bne)
        cols = [ids[src], ids[dst], labels[src], elabels, labels[dst]]
        order = th.arange(src.numel(), device=dev)
        for key in reversed([gid] + cols):                            # least significant key first, every sort stable
            order = order[th.argsort(key[order], stable=True)]
        tdata = {k: c[order] for k, c in zip(CODE_KEYS, cols)}
        if REVFLAG in graph.edata:
            tdata[REVFLAG] = graph.edata[REVFLAG][order]
        lens = bne.cpu().tolist()                                      # (one read of B integers: the lengths are host data from here on)
        L = max(lens) if lens else 0
        return EdgeSeq({k: _pad_left(t, lens, L) for k, t in tdata.items()}, lens)
