"""HGP-SL (Zhang et al. 2019): the pooling layer with structure learning, its GCN conv and the grouped sparsemax, under the reference's
names (models/hgpsl.py, models/sparse_softmax.py).

HGPSLPool scores every node by ||((I - D^-1/2 A D^-1/2) x)_i||_1, keeps the ceil(ratio n) highest of each graph, and learns a new
weighted structure over every ordered pair of kept nodes of a graph: softmax or sparsemax over a row of
leaky_relu(<x_i, att_l> + <x_j, att_r>) + lamb A_ij.  The reference allocates a dense [N', N'] matrix over the whole pooled batch for
that; here only the diagonal blocks exist, as ragged k x k blocks (ops.hgpsl_structure, dn_hgpsl.hip), and the pooled sizes are
known on the host, so a stack of layers reads back once per batch (the precondition checks) and syncs once per layer (the
data-dependent number of surviving pairs).

Precondition: the (row, col) pairs are unique and no edge joins two graphs (ops.HgpslIndex refuses anything else): the reference's
`adj[r, c] += ...` with a repeated pair is undefined on a GPU.  Ties of the score go to the lower node index; NaN scores are out of
scope.  sample=True (the 3-hop "fast mode") is not implemented: see DESIGN.md "GC: HGP-SL"."""
import torch
import torch.nn as nn
from torch.nn import Parameter

from .. import ops


class Sparsemax(nn.Module):
    """sparsemax over the groups of `batch` (sorted group ids), composed in torch: the public counterpart of what the structure
    kernel fuses.  Per group: the maximum subtracted, the support rho z_(rho) > cumsum_rho - 1 of the descending sort,
    tau = (cumsum_supp - 1) / supp, max(z - tau, 0).  Autograd gives g - mean_support(g) on the support and 0 elsewhere."""

    def forward(self, x, batch):
        if x.numel() == 0:
            return x
        cnt = torch.bincount(batch)
        first = torch.cumsum(cnt, 0) - cnt
        nmax = int(cnt.max())
        pos = torch.arange(x.numel(), device=x.device) - first[batch]
        dense = x.new_full((cnt.numel(), nmax), float("-inf"))
        dense[batch, pos] = x
        z = dense - dense.max(dim=-1, keepdim=True).values
        srt = torch.sort(z, dim=-1, descending=True).values
        cs = torch.where(torch.isfinite(srt), srt, torch.zeros_like(srt)).cumsum(dim=-1) - 1.0
        rho = torch.arange(1, nmax + 1, dtype=x.dtype, device=x.device)
        kk = (torch.isfinite(srt) & (rho * srt > cs)).sum(dim=-1, keepdim=True).clamp(min=1)
        tau = cs.gather(-1, kk - 1) / kk.to(x.dtype)
        return torch.clamp(z - tau, min=0)[batch, pos]


class GCN(nn.Module):
    """The conv of models/hgpsl.py: out = sum_{e: col = i} dinv[row_e] w_e dinv[col_e] (x W)[row_e] + b, the degree taken over the
    edges' rows, no self loops added.  On the GPU: ops.linear_any and ops.neighbor_sum(edge_scale=norm) over an EdgeIndex built from
    the call's edges; elsewhere the same sums in torch ops."""

    def __init__(self, in_channels, out_channels, cached=False, bias=True):
        super().__init__()
        self.in_channels, self.out_channels, self.cached = in_channels, out_channels, cached
        self.cached_result = self.cached_num_edges = None
        self.weight = Parameter(torch.Tensor(in_channels, out_channels))
        nn.init.xavier_uniform_(self.weight.data)
        if bias:
            self.bias = Parameter(torch.Tensor(out_channels))
            nn.init.zeros_(self.bias.data)
        else:
            self.register_parameter("bias", None)
        self.reset_parameters()

    def reset_parameters(self):
        self.cached_result = self.cached_num_edges = None

    @staticmethod
    def norm(edge_index, num_nodes, edge_weight, dtype=None):
        row, col = edge_index[0], edge_index[1]
        if edge_weight is None:
            edge_weight = torch.ones((edge_index.size(1),), dtype=dtype, device=edge_index.device)
        deg = edge_weight.new_zeros(num_nodes).index_add(0, row, edge_weight)
        dinv = deg.pow(-0.5)
        dinv = torch.where(dinv == float("inf"), torch.zeros_like(dinv), dinv)
        return edge_index, dinv[row] * edge_weight * dinv[col]

    def forward(self, x, edge_index, edge_weight=None):
        if self.cached and self.cached_result is not None and edge_index.size(1) != self.cached_num_edges:
            raise RuntimeError("Cached {} number of edges, but found {}".format(self.cached_num_edges, edge_index.size(1)))
        if not self.cached or self.cached_result is None:
            self.cached_num_edges = edge_index.size(1)
            _, norm = self.norm(edge_index, x.size(0), edge_weight, x.dtype)
            index = ops.EdgeIndex(edge_index[0], edge_index[1], x.size(0)) if x.is_cuda else None
            self.cached_result = edge_index, norm, index
        edge_index, norm, index = self.cached_result
        if index is not None:
            out = ops.neighbor_sum(ops.linear_any(x, self.weight.t().contiguous()), index, 0.0, norm.contiguous())
        else:
            h = x @ self.weight
            out = torch.zeros_like(h).index_add(0, edge_index[1], norm.view(-1, 1) * h.index_select(0, edge_index[0]))
        return out if self.bias is None else out + self.bias

    def __repr__(self):
        return "{}({}, {})".format(self.__class__.__name__, self.in_channels, self.out_channels)


class HGPSLPool(nn.Module):
    """forward(x, edge_index, edge_attr, batch=None) -> (x[perm], new edge_index, new edge_attr, batch[perm]) as the reference.
    Keyword-only extras: index = the batch's ops.HgpslIndex when the caller has it (graph.hgpsl_index_of, or the one a previous
    layer returned); return_index=True appends the pooled batch's HgpslIndex to the result, built from host sizes with no read-back,
    so that a stack of layers reads the graph sizes back once."""

    def __init__(self, in_channels, ratio=0.8, sample=False, sparse=False, sl=True, lamb=1.0, negative_slop=0.2):
        super().__init__()
        if sample:
            raise NotImplementedError("HGPSLPool(sample=True): the k-hop sampling mode is not implemented; the ragged blocks already "
                                      "avoid the all-pairs work over the batch that it exists to avoid")
        if isinstance(ratio, bool) or not isinstance(ratio, float) or not 0.0 < ratio <= 1.0:
            raise ValueError("HGPSLPool: ratio must be a float in (0, 1] (got %r)" % (ratio,))
        self.in_channels, self.ratio, self.sample, self.sparse, self.sl = in_channels, ratio, sample, sparse, sl
        self.negative_slop, self.lamb = negative_slop, lamb
        self.att = Parameter(torch.Tensor(1, self.in_channels * 2))
        nn.init.xavier_uniform_(self.att.data)
        self.sparse_attention = Sparsemax()

    def forward(self, x, edge_index, edge_attr, batch=None, *, index=None, return_index=False):
        if index is None:
            index = ops.HgpslIndex.from_batch(edge_index, batch, x.size(0))
        if index.num_nodes != x.size(0) or index.num_edges != edge_index.size(1):
            raise ops._lib.DnHipError("HGPSLPool: the index belongs to another batch (%d nodes, %d edges; got %d, %d)"
                                      % (index.num_nodes, index.num_edges, x.size(0), edge_index.size(1)))
        pooled = index.pooled(self.ratio)
        score = ops.hgpsl_score(x, index, edge_attr)
        sel = ops.hgpsl_topk(score, index, pooled)
        if ops.hgpsl_fused_enabled() and ops.hgpsl_fused_supported(x) and pooled.num_rows:
            xp = ops.gather_rows(x, sel.perm32)
        else:
            xp = x.index_select(0, sel.perm)
        if self.sl is False:
            ei, ea = ops.hgpsl_filter(index, sel, edge_attr)
        else:
            blocks = ops.hgpsl_structure(xp, self.att, edge_attr, index, pooled, sel, self.sparse, self.lamb, self.negative_slop)
            ei, ea = ops.hgpsl_compact(blocks, pooled)
        out = (xp, ei, ea, sel.batch)
        if return_index:
            out += (ops.HgpslIndex(ei[0], ei[1], pooled.graph_ptr, pooled.num_rows, sizes=pooled.ks),)
        return out

    def __repr__(self):
        return "{}({}, ratio={})".format(self.__class__.__name__, self.in_channels, self.ratio)
