"""The DiffPool graph classifier with the reference's constructor (``DiffPool(args)``), attribute and state_dict names and
``forward(data) -> log-probs`` surface, its first level on the batch's ragged rows.

reference: graph_classification/graph_neural_networks/models/diffpool.py (adapted there from gnn-comparison), on top of
torch_geometric's DenseSAGEConv / dense_diff_pool / to_dense_batch / to_dense_adj, restated here from their published definitions.

The reference pads the batch to [B, Nmax, F] and a dense [B, Nmax, Nmax] adjacency.  Here level 0 works on the rows [N, .]:

* aggregation is over OUT-edges: to_dense_adj puts edge (src, dst) at adj[src, dst] (duplicates summed, self loops kept) and
  DenseSAGEConv forms (adj @ x) / adj.sum(-1).clamp(min=1) -- row i receives the rows of the destinations of its out-edges, divided by
  max(out-degree, 1); the transpose of the sparse SAGEConv of conv.py.
* BatchNorm sees the padding: the reference flattens to [B Nmax, C], so B Nmax - N zero rows count in the batch statistics (and in
  the n / (n - 1) of the running variance).  batch_norm_counted reproduces that from the real rows and the row count.
* pooling: S = softmax(s) over the clusters, per graph X' = S^T Z and A' = S^T (A S): ops.diffpool_assign.
* levels >= 1 and final_embed are dense and uniform ([B, C, F], [B, C, C], no mask): torch.bmm plus the Linear / BatchNorm kernels.
* the two auxiliary losses are returned by DiffPoolLayer (closed forms on the ragged rows) but DiffPool.forward drops them, as the
  reference does (diffpool.py:160-162), so the model switches their computation off.
"""
import json
from math import ceil

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops
from ..graph import diffpool_index_of
from .conv import HipLinear
from .models import HipBatchNorm1d, hip_batch_norm_forward

NUM_SAGE_LAYERS = 3
EPS = 1e-15


def _linear(lin, x):
    """lin on the last axis; a [B, n, F] input goes through the HIP Linear as [B n, F] rows."""
    if x.dim() == 2:
        return lin(x)
    return lin(x.reshape(-1, x.shape[-1])).view(*x.shape[:-1], -1)


def mean_aggregate(x, adj):
    """(adj @ x) / adj.sum(-1).clamp(min=1): adj a dense [B, n, n] adjacency with x [B, n, F], or the batch's ops.DiffPoolIndex with
    the ragged rows x [N, F]."""
    if isinstance(adj, ops.DiffPoolIndex):
        if x.is_cuda and adj.edge is not None:
            total = ops.neighbor_sum(x, adj.edge_t)
        else:
            total = torch.zeros_like(x).index_add(0, adj.src, x.index_select(0, adj.dst))
        return total * adj.inv_out_deg(x.dtype)
    return torch.bmm(adj, x) / adj.sum(dim=-1, keepdim=True).clamp(min=1)


class DenseSAGEConv(nn.Module):
    """torch_geometric.nn.DenseSAGEConv (2.0.2): lin_rel(mean over the adjacency row) + lin_root(x); lin_rel without bias."""

    def __init__(self, in_channels, out_channels, normalize=False, bias=True):
        super().__init__()
        self.in_channels, self.out_channels, self.normalize = in_channels, out_channels, normalize
        self.lin_rel = HipLinear(in_channels, out_channels, bias=False)
        self.lin_root = HipLinear(in_channels, out_channels, bias=bias)

    def reset_parameters(self):
        self.lin_rel.reset_parameters()
        self.lin_root.reset_parameters()

    def forward(self, x, adj, mask=None, add_loop=False, agg=None):
        """agg: mean_aggregate(x, adj) when the caller already has it (the two conv1 of a DiffPool level share it)."""
        if not isinstance(adj, ops.DiffPoolIndex):
            x = x.unsqueeze(0) if x.dim() == 2 else x
            adj = adj.unsqueeze(0) if adj.dim() == 2 else adj
        if agg is None:
            agg = mean_aggregate(x, adj)
        out = _linear(self.lin_rel, agg) + _linear(self.lin_root, x)
        if self.normalize:
            out = F.normalize(out, p=2.0, dim=-1)
        if mask is not None:
            out = out * mask.view(out.shape[0], out.shape[1], 1).to(x.dtype)
        return out


def batch_norm_counted(mod, x, pad_rows):
    """BatchNorm1d `mod` over the rows x [rows, C] AND pad_rows further rows of zeros that are not stored: training-mode statistics
    over n = rows + pad_rows (mean = sum / n, biased variance, the running variance scaled by n / (n - 1)), running buffers and
    num_batches_tracked updated as torch does.  No padding, or eval mode: the module's own forward."""
    pad_rows = int(pad_rows)
    if pad_rows == 0 or not (mod.training or not mod.track_running_stats):
        return hip_batch_norm_forward(mod, x, False)
    n = x.shape[0] + pad_rows
    mean = x.sum(0) / n
    d = x - mean
    var = ((d * d).sum(0) + pad_rows * (mean * mean)) / n                       # the zero rows lie at -mean
    y = d * torch.rsqrt(var + mod.eps)
    if mod.affine:
        y = y * mod.weight + mod.bias
    if mod.training and mod.track_running_stats:
        with torch.no_grad():
            mod.num_batches_tracked += 1
            mom = mod.momentum if mod.momentum is not None else 1.0 / float(mod.num_batches_tracked)
            mod.running_mean.mul_(1.0 - mom).add_(mean.detach().to(mod.running_mean.dtype), alpha=mom)
            mod.running_var.mul_(1.0 - mom).add_((var.detach() * (n / max(n - 1, 1))).to(mod.running_var.dtype), alpha=mom)
    return y


class SAGEConvolutions(nn.Module):
    """diffpool.py:15-58: three DenseSAGEConv with a BatchNorm behind each of the first two, their outputs concatenated (and a Linear
    over the concatenation for the pooling branch)."""

    def __init__(self, in_channels, hidden_channels, out_channels, normalize=False, lin=True):
        super().__init__()
        self.conv1 = DenseSAGEConv(in_channels, hidden_channels)
        self.bn1 = HipBatchNorm1d(hidden_channels)
        self.conv2 = DenseSAGEConv(hidden_channels, hidden_channels)
        self.bn2 = HipBatchNorm1d(hidden_channels)
        self.conv3 = DenseSAGEConv(hidden_channels, out_channels)
        if lin is True:
            self.lin = HipLinear((NUM_SAGE_LAYERS - 1) * hidden_channels + out_channels, out_channels)
        else:
            self.lin = None

    def bn(self, i, x, pad_rows=0):
        mod = getattr(self, "bn{}".format(i))
        if x.dim() == 2:
            return batch_norm_counted(mod, x, pad_rows)
        return batch_norm_counted(mod, x.reshape(-1, x.shape[-1]), pad_rows).view(x.shape)

    def forward(self, x, adj, mask=None, agg=None):
        """x [B, n, F] with a dense adj [B, n, n] (mask as in the reference), or the ragged rows x [N, F] with the batch's
        ops.DiffPoolIndex: the B Nmax - N rows of padding the reference would carry are counted by the BatchNorms."""
        pad = adj.padded_rows - x.shape[0] if isinstance(adj, ops.DiffPoolIndex) else 0
        x1 = self.bn(1, F.relu(self.conv1(x, adj, mask, add_loop=False, agg=agg)), pad)
        x2 = self.bn(2, F.relu(self.conv2(x1, adj, mask, add_loop=False)), pad)
        x3 = self.conv3(x2, adj, mask, add_loop=False)
        x = torch.cat([x1, x2, x3], dim=-1)
        if self.lin is not None:
            x = _linear(self.lin, x)
        return x


def dense_diff_pool(x, adj, s, mask=None, with_losses=True):
    """torch_geometric.nn.dense_diff_pool on padded tensors: (S^T X, S^T A S, link loss, entropy loss), S = softmax(s, -1).
    with_losses=False: the two losses are zeros and nothing is spent on them."""
    x = x.unsqueeze(0) if x.dim() == 2 else x
    adj = adj.unsqueeze(0) if adj.dim() == 2 else adj
    s = s.unsqueeze(0) if s.dim() == 2 else s
    batch_size, num_nodes, _ = x.size()
    s = torch.softmax(s, dim=-1)
    if mask is not None:
        mask = mask.view(batch_size, num_nodes, 1).to(x.dtype)
        x, s = x * mask, s * mask
    st = s.transpose(1, 2)
    out = torch.bmm(st, x)
    out_adj = torch.bmm(torch.bmm(st, adj), s)
    if not with_losses:
        zero = out.new_zeros(())
        return out, out_adj, zero, zero
    link_loss = torch.norm(adj - torch.bmm(s, st), p=2) / adj.numel()
    ent_loss = (-s * torch.log(s + EPS)).sum(dim=-1).mean()
    return out, out_adj, link_loss, ent_loss


def ragged_diff_pool(z, index, s, with_losses=True):
    """dense_diff_pool of the padded batch from its ragged rows: z [N, F], s [N, C] and the batch's ops.DiffPoolIndex.  The losses in
    closed form: ||A - S S^T||_F^2 = ||A||_F^2 - 2 tr(S^T A S) + ||S^T S||_F^2 over B Nmax^2 entries; the entropy over B Nmax rows."""
    out, out_adj = ops.diffpool_assign(s, z, index)
    if not with_losses:
        zero = out.new_zeros(())
        return out, out_adj, zero, zero
    S = torch.softmax(s, dim=-1)
    gram = ops.segment_gram(S, S, index.graph_ptr, None if not S.is_cuda else index.tiles)
    sq = index.adj_sq_norm().to(S.dtype) - 2.0 * torch.diagonal(out_adj, dim1=1, dim2=2).sum() + (gram * gram).sum()
    link_loss = torch.sqrt(sq.clamp(min=0)) / max(index.num_graphs * index.max_nodes ** 2, 1)
    ent_loss = (-S * torch.log(S + EPS)).sum() / max(index.padded_rows, 1)
    return out, out_adj, link_loss, ent_loss


class DiffPoolLayer(nn.Module):
    """diffpool.py:60-80: GraphSAGE convolutions for the assignment and for the embedding, then the pooling.  Returns
    (x [B, C, F], adj [B, C, C], link loss, entropy loss); with compute_losses = False (what DiffPool sets, which drops them) the two
    losses are zeros and nothing is spent on them."""

    def __init__(self, dim_input, dim_hidden, dim_embedding, no_new_clusters):
        super().__init__()
        self.gnn_pool = SAGEConvolutions(dim_input, dim_hidden, no_new_clusters)
        self.gnn_embed = SAGEConvolutions(dim_input, dim_hidden, dim_embedding, lin=False)
        self.compute_losses = True

    def forward(self, x, adj, mask=None):
        """x [B, n, F], adj [B, n, n] (+ mask), or the ragged rows x [N, F] with adj = the batch's ops.DiffPoolIndex."""
        ragged = isinstance(adj, ops.DiffPoolIndex)
        if not ragged:
            x = x.unsqueeze(0) if x.dim() == 2 else x
            adj = adj.unsqueeze(0) if adj.dim() == 2 else adj
        agg = mean_aggregate(x, adj)                                           # the two conv1 see the same input and adjacency
        s = self.gnn_pool(x, adj, mask, agg=agg)
        x = self.gnn_embed(x, adj, mask, agg=agg)
        if ragged:
            return ragged_diff_pool(x, adj, s, self.compute_losses)
        return dense_diff_pool(x, adj, s, mask, self.compute_losses)


DEFAULT_CONFIG = {"num_layers": 2, "gnn_dim_hidden": 64, "dim_embedding": 128, "dim_embedding_MLP": 50}


class DiffPool(nn.Module):
    """diffpool.py:82-162.  args.additional: a JSON string (as the reference's json.loads expects) or the dict itself; empty: the
    reference's defaults.  The cluster counts follow args.max_num_nodes (the DATASET's maximum, main.py:227-229):
    ceil(f max_num_nodes), then ceil(f previous), f = 0.1 for one layer and 0.25 otherwise."""

    def __init__(self, args):
        super().__init__()
        dim_features = args.num_features
        dim_target = args.num_classes
        self.max_num_nodes = args.max_num_nodes
        additional = getattr(args, "additional", None)
        if additional:
            config = json.loads(additional) if isinstance(additional, (str, bytes)) else dict(additional)
        else:
            config = dict(DEFAULT_CONFIG)
        num_diffpool_layers = config["num_layers"]
        gnn_dim_hidden = config["gnn_dim_hidden"]
        dim_embedding = config["dim_embedding"]
        dim_embedding_MLP = config["dim_embedding_MLP"]
        self.num_diffpool_layers = num_diffpool_layers
        coarse_factor = 0.1 if num_diffpool_layers == 1 else 0.25
        gnn_dim_input = dim_features
        no_new_clusters = ceil(coarse_factor * self.max_num_nodes)
        gnn_embed_dim_output = (NUM_SAGE_LAYERS - 1) * gnn_dim_hidden + dim_embedding
        layers = []
        for _ in range(num_diffpool_layers):
            layer = DiffPoolLayer(gnn_dim_input, gnn_dim_hidden, dim_embedding, no_new_clusters)
            layer.compute_losses = False                                       # forward drops them (diffpool.py:160-162)
            layers.append(layer)
            gnn_dim_input = gnn_embed_dim_output
            no_new_clusters = ceil(no_new_clusters * coarse_factor)
        self.diffpool_layers = nn.ModuleList(layers)
        self.final_embed = SAGEConvolutions(gnn_embed_dim_output, gnn_dim_hidden, dim_embedding, lin=False)
        final_embed_dim_output = gnn_embed_dim_output * (num_diffpool_layers + 1)
        self.lin1 = HipLinear(final_embed_dim_output, dim_embedding_MLP)
        self.lin2 = HipLinear(dim_embedding_MLP, dim_target)

    def forward(self, data):
        x, adj = data.x, diffpool_index_of(data)                               # level 0: ragged rows, no padded tensors
        x_all = []
        for layer in self.diffpool_layers:
            x, adj, _, _ = layer(x, adj)                                       # [B, C, F], [B, C, C] from here on
            x_all.append(torch.max(x, dim=1)[0])
        x = self.final_embed(x, adj)
        x_all.append(torch.max(x, dim=1)[0])
        x = torch.cat(x_all, dim=1)
        x = F.relu(self.lin1(x))
        return F.log_softmax(self.lin2(x), dim=-1)
