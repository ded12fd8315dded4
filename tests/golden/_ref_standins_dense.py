"""Stand-ins for the dense torch_geometric names the reference's models/diffpool.py imports.

TEST TOOLING ONLY (make_golden_gc_diffpool.py), like _ref_standins.py: nothing here is imported by the product package and nothing
here is reference source.  torch_geometric 2.0.2 is not installed where the goldens are made, so the published definitions are
restated in plain torch -- PARITY UNPINNED against a real torch_geometric:

* ``DenseSAGEConv(in, out, normalize=False, bias=True)``: ``lin_rel = Linear(in, out, bias=False)``, ``lin_root = Linear(in, out,
  bias=bias)`` (both ``torch.nn.Linear``); ``forward(x, adj, mask=None)`` = lin_rel((adj @ x) / adj.sum(-1).clamp(min=1)) + lin_root(x),
  L2-normalised when asked, times the mask.  The ``add_loop=False`` keyword the reference passes is accepted and ignored.
* ``dense_diff_pool(x, adj, s, mask=None)`` -> (S^T X, S^T A S, ||A - S S^T|| / numel(A), mean row entropy), S = softmax(s, -1), x and S
  masked, EPS = 1e-15.
* ``to_dense_batch(x, batch)`` -> ([B, Nmax, F] left-aligned rows, [B, Nmax] mask); ``to_dense_adj(edge_index, batch)`` -> [B, Nmax, Nmax]
  with edge (src, dst) ADDED at [graph, src - first, dst - first] (duplicates sum, self loops stay); Nmax = the batch's largest graph.
* ``ToDense``: a bare name (the reference imports it and never calls it).
"""
import sys
import types

import torch

EPS = 1e-15


class DenseSAGEConv(torch.nn.Module):
    def __init__(self, in_channels, out_channels, normalize=False, bias=True):
        super().__init__()
        self.in_channels, self.out_channels, self.normalize = in_channels, out_channels, normalize
        self.lin_rel = torch.nn.Linear(in_channels, out_channels, bias=False)
        self.lin_root = torch.nn.Linear(in_channels, out_channels, bias=bias)
        self.reset_parameters()

    def reset_parameters(self):
        self.lin_rel.reset_parameters()
        self.lin_root.reset_parameters()

    def forward(self, x, adj, mask=None, add_loop=False):
        x = x.unsqueeze(0) if x.dim() == 2 else x
        adj = adj.unsqueeze(0) if adj.dim() == 2 else adj
        B, N, _ = adj.size()
        out = torch.matmul(adj, x)
        out = out / adj.sum(dim=-1, keepdim=True).clamp(min=1)
        out = self.lin_rel(out) + self.lin_root(x)
        if self.normalize:
            out = torch.nn.functional.normalize(out, p=2.0, dim=-1)
        if mask is not None:
            out = out * mask.view(B, N, 1).to(x.dtype)
        return out


def dense_diff_pool(x, adj, s, mask=None):
    x = x.unsqueeze(0) if x.dim() == 2 else x
    adj = adj.unsqueeze(0) if adj.dim() == 2 else adj
    s = s.unsqueeze(0) if s.dim() == 2 else s
    batch_size, num_nodes, _ = x.size()
    s = torch.softmax(s, dim=-1)
    if mask is not None:
        mask = mask.view(batch_size, num_nodes, 1).to(x.dtype)
        x, s = x * mask, s * mask
    out = torch.matmul(s.transpose(1, 2), x)
    out_adj = torch.matmul(torch.matmul(s.transpose(1, 2), adj), s)
    link_loss = adj - torch.matmul(s, s.transpose(1, 2))
    link_loss = torch.norm(link_loss, p=2)
    link_loss = link_loss / adj.numel()
    ent_loss = (-s * torch.log(s + EPS)).sum(dim=-1).mean()
    return out, out_adj, link_loss, ent_loss


def _layout(batch, batch_size=None):
    B = int(batch.max()) + 1 if batch_size is None else int(batch_size)
    cnt = torch.bincount(batch, minlength=B)
    first = torch.cat([cnt.new_zeros(1), torch.cumsum(cnt, 0)])[:-1]
    return B, int(cnt.max()), first


def to_dense_batch(x, batch=None, fill_value=0.0, max_num_nodes=None, batch_size=None):
    if batch is None:
        batch = torch.zeros(x.shape[0], dtype=torch.long)
    B, nmax, first = _layout(batch, batch_size)
    nmax = nmax if max_num_nodes is None else int(max_num_nodes)
    pos = torch.arange(x.shape[0]) - first[batch]
    out = x.new_full((B, nmax) + tuple(x.shape[1:]), fill_value)
    out[batch, pos] = x
    mask = torch.zeros((B, nmax), dtype=torch.bool)
    mask[batch, pos] = True
    return out, mask


def to_dense_adj(edge_index, batch=None, edge_attr=None, max_num_nodes=None):
    assert edge_attr is None
    if batch is None:
        batch = torch.zeros(int(edge_index.max()) + 1 if edge_index.numel() else 0, dtype=torch.long)
    B, nmax, first = _layout(batch)
    nmax = nmax if max_num_nodes is None else int(max_num_nodes)
    g = batch[edge_index[0]]
    i, j = edge_index[0] - first[g], edge_index[1] - first[g]
    flat = torch.zeros(B * nmax * nmax, dtype=torch.get_default_dtype())
    flat.index_add_(0, (g * nmax + i) * nmax + j, torch.ones(edge_index.shape[1], dtype=flat.dtype))
    return flat.view(B, nmax, nmax)


class ToDense:
    pass


def install():
    """Register torch_geometric.nn / .utils / .transforms with the names above (replacing what _ref_standins.install put there for nn)."""
    pyg = sys.modules.get("torch_geometric") or types.ModuleType("torch_geometric")
    nn = getattr(pyg, "nn", None) or types.ModuleType("torch_geometric.nn")
    nn.DenseSAGEConv, nn.dense_diff_pool = DenseSAGEConv, dense_diff_pool
    utils = types.ModuleType("torch_geometric.utils")
    utils.to_dense_batch, utils.to_dense_adj = to_dense_batch, to_dense_adj
    tr = types.ModuleType("torch_geometric.transforms")
    tr.ToDense = ToDense
    pyg.nn, pyg.utils, pyg.transforms = nn, utils, tr
    sys.modules["torch_geometric"] = pyg
    sys.modules["torch_geometric.nn"] = nn
    sys.modules["torch_geometric.utils"] = utils
    sys.modules["torch_geometric.transforms"] = tr
