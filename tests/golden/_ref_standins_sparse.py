"""Stand-ins for the torch_geometric / torch_scatter / torch_sparse names the reference's models/hgpsl.py and models/sparse_softmax.py
import.

TEST TOOLING ONLY (make_golden_gc_hgpsl.py), like _ref_standins_dense.py: nothing here is imported by the product package and nothing
here is reference source.  The three libraries are not installed where the goldens are made, so the published definitions
(torch_geometric 2.0.2, torch_scatter 2.0.9) are restated in plain torch -- PARITY UNPINNED against the real libraries:

* ``MessagePassing(aggr='add')``: ``propagate(edge_index, x=x, **kw)`` = ``update(sum at edge_index[1] of message(x_j = x[edge_index[0]], **kw))``.
* ``topk(x, ratio, batch)``: per graph the ``ceil(ratio * n.float())`` highest entries by a descending sort of the padded batch
  (``TOPK_PERMS`` records every result: the reference's forward does not return perm).
* ``filter_adj``, ``softmax(src, index, num_nodes)`` (max subtracted, 1e-16 added to the sum), ``dense_to_sparse``,
  ``add_remaining_self_loops``; ``scatter_add`` / ``scatter_max`` of torch_scatter; bare names for ``Data``, ``spspmm``, ``coalesce``
  (only ``sample=True`` reaches them).

A REFERENCE QUIRK recorded here: hgpsl.py calls ``softmax(weights, row, x.size(0))``.  In torch_geometric 2.0.2's signature
``softmax(src, index=None, ptr=None, num_nodes=None, dim=0)`` the third positional argument appears to be ``ptr``, which would make the
default ``sparse=False`` branch unrunnable as shipped.  The stand-in takes an int there as ``num_nodes``: the evident intent, and the
signature of the torch_geometric the file was written for.
"""
import sys
import types

import torch

TOPK_PERMS = []


def scatter_add(src, index, dim=-1, out=None, dim_size=None):
    assert (dim == 0 or (dim == -1 and src.dim() == 1)) and out is None
    n = int(index.max()) + 1 if dim_size is None and index.numel() else int(dim_size or 0)
    return src.new_zeros((n,) + tuple(src.shape[1:])).index_add_(0, index, src)


def scatter_max(src, index, dim=-1, out=None, dim_size=None):
    assert dim in (0, -1) and out is None and src.dim() == 1
    n = int(index.max()) + 1 if dim_size is None and index.numel() else int(dim_size or 0)
    res = src.new_full((n,), float("-inf")).scatter_reduce(0, index, src, reduce="amax", include_self=True)
    return res, None


class MessagePassing(torch.nn.Module):
    def __init__(self, aggr="add", **kwargs):
        super().__init__()
        assert aggr == "add" and not kwargs
        self.aggr = aggr

    def propagate(self, edge_index, x, **kwargs):
        msg = self.message(x_j=x[edge_index[0]], **kwargs)
        return self.update(torch.zeros((x.size(0),) + tuple(msg.shape[1:]), dtype=msg.dtype).index_add_(0, edge_index[1], msg))


def topk(x, ratio, batch, min_score=None, tol=1e-7):
    assert min_score is None
    num_nodes = scatter_add(batch.new_ones(x.size(0)), batch, dim=0)
    batch_size, max_num_nodes = num_nodes.size(0), int(num_nodes.max())
    cum = torch.cat([num_nodes.new_zeros(1), num_nodes.cumsum(dim=0)[:-1]], dim=0)
    index = torch.arange(batch.size(0), dtype=torch.long) - cum[batch] + batch * max_num_nodes
    dense_x = x.new_full((batch_size * max_num_nodes,), torch.finfo(x.dtype).min)
    dense_x[index] = x
    dense_x = dense_x.view(batch_size, max_num_nodes)
    _, perm = dense_x.sort(dim=-1, descending=True)
    perm = (perm + cum.view(-1, 1)).view(-1)
    k = (ratio * num_nodes.to(torch.float)).ceil().to(torch.long)
    mask = [torch.arange(int(k[i]), dtype=torch.long) + i * max_num_nodes for i in range(batch_size)]
    perm = perm[torch.cat(mask, dim=0)]
    TOPK_PERMS.append(perm.clone())
    return perm


def filter_adj(edge_index, edge_attr, perm, num_nodes=None):
    mask = perm.new_full((int(num_nodes),), -1)
    mask[perm] = torch.arange(perm.size(0), dtype=torch.long)
    row, col = mask[edge_index[0]], mask[edge_index[1]]
    keep = (row >= 0) & (col >= 0)
    return torch.stack([row[keep], col[keep]], dim=0), (edge_attr[keep] if edge_attr is not None else None)


def softmax(src, index, num_nodes=None):
    assert num_nodes is None or isinstance(num_nodes, int)       # (see the module docstring: an int in the `ptr` place)
    n = int(index.max()) + 1 if num_nodes is None else num_nodes
    out = (src - scatter_max(src, index, dim=0, dim_size=n)[0][index]).exp()
    return out / (scatter_add(out, index, dim=0, dim_size=n)[index] + 1e-16)


def dense_to_sparse(adj):
    index = adj.nonzero(as_tuple=True)
    return torch.stack(index, dim=0), adj[index]


def add_remaining_self_loops(edge_index, edge_attr=None, fill_value=1.0, num_nodes=None):
    N = int(num_nodes)
    row, col = edge_index[0], edge_index[1]
    mask = row != col
    loop_index = torch.arange(N, dtype=torch.long).unsqueeze(0).repeat(2, 1)
    if edge_attr is not None:
        loop_attr = edge_attr.new_full((N,), fill_value)
        rest = edge_attr[~mask]
        if rest.numel() > 0:
            loop_attr[row[~mask]] = rest
        edge_attr = torch.cat([edge_attr[mask], loop_attr], dim=0)
    return torch.cat([edge_index[:, mask], loop_index], dim=1), edge_attr


class Data:
    pass


def spspmm(*a, **k):
    raise NotImplementedError("stand-in: only sample=True reaches spspmm")


def coalesce(*a, **k):
    raise NotImplementedError("stand-in: only sample=True reaches coalesce")


def install():
    def mod(name, **names):
        m = types.ModuleType(name)
        for k, v in names.items():
            setattr(m, k, v)
        sys.modules[name] = m
        return m

    mod("torch_geometric")
    mod("torch_geometric.data", Data=Data)
    mod("torch_geometric.nn")
    mod("torch_geometric.nn.conv", MessagePassing=MessagePassing)
    mod("torch_geometric.nn.pool")
    mod("torch_geometric.nn.pool.topk_pool", topk=topk, filter_adj=filter_adj)
    mod("torch_geometric.utils", softmax=softmax, dense_to_sparse=dense_to_sparse, add_remaining_self_loops=add_remaining_self_loops)
    mod("torch_scatter", scatter_add=scatter_add, scatter_max=scatter_max)
    mod("torch_sparse", spspmm=spspmm, coalesce=coalesce)
