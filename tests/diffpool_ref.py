"""The DiffPool classifier restated on ragged rows in plain torch (no padded tensor, nothing built from the package): the expected
side of tests/test_diffpool_host.py (pinned there against the reference's own run, tests/golden/gc_diffpool.npz, in float64) and of
tests/test_gpu_diffpool.py.

Parameters and buffers come in a dict `p` under the reference's state_dict names; a training-mode call writes the BatchNorm buffers
it would leave behind into `after` (same names).  Level 0 works on the rows x [N, F] with the edges (src, dst) and the graph
boundaries ptr (a list of B + 1 integers); the levels behind it on [B, C, F] / [B, C, C].

  aggregation   row i: sum of x[dst(e)] over the edges with src(e) = i, divided by max(out-degree, 1)
  BatchNorm     level 0: over n = B Nmax rows of which B Nmax - N are zero rows that are not stored: mean = sum / n,
                var = sum of squares / n - mean^2, running variance times n / (n - 1); dense levels: over the B C rows
  pooling       S = softmax(s); per graph X' = S^T Z, A' = S^T (A S)
  losses        link = sqrt(||A||_F^2 - 2 tr(A') + ||S^T S||_F^2) / (B Nmax^2) (||A||_F^2 over duplicate-summed entries),
                ent = sum(-S log(S + 1e-15)) / (B Nmax); dense levels: the plain formulas
"""
import torch
import torch.nn.functional as F

EPS = 1e-15
BN_EPS, BN_MOMENTUM = 1e-5, 0.1


def _bn(p, pre, h, n, training, after):
    """h [rows, C]; n >= rows: the rows counted in the statistics (the others are zeros)."""
    if training:
        mean = h.sum(0) / n
        var = (h * h).sum(0) / n - mean * mean
        if after is not None:
            after[pre + "running_mean"] = (1 - BN_MOMENTUM) * p[pre + "running_mean"] + BN_MOMENTUM * mean.detach()
            after[pre + "running_var"] = (1 - BN_MOMENTUM) * p[pre + "running_var"] + BN_MOMENTUM * var.detach() * n / (n - 1)
            after[pre + "num_batches_tracked"] = p[pre + "num_batches_tracked"] + 1
    else:
        mean, var = p[pre + "running_mean"], p[pre + "running_var"]
    return (h - mean) / torch.sqrt(var + BN_EPS) * p[pre + "weight"] + p[pre + "bias"]


def _conv(p, pre, x, agg):
    return agg @ p[pre + "lin_rel.weight"].t() + x @ p[pre + "lin_root.weight"].t() + p[pre + "lin_root.bias"]


def _sage(p, pre, x, aggregate, n, training, after):
    """SAGEConvolutions on 2-D rows; aggregate(h) is the mean aggregation of the level."""
    x1 = _bn(p, pre + "bn1.", F.relu(_conv(p, pre + "conv1.", x, aggregate(x))), n, training, after)
    x2 = _bn(p, pre + "bn2.", F.relu(_conv(p, pre + "conv2.", x1, aggregate(x1))), n, training, after)
    x3 = _conv(p, pre + "conv3.", x2, aggregate(x2))
    out = torch.cat([x1, x2, x3], dim=-1)
    if pre + "lin.weight" in p:
        out = out @ p[pre + "lin.weight"].t() + p[pre + "lin.bias"]
    return out


def out_edge_mean(x, src, dst):
    deg = torch.bincount(src, minlength=x.shape[0]).clamp(min=1).to(x.dtype)
    return torch.zeros_like(x).index_add(0, src, x[dst]) / deg.view(-1, 1)


def assign(s, z, src, dst, ptr):
    """(X' [B, C, F], A' [B, C, C], S, A S) from the logits s [N, C] and z [N, F]."""
    S = torch.softmax(s, dim=-1)
    AS = torch.zeros_like(S).index_add(0, src, S[dst])
    X = torch.stack([S[a:b].t() @ z[a:b] for a, b in zip(ptr[:-1], ptr[1:])])
    A = torch.stack([S[a:b].t() @ AS[a:b] for a, b in zip(ptr[:-1], ptr[1:])])
    return X, A, S, AS


def layer0(p, pre, x, src, dst, ptr, training=True, after=None):
    """DiffPoolLayer at level 0 -> (x' [B, C, F], adj' [B, C, C], link loss, entropy loss)."""
    B, nmax, N = len(ptr) - 1, max(b - a for a, b in zip(ptr[:-1], ptr[1:])), x.shape[0]
    n = B * nmax
    aggregate = lambda h: out_edge_mean(h, src, dst)  # noqa: E731
    s = _sage(p, pre + "gnn_pool.", x, aggregate, n, training, after)
    z = _sage(p, pre + "gnn_embed.", x, aggregate, n, training, after)
    X, A, S, _ = assign(s, z, src, dst, ptr)
    _, mult = torch.unique(src * N + dst, return_counts=True)
    gram = torch.stack([S[a:b].t() @ S[a:b] for a, b in zip(ptr[:-1], ptr[1:])])
    sq = (mult.to(x.dtype) ** 2).sum() - 2 * torch.diagonal(A, dim1=1, dim2=2).sum() + (gram * gram).sum()
    link = torch.sqrt(sq.clamp(min=0)) / (B * nmax * nmax)
    ent = (-S * torch.log(S + EPS)).sum() / n
    return X, A, link, ent


def _dense_sage(p, pre, x, adj, training, after):
    B, C, _ = x.shape
    deg = adj.sum(-1, keepdim=True).clamp(min=1)
    aggregate = lambda h: (torch.bmm(adj, h.view(B, C, -1)) / deg).reshape(B * C, -1)  # noqa: E731
    return _sage(p, pre, x.reshape(B * C, -1), aggregate, B * C, training, after).view(B, C, -1)


def dense_layer(p, pre, x, adj, training=True, after=None):
    """DiffPoolLayer at a dense level (no mask) -> (x', adj', link loss, entropy loss)."""
    s = _dense_sage(p, pre + "gnn_pool.", x, adj, training, after)
    z = _dense_sage(p, pre + "gnn_embed.", x, adj, training, after)
    S = torch.softmax(s, dim=-1)
    St = S.transpose(1, 2)
    link = torch.norm(adj - torch.bmm(S, St), p=2) / adj.numel()
    ent = (-S * torch.log(S + EPS)).sum(dim=-1).mean()
    return torch.bmm(St, z), torch.bmm(torch.bmm(St, adj), S), link, ent


def forward(p, num_layers, x, src, dst, ptr, training=True, after=None):
    """DiffPool.forward -> log-probs [B, classes]."""
    reads = []
    for i in range(num_layers):
        pre = "diffpool_layers.%d." % i
        if i == 0:
            x, adj, _, _ = layer0(p, pre, x, src, dst, ptr, training, after)
        else:
            x, adj, _, _ = dense_layer(p, pre, x, adj, training, after)
        reads.append(x.max(dim=1)[0])
    reads.append(_dense_sage(p, "final_embed.", x, adj, training, after).max(dim=1)[0])
    h = F.relu(torch.cat(reads, dim=1) @ p["lin1.weight"].t() + p["lin1.bias"])
    return F.log_softmax(h @ p["lin2.weight"].t() + p["lin2.bias"], dim=-1)
