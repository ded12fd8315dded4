"""The float64 restatement of HGP-SL on ragged per-graph blocks (a helper of the HGP-SL tests and of make_golden_gc_hgpsl.py): plain
torch, one graph at a time, nothing shared with the package.  Edges are (row, col); messages flow from row to col."""
import torch


def k_of(ratio, n):
    """ceil(float32(ratio) float32(n)) as torch computes (ratio * n.float()).ceil()."""
    return int((ratio * torch.tensor([n], dtype=torch.float32)).ceil().long())


def score(x, ei, w):
    x = x.detach().double()
    N, row, col = x.shape[0], ei[0], ei[1]
    w = torch.ones(ei.shape[1], dtype=torch.float64) if w is None else w.detach().double()
    deg = torch.zeros(N, dtype=torch.float64).index_add_(0, row, w)
    dinv = torch.where(deg > 0, deg.pow(-0.5), torch.zeros_like(deg))
    coef = dinv[row] * w * dinv[col]
    out = x - torch.zeros_like(x).index_add_(0, col, coef.view(-1, 1) * x[row])
    return out.abs().sum(1)


def select(sc, ptr, ratio):
    """perm (per graph by descending score, ties to the lower node), pooled boundaries, the smallest relative gap of two adjacent
    sorted scores of a graph."""
    perm, pptr, gap = [], [0], float("inf")
    for g in range(len(ptr) - 1):
        beg, end = ptr[g], ptr[g + 1]
        s = sc[beg:end].tolist()
        order = sorted(range(end - beg), key=lambda i: (-s[i], i))
        for a, b in zip(order[:-1], order[1:]):
            gap = min(gap, (s[a] - s[b]) / max(abs(s[a]), 1e-300))
        k = min(k_of(ratio, end - beg), end - beg)
        perm += [beg + i for i in order[:k]]
        pptr.append(pptr[-1] + k)
    return torch.tensor(perm, dtype=torch.long), pptr, gap


def sparsemax_rows(z):
    """(sparsemax over the last dimension of z [k, k], the smallest |rho z_(rho) - (cumsum_rho - 1)| of its support decisions)."""
    z = z - z.max(dim=-1, keepdim=True).values
    srt = torch.sort(z, dim=-1, descending=True).values
    cs = srt.cumsum(-1) - 1.0
    rho = torch.arange(1, z.shape[-1] + 1, dtype=z.dtype)
    dec = rho * srt - cs
    kk = (dec > 0).sum(-1, keepdim=True)
    tau = cs.gather(-1, kk - 1) / kk.to(z.dtype)
    return torch.clamp(z - tau, min=0), float(dec.detach().abs().min())


def structure(xp, perm, pptr, num_nodes, ei, w, att, sparse=False, lamb=1.0, slope=0.2):
    """The structure learning over the kept nodes perm (pooled boundaries pptr: host list) -> dict: blocks (list of [k, k]),
    edge_index, edge_attr, support_margin."""
    H = xp.shape[1]
    inv = torch.full((num_nodes,), -1, dtype=torch.long)
    inv[perm] = torch.arange(perm.numel())
    r, c = inv[ei[0]], inv[ei[1]]
    keep = (r >= 0) & (c >= 0)
    out = dict(support_margin=float("inf"), blocks=[])
    a = att.reshape(-1)
    p, q = xp @ a[:H], xp @ a[H:]
    ww = torch.ones(ei.shape[1], dtype=xp.dtype) if w is None else w
    rows, cols, vals = [], [], []
    for g in range(len(pptr) - 1):
        c0, c1 = pptr[g], pptr[g + 1]
        k = c1 - c0
        if k == 0:
            out["blocks"].append(xp.new_zeros((0, 0)))
            continue
        m = keep & (r >= c0) & (r < c1)
        A = xp.new_zeros((k, k)).index_put((r[m] - c0, c[m] - c0), ww[m])
        z = torch.nn.functional.leaky_relu(p[c0:c1].view(-1, 1) + q[c0:c1].view(1, -1), slope) + lamb * A
        if sparse:
            o, margin = sparsemax_rows(z)
            out["support_margin"] = min(out["support_margin"], margin)
        else:
            e = (z - z.max(-1, keepdim=True).values).exp()
            o = e / (e.sum(-1, keepdim=True) + 1e-16)
        out["blocks"].append(o)
        nz = o.detach().nonzero(as_tuple=True)
        rows.append(nz[0] + c0)
        cols.append(nz[1] + c0)
        vals.append(o[nz])
    if rows:
        out.update(edge_index=torch.stack([torch.cat(rows), torch.cat(cols)]), edge_attr=torch.cat(vals))
    else:
        out.update(edge_index=torch.zeros((2, 0), dtype=torch.long), edge_attr=xp.new_zeros(0))
    return out


def pool(x, ei, w, ptr, att, ratio=0.8, sparse=False, lamb=1.0, slope=0.2, sl=True):
    """One HGPSLPool call.  x [N, H], att [1, 2 H], w [E] or None (autograd flows to the three); ptr: host list of the graph
    boundaries.  Returns a dict: x, edge_index, edge_attr, batch, perm, ptr, blocks (list of [k, k]), score, score_gap, support_margin."""
    N = x.shape[0]
    sc = score(x, ei, w)
    perm, pptr, gap = select(sc, ptr, ratio)
    xp = x[perm]
    batch = torch.tensor([g for g in range(len(ptr) - 1) for _ in range(pptr[g + 1] - pptr[g])], dtype=torch.long)
    out = dict(x=xp, batch=batch, perm=perm, ptr=pptr, score=sc, score_gap=gap, support_margin=float("inf"), blocks=[])
    if not sl:
        inv = torch.full((N,), -1, dtype=torch.long)
        inv[perm] = torch.arange(perm.numel())
        r, c = inv[ei[0]], inv[ei[1]]
        keep = (r >= 0) & (c >= 0)
        out.update(edge_index=torch.stack([r[keep], c[keep]]), edge_attr=None if w is None else w[keep])
        return out
    out.update(structure(xp, perm, pptr, N, ei, w, att, sparse, lamb, slope))
    return out


def flat_blocks(blocks):
    return torch.cat([b.reshape(-1) for b in blocks]) if blocks else torch.zeros(0, dtype=torch.float64)


def gcn(x, ei, w, weight, bias):
    """The GCN conv of the same file: the degree by row, no self loops added."""
    N, row, col = x.shape[0], ei[0], ei[1]
    w = torch.ones(ei.shape[1], dtype=x.dtype) if w is None else w
    deg = torch.zeros(N, dtype=x.dtype).index_add(0, row, w)
    dinv = torch.where(deg > 0, deg.clamp(min=1e-300).pow(-0.5), torch.zeros_like(deg))
    h = x @ weight
    out = torch.zeros_like(h).index_add(0, col, (dinv[row] * w * dinv[col]).view(-1, 1) * h[row])
    return out if bias is None else out + bias
