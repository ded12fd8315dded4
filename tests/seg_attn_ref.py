"""Float64 restatement of ragged multi-head attention with sparsemax or softmax weights, and of DIAMNet's window pooling; and
the loader of tests/golden/si_attn.npz.

Written from the published definitions, on CPU tensors, with a Python loop over the pairs:

* sparsemax (Martins & Astudillo 2016, algorithm 1): sort z descending, k = max{j : 1 + j z_(j) > sum_{i <= j} z_(i)},
  tau = (sum_{i <= k} z_(i) - 1) / k, p = max(z - tau, 0);
* attention: per pair and head z = scale * q_h k_h^T over the pair's live keys, out_h = p v_h; a skipped key takes no weight, a
  skipped query row is a zero row;
* window pooling: per pair the rows first live .. last live (L of them; skipped rows inside are zero rows); L <= mem_len: the rows,
  front-padded with zero rows; else mem_len windows of `kernel = L - (mem_len - 1) * stride` rows every `stride = L // mem_len`."""
import json
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "si_attn.npz")


def load_golden():
    z = np.load(GOLDEN)
    cases = {}
    for m in json.loads(bytes(z["meta"]).decode()):
        arrays = {}
        for name, kind, off, shape in m["index"]:
            blob = z["%s/%s" % (m["tag"], kind)]
            n = int(np.prod(shape)) if shape else 1
            a = blob[off:off + n].reshape(shape)
            arrays[name] = a.astype(bool) if kind == "u8" else a
        m["arrays"] = arrays
        cases[m["name"]] = m
    return cases


def rel_max(a, b):
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp(min=1e-12)) if b.numel() else 0.0


def sparsemax(z):
    """z [..., n] float64 -> (p, tau)."""
    zs = torch.sort(z, dim=-1, descending=True)[0]
    cs = torch.cumsum(zs, -1)
    r = torch.arange(1, z.shape[-1] + 1, dtype=z.dtype)
    k = ((1 + r * zs) > cs).to(z.dtype).sum(-1, keepdim=True)
    tau = (torch.gather(cs, -1, k.long() - 1) - 1) / k
    return torch.clamp(z - tau, min=0), tau


def seg_attention(q, k, v, q_ptr, k_ptr, heads, scale, score="sparsemax", q_skip=None, k_skip=None):
    """(out [Nq, H] float64, margin): margin = the smallest |z - tau| over all live (query, head, key) (inf for softmax)."""
    q, k, v = q.double(), k.double(), v.double()
    Nq, H = q.shape
    dk = H // heads
    rows = []
    margin = float("inf")
    for b in range(len(q_ptr) - 1):
        q0, q1, k0, k1 = int(q_ptr[b]), int(q_ptr[b + 1]), int(k_ptr[b]), int(k_ptr[b + 1])
        live = torch.ones(k1 - k0, dtype=torch.bool) if k_skip is None else ~torch.as_tensor(k_skip[k0:k1]).bool()
        qb = q[q0:q1].view(q1 - q0, heads, dk)
        kb, vb = k[k0:k1][live].view(-1, heads, dk), v[k0:k1][live].view(-1, heads, dk)
        if kb.shape[0] == 0:
            rows.append(torch.zeros(q1 - q0, H, dtype=q.dtype) + 0 * qb.reshape(q1 - q0, H))
            continue
        z = torch.einsum("ind,jnd->inj", qb, kb) * scale
        if score == "sparsemax":
            p, tau = sparsemax(z)
            keep = torch.ones(q1 - q0, dtype=torch.bool) if q_skip is None else ~torch.as_tensor(q_skip[q0:q1]).bool()
            if keep.any():
                margin = min(margin, float((z - tau).detach()[keep].abs().min()))
        else:
            p = torch.softmax(z, dim=-1)
        o = torch.einsum("inj,jnd->ind", p, vb).reshape(q1 - q0, H)
        if q_skip is not None:
            o = o * (~torch.as_tensor(q_skip[q0:q1]).bool()).to(o.dtype).view(-1, 1)
        rows.append(o)
    return torch.cat(rows, 0), margin


def seg_window_pool(rows, ptr, skip, mem_len, mode):
    """(mem [B * mem_len, D] float64, mem_mask [B, mem_len] bool)."""
    rows = rows.double()
    D = rows.shape[1]
    mems, masks = [], []
    for b in range(len(ptr) - 1):
        r0, r1 = int(ptr[b]), int(ptr[b + 1])
        live = torch.ones(r1 - r0, dtype=torch.bool) if skip is None else ~torch.as_tensor(skip[r0:r1]).bool()
        idx = torch.nonzero(live).view(-1)
        if idx.numel() == 0:
            mems.append(torch.zeros(mem_len, D, dtype=rows.dtype) + 0 * rows[:1].sum())
            masks.append(torch.zeros(mem_len, dtype=torch.bool))
            continue
        s, e = int(idx[0]), int(idx[-1]) + 1
        x = rows[r0 + s:r0 + e] * live[s:e].to(rows.dtype).view(-1, 1)
        mk = live[s:e]
        L = e - s
        if L <= mem_len:
            mems.append(torch.cat([torch.zeros(mem_len - L, D, dtype=rows.dtype), x], 0))
            masks.append(torch.cat([torch.zeros(mem_len - L, dtype=torch.bool), mk]))
            continue
        stride = L // mem_len
        kernel = L - (mem_len - 1) * stride
        out, om = [], []
        for i in range(mem_len):
            w = x[i * stride:i * stride + kernel]
            out.append(w.max(0)[0] if mode == "max" else (w.sum(0) if mode == "sum" else w.mean(0)))
            om.append(bool(mk[i * stride:i * stride + kernel].any()))
        mems.append(torch.stack(out, 0))
        masks.append(torch.tensor(om))
    return torch.cat(mems, 0), torch.stack(masks, 0)
