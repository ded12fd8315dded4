"""A float64 torch restatement of ops.txl_attention, written from the formulas of DESIGN.md "SI count models: TXL" and none of the
package's code: the window of every segment, the reference's rel_shift as a FLAT re-indexing (a gather, not the pad-and-view), the
softmax over the whole window and the memory rows read from their own tensors, so that autograd returns their gradient apart from
the own rows'.  Also the loader of tests/golden/si_txl*.npz shared by the host and the GPU tests."""
import json
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def windows(Lp, seg, mem):
    """[(first key row, memory rows, first query row)] of the Lp / seg segments."""
    out = []
    for s in range(Lp // seg):
        mlen = min(mem, s * seg)
        out.append((s * seg - mlen, mlen, s * seg))
    return out


def shift_index(qlen, klen):
    """(row, col) [qlen, klen] of the shifted entry (i, j): f = i klen + j + qlen, row = f // (klen + 1), col = f % (klen + 1); the
    entry is 0 where col == 0, else BD[row, col - 1]."""
    i = torch.arange(qlen).view(-1, 1)
    j = torch.arange(klen).view(1, -1)
    f = i * klen + j + qlen
    return f // (klen + 1), f % (klen + 1)


def attention(q, k, v, k_mem, v_mem, rk, r_w_bias, r_r_bias, seg, mem, scale):
    """out [B, Lp, n d] in the dtype of q (the tests pass float64 leaves and read their .grad)."""
    B, Lp, n, d = q.shape
    outs = []
    for k0, mlen, q0 in windows(Lp, seg, mem):
        klen = seg + mlen
        qs = q[:, q0:q0 + seg]
        keys = [k_mem[:, k0 + j] if j < mlen else k[:, k0 + j] for j in range(klen)]
        vals = [v_mem[:, k0 + j] if j < mlen else v[:, k0 + j] for j in range(klen)]
        K, V = torch.stack(keys, 1), torch.stack(vals, 1)                          # [B, klen, n, d]
        R = rk[klen - 1 - torch.arange(klen)]                                      # row j: relative position klen - 1 - j
        ac = torch.einsum("bind,bjnd->bijn", qs + r_w_bias, K)
        bd = torch.einsum("bind,jnd->bijn", qs + r_r_bias, R)
        row, col = shift_index(seg, klen)
        assert int(row.max()) < seg
        shifted = bd[:, row, (col - 1).clamp(min=0)] * (col > 0).to(bd.dtype).view(1, seg, klen, 1)
        score = (ac + shifted) * scale
        score = score - score.max(dim=2, keepdim=True)[0]
        e = torch.exp(score)
        prob = e / e.sum(dim=2, keepdim=True)
        outs.append(torch.einsum("bijn,bjnd->bind", prob, V).reshape(B, seg, n * d))
    return torch.cat(outs, 1)


def load_cases():
    """Every case of si_txl.npz, si_txl_2.npz, ...: [(meta dict, {key: array})]."""
    cases = []
    for fname in sorted(f for f in os.listdir(GOLDEN) if f.startswith("si_txl") and f.endswith(".npz")):
        z = np.load(os.path.join(GOLDEN, fname))
        for m in json.loads(bytes(z["meta"]).decode()):
            arrs = {}
            for key, kind, off, shape in m["index"]:
                cnt = int(np.prod(shape)) if shape else 1
                a = z["%s/%s" % (m["tag"], kind)][off:off + cnt].reshape(shape)
                arrs[key] = a.astype(bool) if kind == "u8" else a
            cases.append((m, arrs))
    return cases
