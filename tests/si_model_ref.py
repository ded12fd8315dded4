"""Float64 restatement of GraphAdjModel.forward outside the rep nets (subgraph_isomorphism/models/basemodel.py:830-982,
filter.py:10-16, pred.py:17-236, utils/dl.py:51-127): label filter, code embedding, padded masks and the padded head.

Written from the reference's formulas on plain CPU tensors and fed the rep outputs (p_v_rep / g_v_rep) as leaves, so the
gradients into them come out of autograd here.  tests/test_si_model_host.py pins it against the goldens the reference itself
produced (tests/golden/si_models.npz); the GPU tests then use it as the reference for the HIP glue."""
import json
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "si_models.npz")
OUT_KEYS = ("p_v_emb", "p_e_emb", "g_v_emb", "g_e_emb", "p_v_rep", "p_e_rep", "g_v_rep", "g_e_rep", "p_v_mask", "p_e_mask",
            "g_v_mask", "g_e_mask", "pred_c", "pred_v", "pred_e")


def load_golden():
    """{case name: meta dict with "arrays" = {name: np.ndarray}} of si_models.npz."""
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


def state_dict(case, prefix="param"):
    """The full state_dict (aliases of shared modules included) of `prefix` ("init" | "param") as CPU tensors."""
    a = case["arrays"]
    sd = {}
    for k in case["keys"]:
        src = case["alias"].get(k, k)
        sd[k] = torch.from_numpy(np.array(a["%s/%s" % (prefix, src)]))
    return sd


def batch(case, side):
    a = case["arrays"]
    d = {k: a["%s/%s" % (side, k)] for k in ("sizes", "u", "v", "id", "label", "elabel")}
    d["dummy"] = a.get("%s/dummy" % side)
    return d


def rel_max(a, b):
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp(min=1e-12)) if b.numel() else 0.0


# ------------------------------------------------------------------------------------------------ pieces
def pad_mask(sizes, dummy):
    """batch_convert_len_to_mask(pre_pad=True) with the dummy positions cleared: [B, L] bool."""
    sizes = [int(s) for s in sizes]
    L = max(sizes)
    mask = torch.zeros(len(sizes), L, dtype=torch.bool)
    off = 0
    for b, n in enumerate(sizes):
        for j in range(n):
            mask[b, L - n + j] = not (dummy is not None and bool(dummy[off + j]))
        off += n
    return mask


def gate(p, g):
    """[Ng] 0/1: label of graph node v occurs in pattern b, or is 0 while pattern b is shorter than the longest pattern."""
    Lp = int(max(p["sizes"]))
    out = np.zeros(len(g["label"]), np.float64)
    po = go = 0
    for b in range(len(p["sizes"])):
        pn, gn = int(p["sizes"][b]), int(g["sizes"][b])
        labs = set(int(x) for x in p["label"][po:po + pn])
        if pn < Lp:
            labs.add(0)
        for v in range(go, go + gn):
            out[v] = 1.0 if int(g["label"][v]) in labs else 0.0
        po, go = po + pn, go + gn
    return torch.from_numpy(out).view(-1, 1)


def embed(sd, side, d, add_node_id):
    """enc_vl[label] @ W_vl (+ enc_v[id] @ W_v), float64."""
    enc, emb = ("g_enc_net", "g_emb_net") if side == "g" else ("p_enc_net", "p_emb_net")
    lab = torch.from_numpy(np.asarray(d["label"], np.int64))
    out = sd[enc + ".vl.weight"].double()[lab] @ sd[emb + ".vl.weight"].double()
    if add_node_id:
        ids = torch.from_numpy(np.asarray(d["id"], np.int64))
        out = out + sd[enc + ".v.weight"].double()[ids] @ sd[emb + ".v.weight"].double()
    return out


def degrees(d):
    n = int(np.sum(d["sizes"]))
    out_deg = np.bincount(np.asarray(d["u"], np.int64), minlength=n)
    in_deg = np.bincount(np.asarray(d["v"], np.int64), minlength=n)
    return torch.from_numpy(out_deg).double().view(-1, 1), torch.from_numpy(in_deg).double().view(-1, 1)


def node_rows(sd, cfg, side, d, rep):
    """[enc_v(id) | enc_vl(label) | out_deg | in_deg | rep] of basemodel.py:914-944 (parts as cfg asks)."""
    enc = "g_enc_net" if side == "g" else "p_enc_net"
    parts = []
    if cfg.get("pred_with_enc", False):
        parts += [sd[enc + ".v.weight"].double()[torch.from_numpy(np.asarray(d["id"], np.int64))],
                  sd[enc + ".vl.weight"].double()[torch.from_numpy(np.asarray(d["label"], np.int64))]]
    if cfg.get("pred_with_deg", False):
        parts += list(degrees(d))
    return torch.cat(parts + [rep], 1) if parts else rep


def pad_rows(rows, sizes):
    """split_and_batchify_graph_feats(pre_pad=True): [B, L, D], zeros in front."""
    sizes = [int(s) for s in sizes]
    L = max(sizes)
    off, chunks = 0, []
    for n in sizes:
        chunks.append(torch.cat([rows.new_zeros(L - n, rows.shape[1]), rows[off:off + n]], 0))
        off += n
    return torch.stack(chunks, 0)


def pred_params(sd):
    """The pred_net.* tensors of a state_dict as float64 leaves (their gradients are the restated parameter gradients)."""
    return {k[len("pred_net."):]: v.detach().double().cpu().requires_grad_(True) for k, v in sd.items() if k.startswith("pred_net.")}


def head(W, cfg, p_out, p_mask, g_out, g_mask):
    """PredictNet.forward (pred.py:90-155) with agg_graph = sum / mean / max over the padded positions, float64.
    W = pred_params(state_dict)."""
    kind = cfg.get("pred_net", "SumPredictNet")
    act = {"relu": torch.relu, "tanh": torch.tanh,
           "leaky_relu": lambda x: torch.nn.functional.leaky_relu(x, 1 / 5.5)}[cfg.get("pred_act_func", "relu")]
    agg = {"SumPredictNet": lambda t: t.sum(1), "MeanPredictNet": lambda t: t.mean(1),
           "MaxPredictNet": lambda t: t.max(1)[0]}[kind]
    lin = lambda x, n: x @ W[n + ".weight"].t() + W[n + ".bias"]              # noqa: E731
    bsz, g_len = p_mask.shape[0], g_mask.shape[1]
    pl = p_mask.double().sum(1).view(bsz, 1)
    gl = g_mask.double().sum(1).view(bsz, 1)
    pl_inv, gl_inv = 1.0 / pl, 1.0 / gl
    p = agg(lin(p_out, "p_fc")).unsqueeze(1).expand(bsz, g_len, -1)
    g = lin(g_out, "g_fc")
    w = None
    if "weight_fc1.weight" in W:
        ex = lambda t: t.expand(bsz, g_len).unsqueeze(-1)                     # noqa: E731
        w = act(lin(torch.cat([p, g, g - p, g * p, ex(pl), ex(pl_inv)], 2), "weight_fc1"))
        w = lin(torch.cat([w, ex(pl), ex(pl_inv)], 2), "weight_fc2").squeeze(-1)
    p = p[:, 0, :]
    g = agg(g)
    y = act(lin(torch.cat([p, g, g - p, g * p, pl, gl, pl_inv, gl_inv], 1), "pred_fc1"))
    y = lin(torch.cat([y, pl, gl, pl_inv, gl_inv], 1), "pred_fc2")
    return y, w


def loss_coef(B, dtype, device="cpu"):
    """The weights of pred_c in the goldens' loss: (1..B) / B."""
    return torch.arange(1, B + 1, dtype=dtype, device=device).view(-1, 1) / B


def forward_outside_reps(sd, cfg, p, g, p_rep, g_rep, coef_v=None):
    """Everything GraphAdjModel.forward computes around the rep nets, given the rep outputs.  Returns a dict with gate,
    p_v_emb, g_v_emb, p_v_mask, g_v_mask, pred_c, pred_v, and grad_p_rep / grad_g_rep / pred_grads under
    loss = sum(pred_c * (1..B) / B) (+ sum(pred_v * coef_v)), the loss the goldens use."""
    add_id = cfg.get("add_node_id", cfg.get("gnn_add_node_id", False))
    res = {"gate": gate(p, g) if cfg.get("filter_net", "None") == "ScalarFilter" else None,
           "p_v_emb": embed(sd, "p", p, add_id), "g_v_emb": embed(sd, "g", g, add_id),
           "p_v_mask": pad_mask(p["sizes"], p["dummy"]), "g_v_mask": pad_mask(g["sizes"], g["dummy"])}
    pr = torch.as_tensor(p_rep).detach().double().requires_grad_(True)
    gr = torch.as_tensor(g_rep).detach().double().requires_grad_(True)
    outs = []
    for side, d, rep, mask in (("p", p, pr, res["p_v_mask"]), ("g", g, gr, res["g_v_mask"])):
        rows = pad_rows(node_rows(sd, cfg, side, d, rep), d["sizes"])
        outs.append(rows.masked_fill(~mask.unsqueeze(-1), 0.0))
    W = pred_params(sd)
    y, w = head(W, cfg, outs[0], res["p_v_mask"], outs[1], res["g_v_mask"])
    B = y.shape[0]
    loss = (y * loss_coef(B, torch.float64)).sum()
    if w is not None and coef_v is not None:
        loss = loss + (w * torch.as_tensor(coef_v).double()).sum()
    loss.backward()
    res.update(pred_c=y.detach(), pred_v=None if w is None else w.detach(), grad_p_rep=pr.grad, grad_g_rep=gr.grad,
               pred_grads={"pred_net." + k: v.grad for k, v in W.items()})
    return res
