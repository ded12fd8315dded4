"""Float64 restatement of one HGT layer (subgraph_isomorphism/models/hgt.py:18-364) on plain edge lists.

Written from the reference's formulas as it states them -- a [d_k, d_k] matrix gathered per edge and head for the logit and for
the message, a softmax over the in-edges of every destination -- on CPU tensors, so autograd gives the gradients.
tests/test_hgt_host.py pins it against the layer goldens the reference itself produced (tests/golden/si_hgt.npz); the GPU tests
then use it as the reference for shapes the goldens do not reach."""
import json
import os

import numpy as np
import torch

from si_model_ref import OUT_KEYS, batch, loss_coef, rel_max, state_dict  # noqa: F401  (the golden layout is si_models.npz's)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "si_hgt.npz")
LEAKY_SLOPE = 1 / 5.5
ACTS = {"relu": torch.relu, "leaky_relu": lambda x: torch.nn.functional.leaky_relu(x, LEAKY_SLOPE), "none": lambda x: x}


def load_golden():
    """{case name: meta dict with "arrays" = {name: np.ndarray}} of si_hgt.npz (model and layer cases)."""
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


def effective_regularizer(regularizer, num_bases):
    """DecompMultiTransform.__init__ (hgt.py:22-25): num_bases <= 0 means no decomposition whatever the name says."""
    return "none" if num_bases <= 0 else regularizer


def decomp_apply(regularizer, num_bases, W, x, xtype, in_dim, out_dim):
    """DecompMultiTransform.forward (hgt.py:46-111) for integer types: W = {"weight": ..., ("w_comp": ...)}, x [n, in], xtype [n]."""
    reg = effective_regularizer(regularizer, num_bases)
    n = x.shape[0]
    if reg == "none":
        return torch.bmm(x.view(n, 1, in_dim), W["weight"][xtype].view(n, in_dim, out_dim)).view(n, out_dim)
    if reg == "basis":
        w = torch.matmul(W["w_comp"], W["weight"])[xtype].view(n, in_dim, out_dim)
        return torch.bmm(x.view(n, 1, in_dim), w).view(n, out_dim)
    if reg == "bdd":
        si, so = in_dim // num_bases, out_dim // num_bases
        w = W["weight"][xtype].view(-1, si, so)
        return torch.bmm(x.reshape(-1, 1, si), w).view(n, out_dim)
    w = torch.matmul(W["w_comp"][xtype], W["weight"])                            # diag: [n, in]; scalar: [n, 1]
    return x * w.view(n, -1)


def edge_softmax(logit, dst, num_nodes):
    """Softmax over the edges that share a destination, per trailing dimension (max subtracted)."""
    idx = dst.view(-1, *([1] * (logit.dim() - 1))).expand_as(logit)
    mx = torch.full((num_nodes,) + tuple(logit.shape[1:]), float("-inf"), dtype=logit.dtype)
    mx = mx.scatter_reduce(0, idx, logit.detach(), "amax", include_self=True)
    p = torch.exp(logit - mx[dst])
    sm = torch.zeros((num_nodes,) + tuple(logit.shape[1:]), dtype=logit.dtype).index_add(0, dst, p)
    return p / sm[dst]


def attention(q, k, v, att, msg, pri, scale, src, dst, et):
    """agg [N, H] of hgt.py:252-264, 324-333: q, k, v [N, H]; att, msg [R, heads, d_k, d_k]; pri [R, heads]; src, dst, et int64 [E].
    Returns (agg, a [E, heads])."""
    N, H = q.shape
    heads, dk = att.shape[1], att.shape[2]
    qh, kh, vh = (t.view(N, heads, dk) for t in (q, k, v))
    e = (qh[dst] * torch.einsum("bij,bijk->bik", kh[src], att[et])).sum(-1) * pri[et] * scale
    a = edge_softmax(e, dst, N)
    m = a.unsqueeze(-1) * torch.einsum("bij,bijk->bik", vh[src], msg[et])
    agg = torch.zeros((N, heads, dk), dtype=q.dtype).index_add(0, dst, m)
    return agg.view(N, H), a


def layer(P, kw, dims, src, dst, et, ntype, x, training=True):
    """HeteroGraphTransLayer.forward.  P: {state_dict key: float64 tensor} (leaves wanting gradients marked by the caller); kw: the
    layer's keyword arguments; dims: {"H", "T", "R"}."""
    H = dims["H"]
    reg, nb = kw.get("regularizer", "basis"), kw.get("num_bases", -1)
    heads = kw.get("num_heads", 1)

    def tr(name):
        W = {k.split(".")[-1]: t for k, t in P.items() if k.startswith(name + ".weights.")}
        return decomp_apply(reg, nb, W, x, ntype, H, H)

    k, v, q = tr("k_transform"), tr("v_transform"), tr("q_transform")
    scale = (H / heads) ** -0.5
    out, _ = attention(q, k, v, P["relation_att"], P["relation_msg"], P["relation_pri"], scale, src, dst, et)
    if kw.get("self_loop", True):
        out = out + x @ P["loop_weight"]
    if kw.get("bias", True):
        out = out + P["bias"]
    if kw.get("batch_norm", False):
        if training:
            mean, var = out.mean(0), out.var(0, unbiased=False)
        else:
            mean, var = P["bn.running_mean"], P["bn.running_var"]
        out = (out - mean) / torch.sqrt(var + 1e-5) * P["bn.weight"] + P["bn.bias"]
    return ACTS[kw.get("act_func", "relu")](out)


def run_layer_case(case):
    """The layer golden `case` restated: (out, grad of x, {parameter: grad or None})."""
    a = case["arrays"]
    P = {}
    for key in case["keys"]:
        t = torch.from_numpy(np.array(a["param/" + key]))
        P[key] = t.double().requires_grad_(True) if key in case["params"] else t
    x = torch.from_numpy(np.array(a["in/x"])).double().requires_grad_(True)
    src, dst, et, nt = (torch.from_numpy(np.asarray(a["g/" + key], np.int64)) for key in ("u", "v", "elabel", "label"))
    y = layer(P, case["kw"], case["dims"], src, dst, et, nt, x)
    (y * torch.from_numpy(np.array(a["in/coef"])).double()).sum().backward()
    return y.detach(), x.grad, {key: P[key].grad for key in case["params"]}


# ------------------------------------------------------------------------------------------------ the shift in front of a BatchNorm
def bn_shift(case, k):
    """Is parameter k a layer's `bias` with a BatchNorm behind it (hgt.py:299-302)?  Its true gradient is zero -- the norm subtracts
    the batch mean -- and the reference's value is rounding noise (~1e-7 next to weight gradients of ~1), so a bound relative to it
    says nothing: such a gradient is held to |grad| < 1e-4 * the largest weight gradient of its layer, as tests/dmplrp_ref.bn_shift
    and tests/si_dual_model_ref.bn_shift hold the same kind of parameter."""
    bn = case["kw"].get("batch_norm", False) if case["kind"] == "layer" else case["cfg"].get("rep_hgt_batch_norm", False)
    return bool(bn) and (k == "bias" or k.endswith(").bias"))


def layer_weight_grad_scale(case, k):
    """Largest golden gradient magnitude over the weights of the layer that holds parameter k."""
    prefix = k[:k.index(").") + 2] if ")." in k else ""
    a = case["arrays"]
    return max(float(np.abs(a["grad/" + n]).max()) for n in case["params"]
               if n.startswith(prefix) and n.endswith("weight") and "grad/" + n in a)


def grad_error(case, k, got):
    """The error of a parameter gradient against the golden, as a fraction of the scale it is held to (see bn_shift)."""
    if bn_shift(case, k):
        return float(torch.as_tensor(got).detach().double().abs().max()) / layer_weight_grad_scale(case, k)
    return rel_max(got, case["arrays"]["grad/" + k])
