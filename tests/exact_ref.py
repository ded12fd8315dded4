"""Operands on which every kernel's arithmetic is exact, and the references they are compared with bit for bit (test infrastructure
only; not a conftest).

Every operand is an integer sized so that each product and each partial sum a GPU path can form -- in any summation
order, launch split, chunking, at any storage point -- is exactly representable where it is held:
  * bf16 storage (Y rows, slot / aux sums, h, h1, h2, g1, g0, the input gradient): |value| <= 256 q (BF16_LIMIT quanta);
  * fp32 accumulation (weight gradients, column sums, fp32 layers): |value| < 2^24 q (F32_LIMIT quanta); a final bf16 output then equals
    the exact value rounded once (round to nearest even, ``.to(torch.bfloat16)``);
  where q is the quantum of the terms summed (``quantum()``): 1 forward, 1/16 for gradients behind two leaky-ReLU masks at 0.25;
  * fp32 products on the 3-term bf16 split (hi*hi + hi*lo + lo*hi, lo*lo dropped): every operand of a product holds at most 16
    significant bits and the weights / upstream gradients at most 8 (bf16-exact), so the dropped term is 0 -- the pre-aggregated rows
    of the collapsed relations included (sums of gradient rows are a product's narrow operand in the weight gradient).
layer_bounds() evaluates the same stages on absolute values (|operands|, no activation, |coef|): every partial sum of every stage is
bounded by its entry there, which check_premise() holds to the limits above before a test compares anything."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import layers as OL

BF16_LIMIT = 256
F32_LIMIT = 2 ** 24


class PremiseError(AssertionError):
    """The operands of a test are not exact by construction: a fault of the test, not of the kernel under test."""


# ---- generators ------------------------------------------------------------------------------------------------------------------
def sparse_rows(rng, n, h, nnz=2, max_exp=1, scale=1):
    """[n, h] float64 rows with `nnz` nonzeros each, +-2^k * scale, k in 0..max_exp (columns may repeat: sums of two)."""
    out = np.zeros((n, h))
    if n and nnz:
        r = np.repeat(np.arange(n), nnz)
        c = rng.integers(0, h, size=n * nnz)
        v = rng.choice([-1.0, 1.0], size=n * nnz) * 2.0 ** rng.integers(0, max_exp + 1, size=n * nnz) * scale
        np.add.at(out, (r, c), v)
    return torch.from_numpy(out)


def split_rows(rng, n, h, nnz=2, scale=16):
    """fp32 rows for the bf16-split mode: +-scale * (2^a + c), a in {8, 9}, c in 1..15 -- 9 or 10 significant bits, so the lo plane of
    the split carries data (271 = hi 272 + lo -1), and sums of up to 2^6 of them stay within 16 significant bits (multiples of scale)."""
    out = np.zeros((n, h))
    if n and nnz:
        r = np.repeat(np.arange(n), nnz)
        c = rng.integers(0, h, size=n * nnz)
        v = rng.choice([-1.0, 1.0], size=n * nnz) * scale * (2.0 ** rng.integers(8, 10, size=n * nnz) + rng.integers(1, 16, size=n * nnz))
        np.add.at(out, (r, c), v)
    return torch.from_numpy(out)


def signed_weight(rng, k, n, s=1):
    """[k, n] float64 with s nonzero +-1 entries per column in distinct rows; s = 1 and k == n: a random signed permutation (not
    symmetric, so a transposed tile shows)."""
    w = np.zeros((k, n))
    for j in range(n):
        rows = rng.permutation(k)[:s] if s < k else np.arange(k)
        w[rows, j] = rng.choice([-1.0, 1.0], size=len(rows))
    if s == 1 and k == n:                                 # a true permutation: one nonzero per row as well
        p = rng.permutation(k)
        w = np.zeros((k, n))
        w[p, np.arange(n)] = rng.choice([-1.0, 1.0], size=n)
    return torch.from_numpy(w)


def small_ints(rng, *shape, lo=-2, hi=2):
    return torch.from_numpy(rng.integers(lo, hi + 1, size=shape).astype(np.float64))


def tri_coef(rng, n, h):
    """upstream gradients in {-1, 0, 1}"""
    return small_ints(rng, n, h, lo=-1, hi=1)


def layer_params(rng, H, R, num_mlp_layers=2, self_loop=True, regularizer="basis", num_bases=-1, s=1):
    """float64 parameters of an RGINLayer(H, H) under the layer's own names (state_dict keys)."""
    p = {}
    if self_loop:
        p["loop_weight"] = signed_weight(rng, H, H, s)
    p["bias"] = small_ints(rng, H, lo=-1, hi=1)
    for i in range(num_mlp_layers):
        p["mlp.%d.weight" % (2 * i)] = signed_weight(rng, H, H, 1)
        p["mlp.%d.bias" % (2 * i)] = small_ints(rng, H, lo=-1, hi=1)
    B = R if regularizer == "none" or num_bases is None or num_bases > R or num_bases <= 0 else num_bases
    if regularizer in ("none", "basis"):
        p["weight"] = torch.stack([signed_weight(rng, H, H, s) for _ in range(B)])
        if B < R:
            wc = np.zeros((R, B))
            for r in range(R):
                wc[r, rng.integers(0, B)] = rng.choice([-1.0, 1.0])
            p["w_comp"] = torch.from_numpy(wc)
    else:
        si = H // B
        p["weight"] = torch.stack([torch.stack([signed_weight(rng, si, si, s) for _ in range(B)]).reshape(-1) for _ in range(R)])
    return p


def load_params(layer, p):
    """Copy float64 parameters into a module (in its dtype and device; they are exact there)."""
    with torch.no_grad():
        for k, v in layer.named_parameters():
            assert k in p, k
            v.copy_(p[k].to(v.dtype))


# ---- the references --------------------------------------------------------------------------------------------------------------
def _act(name, slope):
    if name == "none":
        return lambda t: t
    if name == "relu":
        return F.relu
    return lambda t: F.leaky_relu(t, slope)


def rgin_ref(x, src, dst, et, p, num_rels, regularizer="basis", num_bases=-1, num_mlp_layers=2, act="relu", slope=0.0, stages=None):
    """RGIN layer (rgin.py:102-160) restated per relation: h = sum_r index_add(x[src_r] @ W_r) + x @ W_loop + bias, then the MLP and
    the activations as oracle.layers.rgin_layer orders them -- without its [E, H, H] weight gather, so it runs on config-5-sized
    batches (on any device).  stages: a dict that receives every intermediate (h, z_i, a_i; 'agg': sum by destination of the source
    rows, the pre-aggregated rows of the collapsed relations)."""
    H = x.shape[1]
    B = num_rels if regularizer == "none" or num_bases is None or num_bases > num_rels or num_bases <= 0 else num_bases
    if regularizer == "bdd":
        W = OL.relation_weights(p["weight"].cpu(), None, "bdd", num_rels, B, H, H).to(x.device)
    else:
        W = OL.relation_weights(p["weight"], p.get("w_comp"), regularizer, num_rels, B, H, H)
    f = _act(act, slope)
    h = x @ p["loop_weight"] if p.get("loop_weight") is not None else x.new_zeros(x.shape[0], W.shape[2])
    for r in range(num_rels):
        e = (et == r).nonzero().reshape(-1)
        if e.numel():
            h = h.index_add(0, dst[e], x[src[e]] @ W[r])
    if p.get("bias") is not None:
        h = h + p["bias"]
    st = {"h": h}
    if stages is not None:
        st["agg"] = x.new_zeros(x.shape).index_add(0, dst, x[src])
    out = h
    for i in range(num_mlp_layers):
        out = F.linear(out, p["mlp.%d.weight" % (2 * i)], p["mlp.%d.bias" % (2 * i)])
        st["z%d" % i] = out
        if i != num_mlp_layers - 1:
            out = f(out)
            st["a%d" % i] = out
    if num_mlp_layers == 0:
        out = f(out)
        st["a"] = out
    out = f(out)
    if stages is not None:
        for k, v in st.items():
            if v.requires_grad:
                v.retain_grad()
        stages.update(st)
    return out


def leaf(t, device=None, dtype=torch.float64):
    return t.detach().to(device=device, dtype=dtype).clone().requires_grad_(True)


def layer_bounds(x, src, dst, et, p, num_rels, coef, regularizer="basis", num_bases=-1, num_mlp_layers=2):
    """The layer's stages on |operands| with no activation and |coef|: {stage: tensor} bounds every partial sum of the stage, forward
    ('h', 'z0', ..., 'agg') and backward ('g:<stage>' the gradient reaching it, 'g:x', 'g:<parameter>'; 'gagg': sum by source of the
    gradient rows reaching h, the backward's pre-aggregated rows)."""
    xa = leaf(x.abs(), x.device)
    pa = {k: leaf(v.abs(), v.device) for k, v in p.items()}
    st = {}
    out = rgin_ref(xa, src, dst, et, pa, num_rels, regularizer, num_bases, num_mlp_layers, act="none", stages=st)
    out.backward(coef.abs().to(out.dtype))
    b = {k: v.detach() for k, v in st.items()}
    b["out"] = out.detach()
    for k, v in st.items():
        if v.grad is not None:
            b["g:" + k] = v.grad.detach()
    b["g:x"] = xa.grad.detach()
    for k, v in pa.items():
        b["g:" + k] = v.grad.detach()
    gh = b["g:h"]
    b["gagg"] = gh.new_zeros(gh.shape).index_add(0, src, gh[dst])
    return b


def _is_param_grad(k):
    return k.startswith("g:") and k[2:] not in ("x", "h", "agg", "a") and not k[2:].startswith(("z", "a"))


def check_premise(bounds, storage="bf16", split_operands=(), q_fwd=1.0, q_bwd=1.0):
    """Hold the bounds to the representation limits, in units of the quantum of the terms summed: forward stages (multiples of q_fwd),
    backward stages ('g:' of a stage, 'g:x', 'gagg'; multiples of q_bwd -- 1/16 behind two leaky-ReLU masks at slope 0.25) and parameter
    gradients (products of the two: multiples of q_fwd q_bwd).  'bf16': every stored stage within 256 quanta, every fp32 accumulation
    (parameter gradients) below 2^24 quanta; 'f32': everything below 2^24 quanta.  split_operands: tensors that enter products on the
    bf16 split as the wider operand (at most 16 significant bits each).  Raises PremiseError."""
    worst = {}
    for k, v in bounds.items():
        m = float(v.abs().max()) if v.numel() else 0.0
        if _is_param_grad(k):
            q, units = q_fwd * q_bwd, F32_LIMIT - 1
        else:
            q = q_bwd if (k.startswith("g:") or k == "gagg") else q_fwd
            units = BF16_LIMIT if storage == "bf16" else F32_LIMIT - 1
        worst[k] = m
        if not m <= units * q:
            raise PremiseError("operand construction is not exact: stage %s reaches %g (limit %g = %g quanta of %g)" % (
                k, m, units * q, units, q))
    for i, t in enumerate(split_operands):
        if sig_bits(t) > 16:
            raise PremiseError("operand %d of a split product holds %d significant bits (at most 16)" % (i, sig_bits(t)))
    return worst


def _low_bits(t):
    """(exponent of the leading bit, exponent of the lowest set bit) of every nonzero element of a tensor (vectorised, on its device)."""
    a = t.detach().double().abs().reshape(-1)
    a = a[a != 0]
    m, e = torch.frexp(a)                                 # a = m 2^e, m in [0.5, 1): m 2^53 is an integer of 53 bits
    q = (m * 2.0 ** 53).to(torch.int64)
    low = torch.log2((q & -q).double()).to(torch.int64)   # the lowest set bit of the mantissa
    return (e - 1).cpu().numpy(), (e - 53 + low).cpu().numpy()


def sig_bits(t):
    """Largest number of significant bits of an element of a tensor (fractions included: 3.25 = 13 / 4 holds 4; 0 for all zeros)."""
    hi, lo = _low_bits(t)
    return int(np.max(hi - lo + 1)) if hi.size else 0


def quantum(*ts):
    """The largest power of two that divides every element of the tensors (1 for all zeros): 1/16 for gradients that crossed two
    leaky-ReLU masks at slope 0.25."""
    lows = [int(lo.min()) for lo in (_low_bits(t)[1] for t in ts) if lo.size]
    return 2.0 ** min(lows) if lows else 1.0


def linear_bounds(x, w, b, g):
    """|operands| of y = x @ w^T + b and its backward with |g|: {'y', 'g:x' (stored stages), 'g:weight', 'g:bias' (accumulations)}."""
    xa, wa, ga = x.abs().double(), w.abs().double(), g.abs().double()
    out = {"y": xa @ wa.t() + (b.abs().double() if b is not None else 0.0), "g:x": ga @ wa, "g:weight": ga.t() @ xa}
    out["g:bias"] = ga.sum(0)
    return out


def per_relation_linear(x, W, rel_ptr, transpose_w=False, bias=None):
    """Y[rows of relation r] = x[rows] @ W[r] (or W[r]^T) (+ bias[r]) in float64: the any-width product's reference."""
    out = []
    for r in range(len(rel_ptr) - 1):
        a, b = int(rel_ptr[r]), int(rel_ptr[r + 1])
        w = W[r].t() if transpose_w else W[r]
        y = x[a:b].double() @ w.double()
        if bias is not None:
            y = y + bias[r].double()
        out.append(y)
    return torch.cat(out, 0)


# ---- the comparison --------------------------------------------------------------------------------------------------------------
def assert_bits(got, ref, what, rel=None, graph=None, pos=None):
    """got must equal ref (float64, exact) rounded once to got's dtype, bit for bit.  On a mismatch: the count of wrong elements and the
    first one's (row, column), with the row's relation / graph / index position when given ([rows] tensors)."""
    got = got.detach()
    want = ref.detach().to(device=got.device, dtype=got.dtype)
    assert got.shape == want.shape, "%s: shape %s, want %s" % (what, tuple(got.shape), tuple(want.shape))
    if torch.equal(got, want):
        return
    bad = got != want
    if got.is_floating_point():
        bad = bad & ~(torch.isnan(got) & torch.isnan(want))
    idx = bad.nonzero()
    n = int(idx.shape[0])
    if n == 0:
        return
    first = tuple(int(i) for i in idx[0])
    msg = "%s: %d of %d elements differ; first at %s: got %r, want %r" % (
        what, n, got.numel(), first, float(got[first]), float(want[first]))
    row = first[0]
    for name, t in (("relation", rel), ("graph", graph), ("index position", pos)):
        if t is not None and row < len(t):
            msg += ", %s %d" % (name, int(t[row]))
    rows = torch.unique(idx[:, 0]).tolist()
    msg += "; rows %s%s" % (rows[:8], " ..." if len(rows) > 8 else "")
    raise AssertionError(msg)


# ---- batches ---------------------------------------------------------------------------------------------------------------------
def si_batch(rng, G, R, nmax, dens, dummy=True, nmin=1):
    """SI-shaped batch: graphs of nmin .. nmax real nodes, multi-edges and self loops, real relations 0 .. R-3 (+ the dummy node
    with relations R-2 / R-1 when dummy).  -> (src, dst, etype, node_ptr, edge_ptr) int64 numpy."""
    src, dst, et, nptr, eptr = [], [], [], [0], [0]
    for _ in range(G):
        n = int(rng.integers(nmin, nmax + 1))
        base = nptr[-1]
        m = int(rng.integers(0, max(1, int(dens * n)) + 1)) if n and dens > 0 else 0
        if m:
            src += list(base + rng.integers(0, n, size=m))
            dst += list(base + rng.integers(0, n, size=m))
            et += list(rng.integers(0, max(1, R - 2 if dummy else R), size=m))
        if dummy and n:
            src += list(base + np.arange(n)) + [base + n] * n
            dst += [base + n] * n + list(base + np.arange(n))
            et += [R - 2] * n + [R - 1] * n
            n += 1
        nptr.append(base + n)
        eptr.append(len(src))
    a = lambda v: np.asarray(v, dtype=np.int64)  # noqa: E731
    return a(src), a(dst), a(et), a(nptr), a(eptr)


def limit_graph(rng, nodes=64, rel_sizes=None):
    """One graph at the whole-graph launch's limits: `nodes` nodes, relation r holding rel_sizes[r] edges (default: 1,024 edges over 16
    relations, 15 buckets of 65 = 2 x 32 + 1 and one of 49 -- padding each bucket to a multiple of 32 adds 31 rows to most)."""
    if rel_sizes is None:
        rel_sizes = [65] * 15 + [49]
    et = np.concatenate([np.full(k, r, dtype=np.int64) for r, k in enumerate(rel_sizes)])
    et = et[rng.permutation(len(et))]
    src = rng.integers(0, nodes, size=len(et)).astype(np.int64)
    dst = rng.integers(0, nodes, size=len(et)).astype(np.int64)
    return src, dst, et, np.array([0, nodes], dtype=np.int64), np.array([0, len(et)], dtype=np.int64)


def concat_batches(*bs):
    """Disjoint union of (src, dst, etype, node_ptr, edge_ptr) batches."""
    src, dst, et, nptr, eptr = [], [], [], [0], [0]
    for s, d, t, np_, ep in bs:
        off = nptr[-1]
        src.append(s + off)
        dst.append(d + off)
        et.append(t)
        nptr += list(np_[1:] + off)
        eptr += list(ep[1:] + eptr[-1])
    return (np.concatenate(src), np.concatenate(dst), np.concatenate(et), np.asarray(nptr, dtype=np.int64),
            np.asarray(eptr, dtype=np.int64))
