"""Float64 restatements of the autograd operators whose backward branches on `needs_input_grad`, for every subset of their inputs
that requires a gradient (test infrastructure only; CPU tensors, plain torch, no HIP library, not a conftest).

A Case holds the float64 operands of ONE operator at one shape and dtype -- the exact-integer kinds of tests/exact_ref.py: sparse
integer rows, signed-permutation weights, small-integer biases, upstream gradients in {-1, 0, 1}, edge scales in {0.5, 1, 2},
split rows for fp32 on the bf16 split -- and restates the operator with index_add / F.linear / F.relu / F.leaky_relu.
  case.run(subset, used) -> (outputs, {input name: gradient or None}): the inputs named in `subset` are leaves that require a
      gradient, the others do not; `used`: which outputs feed the loss (all by default).
  case.premise(): on absolute values (|operands|, no activation, differences as sums), every stored value and every partial sum of
      forward and backward stays within 256 quanta where it is held in bf16 and below 2^24 quanta where it is held in fp32 (weight,
      bias and edge-scale gradients are fp32 accumulations whatever the dtype); on the bf16 split the wide operands hold at most 16
      significant bits and the narrow ones (weights, gradients) at most 8.  Raises exact_ref.PremiseError: a fault of the test.
tests/test_grad_subsets_premise.py proves the premises, the restatements (against per-edge / per-row Python loops) and the None
patterns (against torch.autograd's own) without a GPU; tests/test_gpu_grad_subsets.py then compares bits."""
import functools
import itertools

import numpy as np
import torch
import torch.nn.functional as F

import exact_ref as X
import gc_exact_ref as G
import rel_exact_ref as R

HUB_SPLIT = 64                    # ops.HUB_SPLIT (the GPU tests assert it): lists longer than this are summed in chunks
DUAL_EDGE, DUAL_SUB, DUAL_MULT = 0, 1, 2          # ops.DUAL_* (asserted there too)
DTYPES = {"bf16": torch.bfloat16, "f32": torch.float32, "f32x": torch.float32, "f32s": torch.float32}


def subsets(names, which="all"):
    """Non-empty subsets of `names` in a fixed order; which = 'all': every one; 'singles': all, each input alone, each input left
    out (five inputs: 11); 'first': all, and all but the first input."""
    names = tuple(names)
    if which == "all":
        return [s for k in range(len(names), 0, -1) for s in itertools.combinations(names, k)]
    if which == "first":
        return [names, names[1:]]
    out = [names] + [(n,) for n in names] + [tuple(m for m in names if m != n) for n in names]
    return list(dict.fromkeys(out))


def run_order(subs):
    """all inputs, every proper subset, all inputs again: a subset run must leave nothing behind that the last run reads"""
    return [subs[0]] + list(subs[1:]) + [subs[0]]


class Case:
    """One operator, one shape, one dtype.  ins: {name: float64 tensor} of the differentiable inputs in the operator's argument order;
    params: the inputs whose gradient is an fp32 accumulation; coefs: the upstream gradient of every output; in_dtype: inputs held in
    another dtype than the case's (an fp32 edge scale beside bf16 rows)."""
    params = ()
    in_dtype = {}

    def __init__(self, what, mode, ins, coefs):
        self.what, self.mode, self.ins, self.coefs = what, mode, dict(ins), tuple(coefs)
        self.dtype = DTYPES[mode]
        self.split = mode == "f32s"

    @property
    def names(self):
        return tuple(self.ins)

    def fn(self, t, absolute=False, st=None):
        """-> tuple of outputs.  absolute: the bound's form (no activation, sums for differences); st: receives the stored stages."""
        raise NotImplementedError

    @staticmethod
    def _stage(st, k, v):
        if st is not None:
            if v.requires_grad:
                v.retain_grad()
            st[k] = v
        return v

    def run(self, subset=None, used=None):
        subset = self.names if subset is None else tuple(subset)
        used = tuple(range(len(self.coefs))) if used is None else tuple(used)
        leaves = {k: v.detach().clone().requires_grad_(k in subset) for k, v in self.ins.items()}
        outs = self.fn(leaves)
        grads = torch.autograd.grad([outs[i] for i in used], [leaves[k] for k in subset], [self.coefs[i] for i in used],
                                    allow_unused=True)
        got = dict.fromkeys(self.names)
        got.update(zip(subset, grads))
        return tuple(o.detach() for o in outs), got

    def none_pattern(self, subset, used=None):
        """{name: is the gradient None} as torch.autograd's own .backward() leaves it on the leaves"""
        used = tuple(range(len(self.coefs))) if used is None else tuple(used)
        leaves = {k: v.detach().clone().requires_grad_(k in subset) for k, v in self.ins.items()}
        outs = self.fn(leaves)
        torch.autograd.backward([outs[i] for i in used], [self.coefs[i] for i in used])
        return {k: v.grad is None for k, v in leaves.items()}

    def premise(self):
        """-> {stage: bound in its quanta}; raises exact_ref.PremiseError"""
        st = {}
        leaves = {k: X.leaf(v) for k, v in self.ins.items()}
        outs = self.fn(leaves, st=st)
        torch.autograd.backward(list(outs), list(self.coefs))
        rows = [k for k in self.names if k not in self.params]
        fwd = [v.detach() for v in self.ins.values()] + [v.detach() for v in st.values()] + [o.detach() for o in outs]
        bwd = list(self.coefs) + [v.grad for v in st.values() if v.grad is not None] + [leaves[k].grad for k in rows]
        q_f, q_b = X.quantum(*fwd), X.quantum(*bwd)
        sa = {}
        la = {k: X.leaf(v.abs()) for k, v in self.ins.items()}
        oa = self.fn(la, absolute=True, st=sa)
        torch.autograd.backward(list(oa), [c.abs() for c in self.coefs])
        lim = X.BF16_LIMIT if self.dtype == torch.bfloat16 else X.F32_LIMIT - 1
        bounds = []
        for k, v in list(la.items()) + list(sa.items()) + [("out%d" % i, o) for i, o in enumerate(oa)]:
            bounds.append((k, v.detach(), lim if self.in_dtype.get(k) is None else X.F32_LIMIT - 1, q_f))
        for k, v in sa.items():
            if v.grad is not None:
                bounds.append(("g:" + k, v.grad, lim, q_b))
        for k in self.names:
            bounds.append(("g:" + k, la[k].grad, X.F32_LIMIT - 1 if k in self.params else lim, q_f * q_b if k in self.params else q_b))
        worst = {}
        for k, v, units, q in bounds:
            m = float(v.abs().max()) if v.numel() else 0.0
            worst[k] = m / q
            if not m <= units * q:
                raise X.PremiseError("%s: stage %s reaches %g (limit %g = %g quanta of %g)" % (self.what, k, m, units * q, units, q))
        # every reference value is representable where the operator stores it (the comparison rounds the reference ONCE)
        for k, v in [(k, leaves[k].grad) for k in rows] + [("out%d" % i, o.detach()) for i, o in enumerate(outs)]:
            if not torch.equal(v.to(self.dtype).double(), v):
                raise X.PremiseError("%s: %s is not representable in %s" % (self.what, k, self.dtype))
        if self.split:
            wide = [v.detach() for k, v in self.ins.items() if k in rows] + [v.detach() for v in st.values()]
            narrow = [v for k, v in self.ins.items() if k in self.params] + bwd
            for t in wide + list(self.split_wide(leaves, st)):
                if X.sig_bits(t) > 16:
                    raise X.PremiseError("%s: a split product's wide operand holds %d significant bits" % (self.what, X.sig_bits(t)))
            for t in narrow + list(self.split_narrow(leaves, st)):
                if X.sig_bits(t) > 8:
                    raise X.PremiseError("%s: a split product's narrow operand holds %d significant bits" % (self.what, X.sig_bits(t)))
            if max(X.sig_bits(self.ins[k]) for k in rows) <= 8:
                raise X.PremiseError("%s: the lo plane of the split carries no data" % self.what)
        self.extra_premise()
        return worst

    def split_wide(self, leaves, st):
        return ()

    def split_narrow(self, leaves, st):
        return ()

    def extra_premise(self):
        pass


def _rng(*key):
    return np.random.default_rng([int(k) for k in key])


def _act(t, relu, slope, absolute):
    if absolute or not relu:
        return t
    return F.relu(t) if slope == 0.0 else F.leaky_relu(t, slope)


def _rows(rng, n, h, mode, nnz=2, max_exp=1):
    return X.split_rows(rng, n, h, nnz) if mode == "f32s" else X.sparse_rows(rng, n, h, nnz, max_exp)


def _i64(a):
    return torch.from_numpy(np.asarray(a, dtype=np.int64))


def seg_sum(rows, idx, n):
    """out[s] = sum of the rows with idx == s (float64 index_add)"""
    return rows.new_zeros((n,) + tuple(rows.shape[1:])).index_add(0, idx, rows)


# ---- linear_act / relu_mlp / linear_any ------------------------------------------------------------------------------------------
class MlpCase(Case):
    """act(lin_L(... act(lin_1(x)))): ops.relu_mlp (every Linear followed by the activation); one Linear with relu True / False and an
    optional bias: ops.linear_act.  Inputs x, w0, b0, w1, b1, ...; weights [out, in] (nn.Linear layout)."""

    def __init__(self, rows, H, mode, layers=1, relu=True, slope=0.0, bias=True, seed=0):
        rng = _rng(41, rows, H, layers, int(relu), int(slope * 100), int(bias), list(DTYPES).index(mode), seed)
        small = layers >= 3 and slope != 0.0          # (outputs behind three leaky masks are multiples of 1 / 64: 256 quanta = 4)
        x = _rows(rng, rows, H, mode, nnz=1 if small else 2, max_exp=0 if small else 1)
        if rows > 1:
            x[torch.from_numpy(rng.random(rows) < 0.25)] = 0.0                   # rows whose pre-activations are the bias: ties at 0
        ins = {"x": x}
        for i in range(layers):
            ins["w%d" % i] = X.signed_weight(rng, H, H, 1)
            if bias:
                ins["b%d" % i] = X.small_ints(rng, H, lo=-1, hi=1)
        self.layers, self.relu, self.slope, self.bias, self.rows, self.H = layers, relu, float(slope), bias, rows, H
        self.params = tuple(k for k in ins if k != "x")
        # (behind leaky masks the weight gradients' quantum shrinks by 4 a mask: sparser upstream rows keep their sums below 2^24 quanta)
        coef = X.tri_coef(rng, rows, H) if slope == 0.0 else G.sparse_tri(rng, rows, H, 0.5)
        super().__init__("mlp rows=%d H=%d %s L=%d relu=%s slope=%g bias=%s" % (rows, H, mode, layers, relu, slope, bias), mode, ins,
                         [coef])

    def fn(self, t, absolute=False, st=None):
        out = t["x"]
        for i in range(self.layers):
            z = self._stage(st, "z%d" % i, F.linear(out, t["w%d" % i], t.get("b%d" % i)))
            out = _act(z, self.relu, self.slope, absolute)
            if i != self.layers - 1:
                self._stage(st, "a%d" % i, out)
        return (out,)

    def extra_premise(self):
        if self.relu and self.rows > 1:
            z = self.fn({k: v for k, v in self.ins.items()}, st=(st := {}))[0]
            if not bool((st["z0"] == 0).any()) or not bool((st["z0"] < 0).any()) or not bool((z > 0).any()):
                raise X.PremiseError("%s: the pre-activations show no tie at 0, or one sign only" % self.what)


def mlp_naive(c):
    """the same chain row by row, column by column (small cases)"""
    x = c.ins["x"]
    out = [[float(v) for v in row] for row in x]
    for i in range(c.layers):
        w, b = c.ins["w%d" % i], c.ins.get("b%d" % i)
        nxt = []
        for row in out:
            z = [sum(float(w[o, k]) * row[k] for k in range(len(row)) if float(w[o, k]) != 0.0) + (float(b[o]) if b is not None else 0.0)
                 for o in range(w.shape[0])]
            nxt.append([(v if v > 0 else c.slope * v) if c.relu else v for v in z])
        out = nxt
    return torch.tensor(out, dtype=torch.float64)


class LinearAnyCase(Case):
    """y = x @ weight^T + bias for any widths (ops.linear_any off the square matrix-core widths)"""
    params = ("weight", "bias")

    def __init__(self, rows, fin, fout, mode):
        rng = _rng(42, rows, fin, fout, list(DTYPES).index(mode))
        ins = {"x": X.sparse_rows(rng, rows, fin, nnz=2, max_exp=1), "weight": X.signed_weight(rng, fin, fout, min(2, fin)).t().contiguous(),
               "bias": X.small_ints(rng, fout, lo=-2, hi=2)}
        super().__init__("linear_any %d: %d -> %d %s" % (rows, fin, fout, mode), mode, ins, [G.sparse_tri(rng, rows, fout, 0.5)])

    def fn(self, t, absolute=False, st=None):
        return (F.linear(t["x"], t["weight"], t["bias"]),)


# ---- relu_bwd --------------------------------------------------------------------------------------------------------------------
RELU_BWD_NUMEL = (8, 8 * 255, 8 * 256 * 17)          # one lane, a partial workgroup, a grid-stride remainder


def relu_bwd_case(numel, slope, mode):
    """(g, y, want): g in {-2 .. 2}, y in {-1, 0, 1} (ties at 0 take the slope); want = where(y > 0, g, slope * g) -- exact: slope 0.25
    of a small integer"""
    rng = _rng(43, numel, int(slope * 100), list(DTYPES).index(mode))
    g, y = X.small_ints(rng, numel // 8, 8), X.small_ints(rng, numel // 8, 8, lo=-1, hi=1)
    want = torch.where(y > 0, g, slope * g)
    for v in (g, y, want):
        if not torch.equal(v.to(DTYPES[mode]).double(), v):
            raise X.PremiseError("relu_bwd: an operand is not representable in %s" % mode)
    if not (bool((y == 0).any()) and bool((y > 0).any()) and bool((y < 0).any())):
        raise X.PremiseError("relu_bwd: y lacks a sign or a tie")
    return g, y, want


# ---- the conv: rel_transform_fused and the RGIN layer functions --------------------------------------------------------------------
def conv_graph(hubs, N=300, R=3, seed=0):
    """(src, dst, etype) over N nodes and R = 3 relations.  hubs: relation 1 has every edge INTO node 0 (few distinct destinations: the
    row index collapses it forward) and relation 2 every edge OUT OF node 1 (collapsed backward) -- the hub recipe of
    tests/test_gpu_exact.py (limit_graph with one endpoint fixed).  Every other relation's edges have distinct sources and distinct
    destinations (one permutation each), so whatever share of distinct endpoints the index asks of a relation it keeps edge by
    edge, these have it: which relations collapse is read from the index, not from a threshold written down here."""
    rng = _rng(44, int(hubs), N, R, seed)
    src, dst, et, _, _ = X.limit_graph(rng, N, [200, 40, 40] if hubs else [120, 90, 70])
    for r in range(R):
        e = np.flatnonzero(et == r)
        src[e], dst[e] = rng.permutation(N)[:len(e)], rng.permutation(N)[:len(e)]
    if hubs:
        dst = np.where(et == 1, 0, dst)
        src = np.where(et == 2, 1, src)
    return src, dst, et


class ConvCase(Case):
    """out[v] = sum_{e -> v} x[src_e] W[etype_e] + x[v] W_loop + bias: ops.rel_transform_fused through exact_ref.rgin_ref without an
    MLP or activation.  Inputs x, W [R, H, H], W_loop [H, H], bias [H]."""
    params = ("W", "W_loop", "bias")

    def __init__(self, H, mode, hubs, N=300, R=3):
        rng = _rng(45, H, list(DTYPES).index(mode), int(hubs))
        self.src, self.dst, self.et = (_i64(a) for a in conv_graph(hubs, N, R))
        self.N, self.R, self.H, self.hubs = N, R, H, hubs
        x = _rows(rng, N, H, mode, nnz=1 if mode == "f32s" else 2)
        x[torch.from_numpy(rng.random(N) < 0.1)] = 0.0
        ins = {"x": x, "W": torch.stack([X.signed_weight(rng, H, H, 1) for _ in range(R)]), "W_loop": X.signed_weight(rng, H, H, 1),
               "bias": X.small_ints(rng, H, lo=-1, hi=1)}
        super().__init__("rel_transform_fused H=%d %s %s" % (H, mode, "hubs" if hubs else "no hubs"), mode, ins, [X.tri_coef(rng, N, H)])

    def fn(self, t, absolute=False, st=None):
        p = {"weight": t["W"], "loop_weight": t["W_loop"], "bias": t["bias"]}
        stages = {} if st is not None else None
        out = X.rgin_ref(t["x"], self.src, self.dst, self.et, p, self.R, regularizer="none", num_mlp_layers=0, act="none", stages=stages)
        if st is not None:
            st["agg"] = stages["agg"]
            # the pre-aggregated rows of the collapsed relations, per (endpoint, relation): sums of source rows forward ...
            self._stage(st, "agg_f", seg_sum(t["x"][self.src], self.dst * self.R + self.et, self.N * self.R))
        return (out,)

    def _agg_b(self):
        # ... and of the gradient rows reaching the output backward
        return seg_sum(self.coefs[0][self.dst], self.src * self.R + self.et, self.N * self.R)

    def split_narrow(self, leaves, st):
        return (self._agg_b(),)

    def extra_premise(self):
        lim = X.BF16_LIMIT if self.dtype == torch.bfloat16 else X.F32_LIMIT - 1
        b = seg_sum(self.coefs[0].abs()[self.dst], self.src * self.R + self.et, self.N * self.R)
        if float(b.max()) > lim:
            raise X.PremiseError("%s: the backward pre-aggregated rows reach %g" % (self.what, float(b.max())))
        if self.hubs and not (bool(self._agg_b()[1 * self.R + 2].any())):
            raise X.PremiseError("%s: the backward hub's pre-aggregated row is zero" % self.what)


def conv_naive(c):
    """the conv edge by edge"""
    x, W = c.ins["x"], c.ins["W"]
    out = x @ c.ins["W_loop"] + c.ins["bias"]
    for e in range(len(c.src)):
        out[int(c.dst[e])] += x[int(c.src[e])] @ W[int(c.et[e])]
    return out


class LayerCase(Case):
    """A whole RGIN layer (conv + bias + two Linears + activations) through exact_ref.rgin_ref: the layer functions
    ops.rgin_layer_f32 / _small / _wide / _chain.  Inputs x and the layer's parameters under their state_dict names."""

    def __init__(self, batch, H, R, mode, act="relu", nnz=2, s=1, coef_rows=1.0, seed=0):
        rng = _rng(46, H, R, list(DTYPES).index(mode), seed)
        src, dst, et, nptr, eptr = batch
        self.batch, self.H, self.R, self.act, self.slope = batch, H, R, act, (0.25 if act == "leaky_relu" else 0.0)
        self.src, self.dst, self.et, self.N = _i64(src), _i64(dst), _i64(et), int(nptr[-1])
        p = X.layer_params(rng, H, R, 2, True, "basis", -1, s)
        x = _rows(rng, self.N, H, mode, nnz, 0)
        x[torch.from_numpy(rng.random(self.N) < 0.25)] = 0.0
        coef = X.tri_coef(rng, self.N, H)
        coef[torch.from_numpy(rng.random(self.N) >= coef_rows)] = 0.0
        self.params = tuple(p)
        super().__init__("rgin layer H=%d R=%d %s %s" % (H, R, mode, act), mode, {"x": x, **p}, [coef])

    def fn(self, t, absolute=False, st=None):
        p = {k: v for k, v in t.items() if k != "x"}
        stages = {} if st is not None else None
        out = X.rgin_ref(t["x"], self.src, self.dst, self.et, p, self.R, act="none" if absolute else self.act, slope=self.slope,
                         stages=stages)
        if st is not None:
            st.update(stages)
            self._stage(st, "agg_f", seg_sum(t["x"][self.src], self.dst * self.R + self.et, self.N * self.R))
        return (out,)

    def split_narrow(self, leaves, st):
        gh = st["h"].grad
        return (seg_sum(gh[self.dst], self.src * self.R + self.et, self.N * self.R),)

    def premise(self):
        worst = super().premise()
        # the gradient rows reaching the conv's output, summed per (source, relation) and per graph: stored rows of the backward
        st = {}
        la = {k: X.leaf(v.abs()) for k, v in self.ins.items()}
        self.fn(la, absolute=True, st=st)[0].backward(self.coefs[0].abs())
        real = {}
        lr = {k: X.leaf(v) for k, v in self.ins.items()}
        self.fn(lr, st=real)[0].backward(self.coefs[0])
        q_b = X.quantum(self.coefs[0], *[v.grad for v in real.values() if v.grad is not None])
        nptr = self.batch[3]
        graph = _i64(np.repeat(np.arange(len(nptr) - 1), np.diff(nptr)))
        lim = X.BF16_LIMIT if self.dtype == torch.bfloat16 else X.F32_LIMIT - 1
        for k, v in (("gagg", seg_sum(st["h"].grad[self.dst], self.src * self.R + self.et, self.N * self.R)),
                     ("g1 per graph", seg_sum(st["z0"].grad, graph, len(nptr) - 1))):
            if float(v.max()) > lim * q_b:
                raise X.PremiseError("%s: %s reaches %g (limit %g)" % (self.what, k, float(v.max()), lim * q_b))
            worst[k] = float(v.max()) / q_b
        return worst


# ---- neighbor_sum ----------------------------------------------------------------------------------------------------------------
def hub_iso_graph(N=90, seed=0):
    """(src, dst): node 0 has HUB_SPLIT + 1 in-edges, node 1 HUB_SPLIT + 1 out-edges (both over the chunking threshold), node N - 1 is
    isolated, node N - 2 has no in-edge; duplicates and self loops among the rest."""
    rng = _rng(47, N, seed)
    src, dst = list(rng.integers(2, N - 2, size=150)), list(rng.integers(2, N - 2, size=150))
    src += list(rng.integers(2, N - 1, size=HUB_SPLIT + 1)) + [1] * (HUB_SPLIT + 1) + [5, 5, 6]
    dst += [0] * (HUB_SPLIT + 1) + list(rng.integers(2, N - 2, size=HUB_SPLIT + 1)) + [7, 7, 6]
    return np.asarray(src, np.int64), np.asarray(dst, np.int64)


class NeighborSumCase(Case):
    """out[v] = self_coef x[v] + sum_{e -> v} s_e x[src_e]: ops.neighbor_sum with an fp32 edge scale that takes a gradient
    (d s_e = <x[src_e], g[dst_e]>, fp32)."""
    params = ("edge_scale",)
    in_dtype = {"edge_scale": torch.float32}

    def __init__(self, H, mode, self_coef, N=90):
        rng = _rng(48, H, list(DTYPES).index(mode), int(self_coef))
        src, dst = hub_iso_graph(N)
        self.src, self.dst, self.N, self.H, self.self_coef = _i64(src), _i64(dst), N, H, float(self_coef)
        ins = {"x": X.sparse_rows(rng, N, H, nnz=1 if H < 16 else 2, max_exp=1),
               "edge_scale": torch.from_numpy(rng.choice([0.5, 1.0, 2.0], size=len(src)))}
        super().__init__("neighbor_sum H=%d %s self_coef=%g" % (H, mode, self_coef), mode, ins, [G.sparse_tri(rng, N, H, 0.5)])

    def fn(self, t, absolute=False, st=None):
        rows = t["x"][self.src] * t["edge_scale"].view(-1, 1)
        return (self.self_coef * t["x"] + seg_sum(rows, self.dst, self.N),)

    def extra_premise(self):
        indeg, outdeg = np.bincount(self.dst.numpy(), minlength=self.N), np.bincount(self.src.numpy(), minlength=self.N)
        if not (indeg[0] > HUB_SPLIT and outdeg[1] > HUB_SPLIT and indeg[-1] == 0 and outdeg[-1] == 0 and indeg[-2] == 0):
            raise X.PremiseError("%s: the graph lacks its hubs or its isolated node" % self.what)
        s = self.ins["edge_scale"]
        if len(set(s[self.dst == 0].tolist())) < 3:
            raise X.PremiseError("%s: the hub's edge scales do not differ" % self.what)


def neighbor_sum_naive(c):
    x, s = c.ins["x"], c.ins["edge_scale"]
    out = c.self_coef * x.clone()
    for e in range(len(c.src)):
        out[int(c.dst[e])] += float(s[e]) * x[int(c.src[e])]
    return out


def edge_dot_ref(c):
    """d edge_scale[e] = <x[src_e], g[dst_e]>"""
    return (c.ins["x"][c.src] * c.coefs[0][c.dst]).sum(1)


# ---- rel_agg_transform: rel_exact_ref.AggCase as a Case ---------------------------------------------------------------------------
class RelAggCase(Case):
    """ops.rel_agg_transform on the operands and the restatement (agg_ref) of rel_exact_ref.AggCase; its premise is AggCase's own."""
    params = ("W",)

    def __init__(self, fin, fout, mode, scaled):
        self.agg = a = R.agg_case(fin, fout, mode, scaled)
        self.src, self.dst, self.et = (_i64(v) for v in (a.src, a.dst, a.et))
        super().__init__(a.what, mode, {"x": a.x, "W": a.W}, [a.g])

    def fn(self, t, absolute=False, st=None):
        s = self.agg.scale.view(-1, 1) if self.agg.scale is not None else None
        return (R.agg_ref(t["x"], t["W"], self.src, self.dst, self.et, self.agg.N, s),)

    def premise(self):
        return self.agg.premise()


# ---- si_embed --------------------------------------------------------------------------------------------------------------------
class SiEmbedCase(Case):
    """emb[v] = enc1[key1_v] @ W1 + enc2[key2_v] @ W2 (ops.si_embed; the enc tables and keys take no gradient)"""
    params = ("W1", "W2")

    def __init__(self, N, H, mode, K=(7, 12), rows=(5, 40)):
        rng = _rng(49, N, H, list(DTYPES).index(mode))
        self.key = [_i64(rng.integers(0, r, size=N)) for r in rows]
        self.enc = [X.small_ints(rng, r, k, lo=0, hi=1) for r, k in zip(rows, K)]          # binary codes, as the models' are
        ins = {"W1": X.small_ints(rng, K[0], H), "W2": X.small_ints(rng, K[1], H)}
        super().__init__("si_embed N=%d H=%d %s" % (N, H, mode), mode, ins, [G.sparse_tri(rng, N, H, 0.5)])

    def fn(self, t, absolute=False, st=None):
        return (self.enc[0][self.key[0]] @ t["W1"] + self.enc[1][self.key[1]] @ t["W2"],)


def si_embed_naive(c):
    out = torch.zeros(len(c.key[0]), c.ins["W1"].shape[1], dtype=torch.float64)
    for v in range(out.shape[0]):
        for i, w in enumerate(("W1", "W2")):
            code = c.enc[i][int(c.key[i][v])]
            for k in range(len(code)):
                out[v] += float(code[k]) * c.ins[w][k]
    return out


# ---- the dual message pass: dual_agg, dmp_edge_update ------------------------------------------------------------------------------
def dual_graph(kind, N=40, seed=0):
    """(u, v, rev) of _graph_for_exact in tests/test_gpu_si_dual_model.py: a hub at node 0 on both sides -- 'below': of exactly
    HUB_SPLIT entries; 'above': HUB_SPLIT + 1, and a second hub of 2 HUB_SPLIT + 5 in-edges at node 1.  Nodes N - 3 .. N - 1 have
    no in-edges."""
    rng = _rng(50, ("below", "above").index(kind), N, seed)
    S = HUB_SPLIT
    u, v = list(rng.integers(0, N - 3, size=60)), list(rng.integers(1, N - 3, size=60))
    v = [int(t) if t != 0 else 1 for t in v]
    u = [int(t) if t != 0 else 1 for t in u]
    hub = S + 1 if kind == "above" else S
    u += list(rng.integers(1, N, size=hub)) + [0] * hub
    v += [0] * hub + list(rng.integers(1, N - 3, size=hub))
    if kind == "above":
        u += list(rng.integers(2, N, size=2 * S + 5))
        v += [1] * (2 * S + 5)
    u, v = np.array(u, np.int64), np.array(v, np.int64)
    return u, v, rng.integers(0, 2, size=len(u)).astype(bool)


class _DualCase(Case):
    def _graph(self, kind, N):
        u, v, rev = dual_graph(kind, N)
        self.kind, self.N, self.E = kind, N, len(u)
        self.u, self.v, self.rev = _i64(u), _i64(v), torch.from_numpy(rev)

    def extra_premise(self):
        indeg, outdeg = np.bincount(self.v.numpy(), minlength=self.N), np.bincount(self.u.numpy(), minlength=self.N)
        hub = HUB_SPLIT + (self.kind == "above")
        if not (indeg[0] == hub and outdeg[0] >= hub and (indeg[self.N - 3:] == 0).all()
                and bool(self.rev.any()) and not bool(self.rev.all())):
            raise X.PremiseError("%s: the graph lacks its hub, its nodes without in-edges or a direction" % self.what)


class DualAggCase(_DualCase):
    """(sum over the forward in-edges, sum over the reversed in-edges) of s_e m_e per destination; m_e = x[src_e] - ef_e (DUAL_SUB) or
    x[src_e] * ef_e (DUAL_MULT): ops.dual_agg with scales in {1, 2}.  Inputs ef [E, H], x [N, H]; two outputs."""

    def __init__(self, mode_op, kind, H, mode, N=40):
        rng = _rng(51, mode_op, ("below", "above").index(kind), H, list(DTYPES).index(mode))
        self._graph(kind, N)
        self.mode_op, self.H = mode_op, H
        ef = X.small_ints(rng, self.E, H, lo=-1, hi=1)
        ef[torch.arange(self.E) % 6 != 0] = 0.0
        x = X.small_ints(rng, N, H, lo=-1, hi=1)
        if mode_op == DUAL_SUB:
            x[torch.arange(N) % 8 != 0] = 0.0                       # (x - ef is non-zero wherever x is)
        self.scale = torch.from_numpy(rng.integers(1, 3, size=self.E).astype(np.float64))
        keep = (torch.arange(N) % 4 == 0).view(-1, 1)
        super().__init__("dual_agg mode=%d %s H=%d %s" % (mode_op, kind, H, mode), mode, {"ef": ef, "x": x},
                         [X.tri_coef(rng, N, H) * keep, X.tri_coef(rng, N, H) * keep])

    def fn(self, t, absolute=False, st=None):
        xs = t["x"][self.u]
        m = xs * t["ef"] if self.mode_op == DUAL_MULT else (xs + t["ef"] if absolute else xs - t["ef"])
        m = m * self.scale.view(-1, 1)
        return (seg_sum(m[~self.rev], self.v[~self.rev], self.N), seg_sum(m[self.rev], self.v[self.rev], self.N))


def dual_agg_naive(c):
    o = [torch.zeros(c.N, c.H, dtype=torch.float64) for _ in range(2)]
    for e in range(c.E):
        xs, ef = c.ins["x"][int(c.u[e])], c.ins["ef"][e]
        o[int(c.rev[e])][int(c.v[e])] += float(c.scale[e]) * (xs * ef if c.mode_op == DUAL_MULT else xs - ef)
    return tuple(o)


class DmpEdgeCase(_DualCase):
    """out[e] = p_loop[e] + coef[dst_e] p_diff[e] + xd[a_e] - xs[b_e] + ebias with (a, b) = (dst, src) of a forward edge and
    (src, dst) of a reversed one: ops.dmp_edge_update with the index's coefficient table replaced by small integers."""
    params = ("ebias",)

    def __init__(self, kind, H, mode, N=40):
        rng = _rng(52, ("below", "above").index(kind), H, list(DTYPES).index(mode))
        self._graph(kind, N)
        self.H = H
        self.coef = torch.from_numpy(rng.integers(1, 4, size=N).astype(np.float64))
        E = self.E
        ins = {"p_loop": X.small_ints(rng, E, H), "p_diff": X.small_ints(rng, E, H), "xd": X.small_ints(rng, N, H, lo=-3, hi=3),
               "xs": X.small_ints(rng, N, H, lo=-3, hi=3), "ebias": X.small_ints(rng, H)}
        g = X.tri_coef(rng, E, H)
        g[torch.arange(E) % 3 != 0] = 0.0                            # row sums over the longest lists stay within 256
        self.a, self.b = torch.where(self.rev, self.u, self.v), torch.where(self.rev, self.v, self.u)
        super().__init__("dmp_edge_update %s H=%d %s" % (kind, H, mode), mode, ins, [g])

    def fn(self, t, absolute=False, st=None):
        xs = t["xs"][self.b]
        return (t["p_loop"] + self.coef[self.v].view(-1, 1) * t["p_diff"] + t["xd"][self.a] + (xs if absolute else -xs) + t["ebias"],)


def dmp_edge_naive(c):
    out = torch.zeros(c.E, c.H, dtype=torch.float64)
    for e in range(c.E):
        u, v = int(c.u[e]), int(c.v[e])
        a, b = (u, v) if bool(c.rev[e]) else (v, u)
        out[e] = c.ins["p_loop"][e] + float(c.coef[v]) * c.ins["p_diff"][e] + c.ins["xd"][a] - c.ins["xs"][b] + c.ins["ebias"]
    return out


# ---- typed_linear, hgt_pair_expand, hgt_pair_reduce ------------------------------------------------------------------------------
def zoo(R_):
    """The 320-node graph of tests/test_gpu_hgt.py (_zoo): in-degrees 0, 1, 63, 64, 65 at nodes 0 - 4, a hub of 300 at node 5, 0 - 6
    elsewhere; the edge 7 -> 8 of type 0 twice, the self loop 9 -> 9."""
    rng = np.random.default_rng(50 + R_)
    N = 320
    deg = rng.integers(0, 7, size=N)
    deg[:6] = [0, 1, 63, 64, 65, 300]
    dst = np.repeat(np.arange(N), deg)
    src = rng.integers(0, N, size=len(dst))
    et = rng.integers(0, R_, size=len(dst))
    src = np.concatenate([src, [7, 7, 9]])
    dst = np.concatenate([dst, [8, 8, 9]])
    et = np.concatenate([et, [0, 0, R_ - 1]])
    order = rng.permutation(len(src))
    return N, src[order], dst[order], et[order]


def two_graphs(R_):
    """_two_graphs of tests/test_gpu_hgt.py: 3 + 4 nodes, 5 + 7 edges"""
    src = np.array([0, 1, 2, 2, 0, 3, 4, 5, 6, 3, 5, 4])
    dst = np.array([1, 2, 0, 1, 0, 4, 5, 6, 3, 5, 3, 4])
    return 7, src, dst, np.arange(12) % R_


HGT_GRAPHS = {"zoo": zoo, "two_graphs": two_graphs}


def pair_rows(dst, et, R_):
    """(row_dst, row_rel) of ops.HgtIndex: the non-empty (destination, edge type) pairs, grouped by edge type, by destination inside"""
    key = np.unique(np.asarray(et, np.int64) * (int(np.max(dst, initial=0)) + 1) + np.asarray(dst, np.int64))
    n = int(np.max(dst, initial=0)) + 1
    return key % n, key // n


class TypedCase(Case):
    """y[i] = rows[i] @ W[type_i] (ops.typed_linear: kind 'typed', the type = a node label; ops.hgt_pair_expand: kind 'expand', the
    rows = q[row_dst], the type = row_rel, gradient of q summed over a destination's pairs) or agg[d] = sum over the pairs of d of
    U[row] @ W[row_rel] (ops.hgt_pair_reduce: kind 'reduce').  Integer rows, signed-permutation weights."""
    params = ("W",)

    def __init__(self, kind, graph, mode, R_=4, H=16):
        rng = _rng(53, ("typed", "expand", "reduce").index(kind), sorted(HGT_GRAPHS).index(graph), list(DTYPES).index(mode))
        N, src, dst, et = HGT_GRAPHS[graph](R_)
        self.kind, self.N, self.R, self.H = kind, N, R_, H
        self.graph = (src, dst, et)
        rd, rr = pair_rows(dst, et, R_)
        self.row_dst, self.row_rel = _i64(rd), _i64(rr)
        P = len(rd)
        if kind == "typed":
            # (the node types belong to the graph, not to the dtype: one TypeIndex serves both)
            self.types = _i64(_rng(53, sorted(HGT_GRAPHS).index(graph)).integers(0, R_, size=N))
            self.types[:R_] = torch.arange(R_)
            n_in, n_out = N, N
        else:
            n_in, n_out = (N, P) if kind == "expand" else (P, N)
        name = {"typed": "x", "expand": "q", "reduce": "U"}[kind]
        ins = {name: X.sparse_rows(rng, n_in, H, nnz=2, max_exp=1), "W": torch.stack([X.signed_weight(rng, H, H, 1) for _ in range(R_)])}
        self.rows_name = name
        super().__init__("%s %s %s" % (kind, graph, mode), mode, ins, [G.sparse_tri(rng, n_out, H, 0.3)])

    def fn(self, t, absolute=False, st=None):
        rows, W = t[self.rows_name], t["W"]
        if self.kind == "expand":
            rows = rows[self.row_dst]
        types = self.types if self.kind == "typed" else self.row_rel
        y = rows.new_zeros(rows.shape[0], W.shape[2])
        for r in range(self.R):
            i = (types == r).nonzero().reshape(-1)
            if i.numel():
                y = y.index_add(0, i, rows[i] @ W[r])
        return (seg_sum(y, self.row_dst, self.N) if self.kind == "reduce" else y,)


def typed_naive(c):
    rows, W = c.ins[c.rows_name], c.ins["W"]
    types = c.types if c.kind == "typed" else c.row_rel
    out = torch.zeros(c.N if c.kind == "reduce" else len(types), W.shape[2], dtype=torch.float64)
    for i in range(len(types)):
        row = rows[int(c.row_dst[i])] if c.kind == "expand" else rows[i]
        y = row @ W[int(types[i])]
        if c.kind == "reduce":
            out[int(c.row_dst[i])] += y
        else:
            out[i] = y
    return out


# ---- batchnorm_rows --------------------------------------------------------------------------------------------------------------
class BatchNormCase(Case):
    """Training-mode BatchNorm over the rows of [N, C] with N a power of two and integer rows: mean and biased variance are exact
    (sums of integers divided by a power of two); the normalised rows are not -- the one operator here that is compared within a bound.
    The statistics outputs take no gradient."""
    params = ("weight", "bias")
    EPS = 1e-5

    def __init__(self, N, C, mode):
        assert N & (N - 1) == 0
        rng = _rng(54, N, C, list(DTYPES).index(mode))
        ins = {"x": X.small_ints(rng, N, C, lo=-4, hi=4), "weight": X.small_ints(rng, C, lo=1, hi=2), "bias": X.small_ints(rng, C, lo=-1, hi=1)}
        super().__init__("batchnorm_rows %dx%d %s" % (N, C, mode), mode, ins, [X.tri_coef(rng, N, C)])

    def fn(self, t, absolute=False, st=None):
        return (F.batch_norm(t["x"], None, None, t["weight"], t["bias"], training=True, eps=self.EPS),)

    def stats(self):
        """(mean, biased variance) in exact arithmetic: S / N and (N sum x^2 - S^2) / N^2 with integers below 2^53 and N a power of two"""
        x = self.ins["x"]
        n = float(x.shape[0])
        s, s2 = x.sum(0), (x * x).sum(0)
        return s / n, (n * s2 - s * s) / (n * n)

    def premise(self):
        mean, var = self.stats()
        for k, v in (("mean", mean), ("var", var)):
            if not torch.equal(v.float().double(), v):
                raise X.PremiseError("%s: the batch %s is not exact in fp32" % (self.what, k))
        if not bool((var > 0).all()):
            raise X.PremiseError("%s: a constant column" % self.what)
        return {}


# ---- the cases, by id (built once, shared by the premise tests and the GPU tests, never changed) -------------------------------------
LINEAR_ACT = [(rows, H, mode, relu, bias) for rows in (1, 33, 300) for H, mode in ((64, "bf16"), (256, "bf16"), (64, "f32s"))
              for relu in (True, False) for bias in (True, False)]
# (Linears, H, mode): the generic loop (1 and 3 Linears), the fp32 chain, the bf16 chain, the three-launch chain at H = 256
RELU_MLP = [(L, H, mode, slope, rows) for L, H, mode in ((1, 64, "bf16"), (3, 64, "bf16"), (2, 64, "f32s"), (2, 64, "bf16"), (2, 256, "bf16"))
            for slope in (0.0, 0.25) for rows in (33, 300)]
CONV = [(H, mode, hubs) for H, mode in ((64, "bf16"), (256, "bf16"), (64, "f32s"), (64, "f32x")) for hubs in (True, False)]
NEIGHBOR_SUM = [(H, mode, sc) for H in (5, 64) for mode in ("f32", "bf16") for sc in (0, 1)]
REL_AGG = [(fin, fout, mode, scaled) for fin, fout in ((64, 64), (5, 7)) for mode in ("bf16", "f32s") for scaled in (False, True)]
LINEAR_ANY = [(rows, fin, fout, mode) for rows in (1, 300) for fin, fout in ((5, 128), (128, 3)) for mode in ("f32", "bf16")]
SI_EMBED = [(N, H, mode) for N, H in ((1, 64), (300, 64), (77, 20)) for mode in ("f32", "bf16")]
DUAL_AGG = [(m, kind, H, mode) for m in (DUAL_SUB, DUAL_MULT) for kind in ("below", "above") for H in (16, 128) for mode in ("f32", "bf16")]
DMP_EDGE = [(kind, 64, mode) for kind in ("below", "above") for mode in ("f32", "bf16")]
TYPED = [(kind, graph, mode) for kind in ("typed", "expand", "reduce") for graph in ("two_graphs", "zoo") for mode in ("f32", "bf16")]
# the layer functions: (function, H, mode, R) -- one batch of dummy-augmented graphs each (the dummy node: a hub on both sides)
LAYERS = [("f32", 64, "f32s", 8), ("small", 64, "bf16", 8), ("wide", 256, "bf16", 8), ("chain", 256, "bf16", 16)]
BATCHNORM = [(N, C, mode) for N, C in ((64, 64), (256, 40)) for mode in ("f32", "bf16")]


@functools.lru_cache(maxsize=None)
def linear_act_case(rows, H, mode, relu, bias):
    return MlpCase(rows, H, mode, 1, relu, 0.0, bias)


@functools.lru_cache(maxsize=None)
def relu_mlp_case(L, H, mode, slope, rows):
    return MlpCase(rows, H, mode, L, True, slope, True, seed=1)


@functools.lru_cache(maxsize=None)
def layer_case(fn, H, mode, R_):
    """chain: eight graphs of 30 nodes + the dummy node (every graph within one 32-node tile, as the function asks); else twelve graphs
    of up to 30 nodes"""
    rng = _rng(55, H, R_)
    batch = X.si_batch(rng, 8, R_, 30, 2.0, nmin=30) if fn == "chain" else X.si_batch(rng, 12, R_, 30, 2.0)
    return LayerCase(batch, H, R_, mode, nnz=1 if mode == "f32s" else 2)


conv_case = functools.lru_cache(maxsize=None)(ConvCase)
neighbor_sum_case = functools.lru_cache(maxsize=None)(NeighborSumCase)
rel_agg_case = functools.lru_cache(maxsize=None)(RelAggCase)
linear_any_case = functools.lru_cache(maxsize=None)(LinearAnyCase)
si_embed_case = functools.lru_cache(maxsize=None)(SiEmbedCase)
dual_agg_case = functools.lru_cache(maxsize=None)(DualAggCase)
dmp_edge_case = functools.lru_cache(maxsize=None)(DmpEdgeCase)
typed_case = functools.lru_cache(maxsize=None)(TypedCase)
batchnorm_case = functools.lru_cache(maxsize=None)(BatchNormCase)


def all_cases():
    """(id, constructor, arguments) of every case above"""
    out = []
    for name, fn, table in (("linear_act", linear_act_case, LINEAR_ACT), ("relu_mlp", relu_mlp_case, RELU_MLP), ("conv", conv_case, CONV),
                            ("neighbor_sum", neighbor_sum_case, NEIGHBOR_SUM), ("rel_agg", rel_agg_case, REL_AGG),
                            ("linear_any", linear_any_case, LINEAR_ANY), ("si_embed", si_embed_case, SI_EMBED),
                            ("dual_agg", dual_agg_case, DUAL_AGG), ("dmp_edge", dmp_edge_case, DMP_EDGE), ("typed", typed_case, TYPED),
                            ("layer", layer_case, LAYERS), ("batchnorm", batchnorm_case, BATCHNORM)):
        out += [("%s-%s" % (name, "-".join(str(v) for v in a)), fn, a) for a in table]
    return out
