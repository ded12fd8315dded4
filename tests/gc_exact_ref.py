"""Operands on which the graph-classification kernels' arithmetic is exact, and their references (test infrastructure only; not a
conftest).  The GC side of tests/exact_ref.py: dn_segment.hip (gather_segsum in its five forms, the readouts, max routing, edge_dot),
dn_graphsum.hip (the tile path of the fp32 GIN aggregation) and dn_gemm.hip (the any-width products).

The reference of every case is float64 index_add / matmul on the same operands.  Every case holds its PREMISE on absolute values before
anything is compared (check_premise):
  * the float64 reference is exactly representable in the output dtype (rounding it once changes nothing);
  * for every output element, sum |terms| / quantum < 2^24: whatever order, chunking or accumulator split a kernel uses, each partial
    sum is an integer number of quanta below 2^24, so fp32 accumulation is exact.
Operands: fp32 -- integer rows in [-8, 8], scales in {-1, 0.5, 1, 2}, self_coef 1.25; bf16 -- sparse rows in {-2 .. 2} and summed lists
of at most 257 entries, so that every output stays within 256.  A mean over a list of n entries is exact for n a power of two; for any
other n the kernels multiply by the rounded reciprocal, which is accepted: at most 1 ulp (of the output dtype) from the correctly rounded
float64 quotient (assert_mean) -- one dropped small-integer row is far more.

Everything here runs on the CPU; tests/test_gc_exact_premise.py proves the premises and checks the references against naive loops
without a GPU, tests/test_gpu_gc_exact.py holds the kernels to them."""
import numpy as np
import torch

import exact_ref as X

F32, BF16 = torch.float32, torch.bfloat16
SELF_COEF = 1.25
F32_LIMIT = 2 ** 24


# ---- premise and comparisons -----------------------------------------------------------------------------------------------------
def check_premise(ref, bound, dtype, terms, what=""):
    """ref: the float64 reference; bound: the same sum over |terms|; terms: tensors whose elements are the terms summed (they define
    the quantum).  Raises exact_ref.PremiseError -- a fault of the test's operands, never a reason to skip."""
    fin = torch.isfinite(ref)
    r = torch.where(fin, ref, torch.zeros_like(ref))
    if not torch.equal(r.to(dtype).double(), r):
        bad = (r.to(dtype).double() != r).nonzero()[0].tolist()
        raise X.PremiseError("%s: the reference is not representable in %s (first at %s: %r)" % (what, dtype, bad, float(r[tuple(bad)])))
    q = X.quantum(*[torch.where(torch.isfinite(t), t, torch.zeros_like(t)) for t in terms])
    b = torch.where(torch.isfinite(bound), bound, torch.zeros_like(bound))
    m = float(b.abs().max()) if b.numel() else 0.0
    if not m / q < F32_LIMIT:
        raise X.PremiseError("%s: sum |terms| reaches %g = %g quanta of %g (limit 2^24)" % (what, m, m / q, q))
    return m / q


def _ordered(t):
    """floats -> integers in which neighbouring floats differ by 1 (sign-magnitude, -0 == +0)"""
    if t.dtype == BF16:
        i, mask = t.contiguous().view(torch.int16).to(torch.int64), 0x7fff
    else:
        i, mask = t.contiguous().view(torch.int32).to(torch.int64), 0x7fffffff
    mag = i & mask
    return torch.where(i < 0, -mag, mag)


def ulp_diff(got, want):
    return (_ordered(got) - _ordered(want.to(got.dtype))).abs()


def is_pow2(n):
    n = torch.as_tensor(n).long()
    return (n > 0) & ((n & (n - 1)) == 0)


def mean_want(total, lens, dtype):
    """The correctly rounded quotient total[s] / lens[s] (float64 division, one rounding to dtype); 0 for an empty list."""
    q = total / lens.clamp(min=1).double().view(-1, *([1] * (total.dim() - 1)))
    return q.to(dtype)


def assert_mean(got, total, lens, what):
    """got[s] against total[s] / lens[s]: bit-exact where lens[s] is a power of two (or 0), at most 1 ulp of got's dtype elsewhere."""
    got = got.detach()
    want = mean_want(total, lens, got.dtype).to(got.device)
    lens = lens.to(got.device)
    exact = is_pow2(lens) | (lens == 0)
    d = ulp_diff(got, want)
    lim = torch.where(exact, 0, 1).view(-1, *([1] * (got.dim() - 1)))
    bad = d > lim
    if bool(bad.any()):
        i = tuple(int(v) for v in bad.nonzero()[0])
        raise AssertionError("%s: %d elements off; first at %s (list of %d): got %r, want %r (%d ulp)" % (
            what, int(bad.sum()), i, int(lens[i[0]]), float(got[i]), float(want[i]), int(d[i])))


# ---- operands --------------------------------------------------------------------------------------------------------------------
def int_rows(rng, n, h, dtype):
    """fp32: dense integers in [-8, 8]; bf16: sparse rows in {-2 .. 2} (about two nonzeros a row, at least 6 % of the elements: a list
    of 257 entries then sums to a few dozen, far inside 256)."""
    if dtype == F32:
        return X.small_ints(rng, n, h, lo=-8, hi=8)
    keep = rng.random((n, h)) < min(0.5, max(2.0 / h, 0.06))
    return X.small_ints(rng, n, h, lo=-2, hi=2) * torch.from_numpy(keep.astype(np.float64))


def scales(rng, n):
    return torch.from_numpy(rng.choice([-1.0, 0.5, 1.0, 2.0], size=n))


def sparse_tri(rng, n, h, density=0.25):
    """upstream gradients in {-1, 0, 1}, mostly 0"""
    g = X.tri_coef(rng, n, h)
    return g * torch.from_numpy((rng.random((n, h)) < density).astype(np.float64))


def unaligned(t):
    """A contiguous copy of t that starts one element (4 bytes fp32, 2 bytes bf16) into a larger flat allocation: never 16-byte aligned."""
    flat = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    v = flat[1:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and (v.numel() == 0 or v.data_ptr() % 16 != 0)
    return v


# ---- (a) gather_segsum -----------------------------------------------------------------------------------------------------------
VEC_H = {F32: [4, 16, 20, 64, 128, 256, 260, 512], BF16: [8, 32, 64, 128, 256, 512, 520]}
SCALAR_H = {F32: [1, 3, 9], BF16: [70]}
ALIGN_H = [64, 128]
FORMS = ("pipelined", "vec1", "block")


def lpr_class(H, dtype, aligned=True):
    """(LPR, vector form?) as gather_segsum in dn_segment.hip picks them: 16-byte pieces per row -> the smallest LPR in {4 .. 64} that
    covers them (wider rows: several column passes at 64); H no multiple of the vector width or an unaligned pointer -> scalar, LPR 8
    for H <= 8, else 64."""
    vn = 4 if dtype == F32 else 8
    if aligned and H % vn == 0:
        pieces = H // vn
        for lpr in (4, 8, 16, 32, 64):
            if pieces <= lpr:
                return lpr, True
        return 64, True
    return (8 if H <= 8 else 64), False


def seg_counts(lpr):
    """S at the chunk edges: a chunk is 2 * 256 / LPR segments, the grid is rounded up to a multiple of 8 chunks (the tail: dn_xcd_chunk)."""
    c = 2 * 256 // lpr
    return sorted({1, 2, c - 1, c, c + 1, 7 * c + 1, 8 * c, 8 * c + 1})


def list_lengths(rng, S, lpr, form, pow2=False):
    """S list lengths from {0, 1, 7, 8, 9, LPR-1, LPR, LPR+1, 2 LPR, 2 LPR+1} (around KU = 8 row loads in flight and the re-fetch branch
    `base != beg` of lists longer than LPR) whose average M / S (integer division, as launch_lpr computes it) selects `form`:
    pipelined M / S < 16, vec1 16 <= M / S < 24, block (workgroup per segment) M / S >= 24.  Where the set cannot reach the average
    (LPR 4 and 8 top out at 9 and 17) lengths from {17, 31, 32, 33, 47, 4 LPR + 1} fill in.  pow2: powers of two (and 0) only."""
    base = [0, 1, 7, 8, 9, lpr - 1, lpr, lpr + 1, 2 * lpr, 2 * lpr + 1]
    fill = [17, 31, 32, 33, 47, min(4 * lpr + 1, 255)]
    if pow2:
        base, fill = [0, 1, 8, lpr, 2 * lpr], [16, 32, 64]
    cand = sorted(set(base + fill))
    lo, hi = {"pipelined": (0, 16), "vec1": (16, 24), "block": (24, 1 << 30)}[form]
    lens = np.array([base[i % len(base)] for i in range(S)], dtype=np.int64)
    rng.shuffle(lens)
    cand_a = np.asarray(cand, dtype=np.int64)
    for _ in range(20000):
        M = int(lens.sum())
        a = M // S
        if lo <= a < hi:
            return lens
        # (replace lengths that occur more than once while there are some: every member of the set stays in as long as S allows; several
        #  at a time while the average is far off -- each moves the total by at most the largest length, so nothing overshoots)
        vals, inv, cnt = np.unique(lens, return_inverse=True, return_counts=True)
        down = a >= hi
        movable = lens > cand[0] if down else lens < cand[-1]
        pool = np.flatnonzero(movable & (cnt[inv] > 2))
        if len(pool) == 0:
            pool = np.flatnonzero(movable)
        need = (M - hi * S + 1) if down else (lo * S - M)
        k = max(1, min(len(pool) // 2, need // int(cand[-1])))
        pick = rng.choice(pool, size=k, replace=False)
        pos = np.searchsorted(cand_a, lens[pick])
        new = rng.integers(0, pos) if down else rng.integers(pos + 1, len(cand_a))
        lens[pick] = cand_a[new]
    raise X.PremiseError("no list lengths with average in [%d, %d) for S = %d, LPR = %d" % (lo, hi, S, lpr))


COMBOS = {
    # name: (idx given, ptr given, scale, self term, mean, power-of-two lengths only)
    "plain": (True, True, False, False, False, False),
    "scale": (True, True, True, False, False, False),
    "self": (True, True, False, True, False, False),
    "scale+self": (True, True, True, True, False, False),
    "mean": (True, True, False, False, True, False),
    "idx=None": (False, True, False, True, False, False),
    "ptr=None": (True, False, True, False, False, False),
    # (a mean next to a self term is exact only for power-of-two lengths; in bf16 its sum with 1.25 self is not representable)
    "mean+scale+self": (True, True, True, True, True, True),
}


def combos_of(dtype):
    return [k for k in COMBOS if dtype == F32 or k != "mean+scale+self"]


class GatherCase:
    """One gather_segsum problem: x [rows, H], idx [M], ptr [S + 1], scale [M], self_in [S, H] (float64 / int64, CPU) for one combination
    of arguments; .ref (float64 sum, before a mean's division), .lens, .bound."""

    def __init__(self, seed, dtype, H, lpr, S, form, combo):
        use_idx, use_ptr, use_scale, use_self, mean, pow2 = COMBOS[combo]
        rng = np.random.default_rng([seed, H, S, FORMS.index(form), sorted(COMBOS).index(combo), 0 if dtype == F32 else 1])
        lens = list_lengths(rng, S, lpr, form, pow2)
        M = int(lens.sum())
        self.dtype, self.H, self.S, self.M, self.mean, self.combo = dtype, H, S, M, mean, combo
        rows = max(300, M)
        self.x = int_rows(rng, rows, H, dtype)
        idx = torch.from_numpy(rng.integers(0, rows, size=M))
        ptr = torch.from_numpy(np.concatenate([[0], np.cumsum(lens)]))
        scale = scales(rng, M) if use_scale else None
        if not use_ptr:                                   # a pure (scaled) row gather: S = M lists of one entry
            lens = np.ones(M, dtype=np.int64)
            self.S = S = M
            ptr_ref = torch.arange(M + 1)
        else:
            ptr_ref = ptr
        self.idx, self.ptr, self.scale = (idx if use_idx else None), (ptr if use_ptr else None), scale
        self.self_in = int_rows(rng, S, H, dtype) if use_self else None
        self.lens = torch.from_numpy(lens)
        seg = torch.repeat_interleave(torch.arange(S), self.lens)
        rows_ = self.x[idx] if use_idx else self.x[:M]
        if scale is not None:
            rows_ = rows_ * scale.view(-1, 1)
        self.ref = torch.zeros(S, H, dtype=torch.float64).index_add(0, seg, rows_)
        self.bound = torch.zeros(S, H, dtype=torch.float64).index_add(0, seg, rows_.abs())
        terms = [rows_]
        if mean:                                          # (only reached with power-of-two lengths when a self term follows)
            div = self.lens.clamp(min=1).double().view(-1, 1)
            if use_self:
                self.ref, self.bound = self.ref / div, self.bound / div
                terms = [rows_ / div[seg]]
        if use_self:
            self.ref = self.ref + SELF_COEF * self.self_in
            self.bound = self.bound + SELF_COEF * self.self_in.abs()
            terms.append(SELF_COEF * self.self_in)
        self.terms = terms
        self.self_coef = SELF_COEF if use_self else 0.0
        self.what = "gather_segsum %s H=%d S=%d M=%d %s %s" % (str(dtype)[6:], H, S, M, form, combo)

    def premise(self):
        if self.mean and self.self_in is None:            # the sum is the exact part; the quotient follows the 1-ulp rule
            return check_premise(self.ref, self.bound, F32, self.terms, self.what)
        return check_premise(self.ref, self.bound, self.dtype, self.terms, self.what)

    def compare(self, got):
        if self.mean and self.self_in is None:
            assert_mean(got, self.ref, self.lens, self.what)
        else:
            X.assert_bits(got, self.ref, self.what)


def gather_cases(seed, dtype, H, aligned=True):
    lpr, _ = lpr_class(H, dtype, aligned)
    for S in seg_counts(lpr):
        for form in FORMS:
            for combo in combos_of(dtype):
                yield GatherCase(seed, dtype, H, lpr, S, form, combo)


# ---- (b) hub splitting -----------------------------------------------------------------------------------------------------------
HUB_DEGREES = {F32: (63, 64, 65, 128, 129, 600), BF16: (63, 64, 65, 128, 129)}


def hub_graph(rng, degrees, others=700):
    """Nodes 0 .. len(degrees)-1 have in-degree AND out-degree exactly degrees[k] (distinct partners among the other nodes); the others
    carry a few random edges among themselves.  -> (src, dst, N) int64 numpy, edges shuffled."""
    nh = len(degrees)
    N = nh + others
    src, dst = [], []
    for k, d in enumerate(degrees):
        a = nh + rng.permutation(others)[:d]
        b = nh + rng.permutation(others)[:d]
        src += list(a) + [k] * d
        dst += [k] * d + list(b)
    m = 2 * others
    src += list(nh + rng.integers(0, others, size=m))
    dst += list(nh + rng.integers(0, others, size=m))
    p = rng.permutation(len(src))
    src, dst = np.asarray(src, np.int64)[p], np.asarray(dst, np.int64)[p]
    for k, d in enumerate(degrees):
        assert int((dst == k).sum()) == d and int((src == k).sum()) == d
    return src, dst, N


class NeighborCase:
    """out = self_coef x + sum_{e -> v} w_e rows[e] and its input gradient under upstream g (float64 references, premises on both).
    edge rows: rows[e] = x[src[e]] (neighbor_sum) or ef[e] (edge_sum, self_coef 0)."""

    def __init__(self, x, src, dst, N, g, self_coef=0.0, w=None, edge_rows=False, what=""):
        src, dst = torch.as_tensor(src), torch.as_tensor(dst)
        ws = w.view(-1, 1) if w is not None else 1.0
        rows = (x if edge_rows else x[src]) * ws
        z = torch.zeros(N, x.shape[1], dtype=torch.float64)
        self.out = z.index_add(0, dst, rows)
        self.out_bound = z.index_add(0, dst, rows.abs())
        self.out_terms = [rows]
        grows = g[dst] * ws
        if edge_rows:
            self.gin, self.gin_bound = grows, grows.abs()
        else:
            self.out = self.out + self_coef * x
            self.out_bound = self.out_bound + abs(self_coef) * x.abs()
            self.out_terms.append(self_coef * x)
            zr = torch.zeros(x.shape[0], x.shape[1], dtype=torch.float64)
            self.gin = zr.index_add(0, src, grows) + self_coef * g
            self.gin_bound = zr.index_add(0, src, grows.abs()) + abs(self_coef) * g.abs()
        self.gin_terms = [grows, self_coef * g]
        self.what = what

    def premise(self, dtype):
        check_premise(self.out, self.out_bound, dtype, self.out_terms, self.what + " output")
        check_premise(self.gin, self.gin_bound, dtype, self.gin_terms, self.what + " input gradient")


# ---- (c) the tile path -----------------------------------------------------------------------------------------------------------
# graphs of 0, 1, 63, 64, 65 and 200 rows: tiles packed to exactly 64 rows (63 + 1, 64, 1 + 63), empty graphs first, in the middle and
# last, graphs of 65 and 200 rows (row lists) between the tiles, the last tile ending at N
TILE_SIZES = [0, 63, 1, 0, 64, 65, 1, 63, 200, 0, 63, 1, 200, 65, 64, 1, 63, 0]


def tile_batch(rng, flaw=None):
    """-> (src, dst, node_ptr, info).  Every graph: random edges (multi-edges included) and self loops.  Graphs of 200 rows: node 0 wired
    both ways to all 199 others (in- and out-list of 199: workgroup per row), nodes 1 / 2 with in-lists of exactly 64 / 65, nodes 3 / 4
    with out-lists of exactly 64 / 65 (the boundary between the lane-group and the workgroup row list).  The first graph of 63 rows holds
    255 parallel edges 5 -> 6, the first of 64 rows 256 parallel edges 9 -> 3: the largest counts the bf16 adjacency holds exactly.
    flaw = 'parallel257': 257 parallel edges on one pair; flaw = 'cross': one edge between two graphs (of different tiles) -- in-bounds
    inputs the tile kernel is written to refuse (its flag), for the fallback tests; on a small batch."""
    sizes = TILE_SIZES if flaw is None else [0, 30, 34, 64, 10, 70, 0]
    nptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    src, dst = [], []
    seen63 = seen64 = False
    for gi, n in enumerate(sizes):
        base = int(nptr[gi])
        if n == 0:
            continue
        free = np.arange(n)
        if n == 200:
            free = np.arange(5, n)
            for u in range(1, n):
                src += [base + u, base]; dst += [base, base + u]
            for node, k in ((1, 63), (2, 64)):                            # + 1 from node 0
                s = rng.permutation(free)[:k]
                src += list(base + s); dst += [base + node] * k
            for node, k in ((3, 63), (4, 64)):                            # + 1 to node 0
                d = rng.permutation(free)[:k]
                src += [base + node] * k; dst += list(base + d)
        m = int(2.5 * len(free))
        if len(free) > 1:
            s, d = rng.choice(free, size=m), rng.choice(free, size=m)
            keep = ~(((s == 5) & (d == 6)) | ((s == 9) & (d == 3)))        # (the counted pairs get no random edge on top)
            src += list(base + s[keep]); dst += list(base + d[keep])
        loops = rng.choice(free, size=max(1, len(free) // 8))
        src += list(base + loops); dst += list(base + loops)
        if flaw is None and n == 63 and not seen63:
            seen63 = True
            src += [base + 5] * 255; dst += [base + 6] * 255
        if flaw is None and n == 64 and not seen64:
            seen64 = True
            src += [base + 9] * 256; dst += [base + 3] * 256
    if flaw == "parallel257":
        b = int(nptr[3])
        src += [b + 9] * 257; dst += [b + 3] * 257
    elif flaw == "cross":
        src += [int(nptr[1]) + 2]; dst += [int(nptr[3]) + 7]              # graph 1 (tile 0) -> graph 3 (tile 1)
    p = rng.permutation(len(src))
    src, dst = np.asarray(src, np.int64)[p], np.asarray(dst, np.int64)[p]
    return src, dst, nptr


def plain_rows(src, dst, N):
    """Rows without a self loop whose every edge pair (either way) occurs once: a wide value there enters every sum at most once."""
    key = src * N + dst
    _, inv, cnt = np.unique(key, return_inverse=True, return_counts=True)
    multi = cnt[inv] > 1
    bad = np.zeros(N, dtype=bool)
    bad[src[multi]] = True
    bad[dst[multi]] = True
    bad[src[src == dst]] = True
    return ~bad


def tile_rows(rng, src, dst, nptr, H, self_coef, p_wide=0.3):
    """fp32 rows for the tile path: small integers; in a graph's column, with probability p_wide, zeros and ONE wide odd value (17 .. 24
    significant bits: all three bf16 planes hi / mid / lo of the kernel's split carry bits) at a plain row -- every sum that meets it
    is the value once (+ self_coef times it at its own row), still one fp32 value.  With self_coef = 1.25 = 5 / 4 the widest is 21 bits."""
    N = int(nptr[-1])
    x = X.small_ints(rng, N, H, lo=-8, hi=8)
    plain = plain_rows(src, dst, N)
    top = 24 if float(self_coef) in (0.0, 1.0) else 21
    for g in range(len(nptr) - 1):
        a, b = int(nptr[g]), int(nptr[g + 1])
        cand = a + np.flatnonzero(plain[a:b])
        if b == a:
            continue
        cols = np.flatnonzero(rng.random(H) < p_wide)
        x[a:b, cols] = 0.0
        if len(cand) == 0:
            continue
        for c in cols:
            bits = int(rng.integers(17, top + 1))
            v = float(int(rng.integers(2 ** (bits - 1), 2 ** bits)) | 1) * float(rng.choice([-1.0, 1.0]))
            x[int(rng.choice(cand)), c] = v
    return x


# ---- (d) readouts and max routing ------------------------------------------------------------------------------------------------
READOUT_H = [2, 7, 16, 64, 128, 200, 256]
READOUT_SIZES = [3, 0, 17, 1, 40, 0, 9, 64, 65, 130, 6, 5, 0]


def readout_rows(rng, H, with_inf):
    """Rows of small integers with many ties; segment 2 is one row repeated (a whole tied segment), segment 6 all negative, segment 10
    (with_inf, max only) holds only -inf; segments 1, 5 and 12 are empty.  bf16-exact: values in {-2 .. 2}, about half of them zero."""
    ptr = np.concatenate([[0], np.cumsum(READOUT_SIZES)]).astype(np.int64)
    N = int(ptr[-1])
    x = X.small_ints(rng, N, H, lo=-2, hi=2) * torch.from_numpy((rng.random((N, H)) < 0.6).astype(np.float64))
    x[ptr[2]:ptr[3]] = x[ptr[2]].clone()
    x[ptr[6]:ptr[7]] = -1.0 - torch.from_numpy(rng.integers(0, 2, size=(READOUT_SIZES[6], H)).astype(np.float64))
    if with_inf:
        x[ptr[10]:ptr[11]] = float("-inf")
    return x, ptr


def first_max_onehot(vals):
    """[k, H] -> bool [k, H]: the first row (lowest k) among the maxima of every column"""
    m = vals.max(0, keepdim=True).values
    hit = vals == m
    return hit & (hit.int().cumsum(0) == 1)


def segment_max_ref(x, ptr, g):
    """out[s] = max over rows [ptr[s], ptr[s+1]) (0 for an empty segment); gin: the first (lowest) row among the tied maxima receives
    the whole upstream entry -- the rule dn_segment_max documents, stated from the inputs."""
    S = len(ptr) - 1
    out = torch.zeros(S, x.shape[1], dtype=torch.float64)
    gin = torch.zeros_like(x)
    for s in range(S):
        a, b = int(ptr[s]), int(ptr[s + 1])
        if b > a:
            out[s] = x[a:b].max(0).values
            gin[a:b] = first_max_onehot(x[a:b]).double() * g[s]
    return out, gin


def neighbor_max_ref(x, src, dst, N, g):
    """out[v] = max over the edges into v of x[src] (0 for a node without in-edges); gin: among the tied maxima of (v, column) the edge
    with the lowest ORIGINAL edge index into v receives g[v, column], added onto its source row."""
    out = torch.zeros(N, x.shape[1], dtype=torch.float64)
    gin = torch.zeros_like(x)
    for v in range(N):
        e = np.flatnonzero(dst == v)                               # ascending: original edge order
        if len(e):
            vals = x[src[e]]
            out[v] = vals.max(0).values
            gin.index_add_(0, torch.from_numpy(src[e]), first_max_onehot(vals).double() * g[v])
    return out, gin


def max_graph(rng, N=160, E=700):
    """Edges with multi-edges (the same source row gathered twice by one destination), isolated nodes (0, 1), node 2 fed by copies of
    one row (whole tied list), node 3 fed by all-negative rows 10 .. 14, node 4 fed only by the -inf rows 15 .. 17."""
    src, dst = rng.integers(5, N, size=E), rng.integers(5, N, size=E)
    dup = rng.integers(0, E, size=E // 5)
    src, dst = np.concatenate([src, src[dup]]), np.concatenate([dst, dst[dup]])
    src = np.concatenate([src, [20, 21, 22, 20], [10, 11, 12, 13, 14, 12], [15, 16, 17, 16]])
    dst = np.concatenate([dst, [2, 2, 2, 2], [3] * 6, [4] * 4])
    p = rng.permutation(len(src))
    return src[p].astype(np.int64), dst[p].astype(np.int64), N


def max_rows(rng, N, H):
    x = X.small_ints(rng, N, H, lo=-2, hi=2)
    x[21] = x[20]; x[22] = x[20]
    x[10:15] = -1.0 - torch.from_numpy(rng.integers(0, 2, size=(5, H)).astype(np.float64))
    x[15:18] = float("-inf")
    return x


# ---- (e) edge_dot ----------------------------------------------------------------------------------------------------------------
EDGE_DOT_H = [1, 3, 16, 17, 64, 128, 200, 256]
EDGE_DOT_E = [1, 15, 16, 17, 1000]


def edge_dot_case(rng, dtype, H, E, use_ia, use_ib):
    """-> (a, ia, b, ib, ref [E] float64, bound): ia / ib None = row e itself."""
    na, nb = (50 if use_ia else E), (60 if use_ib else E)
    a, b = int_rows(rng, na, H, dtype), int_rows(rng, nb, H, dtype)
    ia = torch.from_numpy(rng.integers(0, na, size=E)) if use_ia else None
    ib = torch.from_numpy(rng.integers(0, nb, size=E)) if use_ib else None
    ra, rb = (a[ia] if use_ia else a), (b[ib] if use_ib else b)
    return a, ia, b, ib, (ra * rb).sum(1), (ra * rb).abs().sum(1), [ra * rb]


# ---- (f) the any-width products --------------------------------------------------------------------------------------------------
REL_SIZES = [0, 1, 63, 64, 65, 511, 512, 513, 1025]
GEMM_KN = [(1, 1), (5, 128), (38, 256), (65, 63), (100, 7), (64, 64)]


def sparse_ints(rng, n, h, nnz=2):
    """rows with at most nnz nonzeros of +-1 / +-2 (h = 1: a third of the rows nonzero, so that a thousand of them sum within 256)"""
    if h == 1:
        return X.small_ints(rng, n, 1, lo=-2, hi=2) * torch.from_numpy((rng.random((n, 1)) < 0.33).astype(np.float64))
    return X.sparse_rows(rng, n, h, nnz=nnz, max_exp=1)


class GemmCase:
    """Relation-major rows A [P, K], upstream rows G [P, N], weights W [R, K, N] of signed 0 / +-1 columns, bias [R, N]; float64 references
    of Y = A W_r + bias_r, Yt = G W_r^T, gW[r] = A_r^T G_r and the column sums of A per relation, with their bounds."""

    def __init__(self, seed, K, N, sizes=REL_SIZES):
        rng = np.random.default_rng([seed, K, N])
        self.K, self.N, self.sizes = K, N, sizes
        self.rel_ptr = [0] + [int(v) for v in np.cumsum(sizes)]
        R, P = len(sizes), self.rel_ptr[-1]
        self.R, self.P = R, P
        self.A, self.G = sparse_ints(rng, P, K), sparse_ints(rng, P, N, nnz=1) * torch.from_numpy(rng.integers(0, 2, size=(P, 1)).astype(np.float64))
        self.W = torch.stack([X.signed_weight(rng, K, N, s=min(2, K)) for _ in range(R)])
        self.bias = X.small_ints(rng, R, N, lo=-1, hi=1)
        rp = self.rel_ptr
        self.Y = X.per_relation_linear(self.A, self.W, rp, bias=self.bias)
        self.Y_bound = X.per_relation_linear(self.A.abs(), self.W.abs(), rp, bias=self.bias.abs())
        self.Yt = X.per_relation_linear(self.G, self.W, rp, transpose_w=True)
        self.Yt_bound = X.per_relation_linear(self.G.abs(), self.W.abs(), rp, transpose_w=True)
        self.gW = torch.stack([self.A[rp[r]:rp[r + 1]].t() @ self.G[rp[r]:rp[r + 1]] for r in range(R)])
        self.gW_bound = torch.stack([self.A[rp[r]:rp[r + 1]].abs().t() @ self.G[rp[r]:rp[r + 1]].abs() for r in range(R)])
        self.colsum = torch.stack([self.A[rp[r]:rp[r + 1]].sum(0) for r in range(R)])
        self.colsum_bound = torch.stack([self.A[rp[r]:rp[r + 1]].abs().sum(0) for r in range(R)])

    def premise(self, dtype):
        w = "any-width products K=%d N=%d " % (self.K, self.N)
        ints = [self.A, self.G, self.W, self.bias]
        check_premise(self.Y, self.Y_bound, dtype, ints, w + "Y")
        check_premise(self.Yt, self.Yt_bound, dtype, ints, w + "Yt")
        check_premise(self.gW, self.gW_bound, dtype, ints, w + "gW")
        check_premise(self.colsum, self.colsum_bound, F32, ints, w + "column sums")


class LinearCase:
    """y = x w^T + b over P rows (w [N, K] as nn.Linear stores it) and its three gradients under upstream g."""

    def __init__(self, seed, P, K, N):
        rng = np.random.default_rng([seed, P, K, N])
        self.P, self.K, self.N = P, K, N
        self.x, self.g = sparse_ints(rng, P, K), sparse_ints(rng, P, N, nnz=1) * torch.from_numpy(rng.integers(0, 2, size=(P, 1)).astype(np.float64))
        self.w = X.signed_weight(rng, K, N, s=min(2, K)).t().contiguous()
        self.b = X.small_ints(rng, N, lo=-1, hi=1)
        bd = X.linear_bounds(self.x, self.w, self.b, self.g)
        self.bounds = {"y": bd["y"], "gx": bd["g:x"], "gw": bd["g:weight"], "gb": bd["g:bias"]}
        self.refs = {"y": self.x @ self.w.t() + self.b, "gx": self.g @ self.w, "gw": self.g.t() @ self.x, "gb": self.g.sum(0)}

    def premise(self, dtype):
        for k, v in self.refs.items():
            check_premise(v, self.bounds[k], dtype, [self.x, self.g, self.w, self.b], "linear_any P=%d K=%d N=%d %s" % (self.P, self.K, self.N, k))


# ---- the cases of (b), (c), (d) as the GPU tests and the CPU premise tests both build them ----------------------------------------
def hub_case(seed, dtype, H, scaled):
    """neighbor_sum (self_coef 1.25) and edge_sum over hub_graph(HUB_DEGREES[dtype]), with or without a power-of-two edge_scale."""
    rng = np.random.default_rng([seed, H, int(scaled), 0 if dtype == F32 else 1])
    src, dst, N = hub_graph(rng, HUB_DEGREES[dtype])
    E = len(src)
    x, ef = int_rows(rng, N, H, dtype), int_rows(rng, E, H, dtype)
    g = X.tri_coef(rng, N, H) if dtype == F32 else sparse_tri(rng, N, H)
    w = torch.from_numpy(rng.choice([0.5, 1.0, 2.0], size=E)) if scaled else None
    what = "%s H=%d %s" % (str(dtype)[6:], H, "scaled" if scaled else "unscaled")
    return dict(src=src, dst=dst, N=N, x=x, ef=ef, g=g, w=w,
                neighbor=NeighborCase(x, src, dst, N, g, SELF_COEF, w, what="neighbor_sum over hubs " + what),
                edge=NeighborCase(ef, src, dst, N, g, 0.0, w, edge_rows=True, what="edge_sum over hubs " + what))


def tile_case(seed, H, self_coef, flaw=None):
    rng = np.random.default_rng([seed, H, int(self_coef * 4), {None: 0, "parallel257": 1, "cross": 2}[flaw]])
    src, dst, nptr = tile_batch(rng, flaw)
    N = int(nptr[-1])
    x, g = tile_rows(rng, src, dst, nptr, H, self_coef), tile_rows(rng, src, dst, nptr, H, self_coef)
    what = "tile path H=%d self_coef=%g %s" % (H, self_coef, flaw or "")
    return dict(src=src, dst=dst, nptr=nptr, N=N, x=x, g=g, case=NeighborCase(x, src, dst, N, g, self_coef, what=what))


def greedy_tiles(nptr, max_rows=64):
    """The packing dn_graph_tiles_host documents, restated: runs of whole graphs of at most max_rows rows; larger graphs break a run."""
    tiles, beg, end = [], None, None
    for g in range(len(nptr) - 1):
        a, b = int(nptr[g]), int(nptr[g + 1])
        if b == a:
            continue
        if b - a > max_rows:
            if beg is not None:
                tiles.append((beg, end))
            beg = None
            continue
        if beg is not None and b - beg > max_rows:
            tiles.append((beg, end))
            beg = None
        if beg is None:
            beg = a
        end = b
    if beg is not None:
        tiles.append((beg, end))
    return tiles
