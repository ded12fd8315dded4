"""Operands, restatements and references for the exact tests of the aggregate-then-transform ("two-pass") relation path and of
everything only RGCN uses (test infrastructure only; not a conftest).  The third member of tests/exact_ref.py (RGIN layer paths) and
tests/gc_exact_ref.py (graph-classification kernels):

  A. ops.RelIndex / dn_rel_index_build_i32: rel_index_ref() restates the ten tables from the contract in include/dn_hip.h (stable
     argsort of etype * N + dst, runs of equal key, stable groupings by destination and by source); check_row_table() decodes a tile
     / chunk table the way its consumers do.  Integer tables: compared with torch.equal.
  B. ops.rel_agg_transform: AggCase -- out[v] = sum_e s_e x[src_e] W[etype_e] by index_add and autograd in float64, and a premise on
     EVERY storage point of the path (the [P, in] aggregated rows, the [P, out] products, the per-node sums, backwards gY, gA, gx, gW).
  C. graph_classification RGCNConv on that path: ConvCase (mean over (relation, destination) segments of power-of-two length is exact;
     MeanCase: lengths 3 and 5 under the 1-ulp rule of gc_exact_ref.assert_mean).
  D. subgraph_isomorphism RGCNLayer with edge_norm none / in / both: norm_batch() builds graphs whose every degree (+ 1 with the self
     loop) is a power of four, so that 1 / d, both square roots, their bf16 casts and sqrt(out_norm[src] * in_norm[dst]) are exact;
     rgcn_ref() restates oracle.layers.rgcn_layer per relation (pinned to it bit for bit by the CPU guard).

Operand rules (as the two earlier files): integer / sparse rows, signed 0 / +-1 weights, upstream gradients in {-1, 0, 1}, edge scales in
{-1, 0.5, 1, 2}.  Premises: a stored value is exactly representable where it is held and sum |terms| / quantum < 2^24 for every sum
(gc_exact_ref.check_premise; B and C), or every stage bounded on absolute values by 256 quanta in bf16 / 2^24 in fp32
(exact_ref.check_premise; D, whose fused formulation holds partial sums of a stage in bf16).  fp32 products on the 3-term bf16 split:
the wide operand holds at most 16 significant bits, the narrow one at most 8.  A premise failure raises exact_ref.PremiseError: a fault
of the test, never a reason to skip.

Everything here runs on the CPU and nothing imports the package's HIP library; tests/test_rel_exact_premise.py proves the premises and
checks the restatements against naive loops, tests/test_gpu_rel_exact.py holds the kernels to them."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

import exact_ref as X
import gc_exact_ref as G
from oracle import layers as OL

F32, BF16 = torch.float32, torch.bfloat16
WGRAD_CHUNK_ROWS = 4096                     # ops.WGRAD_CHUNK_ROWS (its default): the step of RelIndex.chunk_table
TABLE_STEPS = (64, 1024, WGRAD_CHUNK_ROWS)  # gemm_tiles, gemm_chunks, chunk_table
# relation sizes in segments at the edges of all three row tables, an empty relation among them
TABLE_EDGE_SIZES = [0, 1, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097]
INDEX_TABLES = ("perm1", "src1", "seg_ptr", "seg_dst", "rel_ptr", "dptr", "sperm", "optr", "operm", "seg_by_src")


def _i64(a):
    return np.asarray(a, dtype=np.int64)


# ---- A. the relation index -------------------------------------------------------------------------------------------------------
def rel_index_ref(src, dst, et, N, R):
    """dn_rel_index_build_i32 restated from its contract (include/dn_hip.h): {table: int64 numpy} for the ten tables, 'P' and
    'rel_ptr_host'."""
    src, dst, et = _i64(src), _i64(dst), _i64(et)
    E = len(src)
    key = et * N + dst
    perm1 = np.argsort(key, kind="stable")
    skey = key[perm1]
    head = np.ones(E, dtype=bool)
    head[1:] = skey[1:] != skey[:-1]
    starts = np.flatnonzero(head)
    P = len(starts)
    seg_key = skey[starts]
    seg_dst, seg_rel = (seg_key % N, seg_key // N) if N else (seg_key, seg_key)
    seg_of_edge = np.empty(E, dtype=np.int64)
    seg_of_edge[perm1] = np.cumsum(head) - 1
    operm = np.argsort(src, kind="stable")
    out = {
        "perm1": perm1, "src1": src[perm1], "seg_ptr": np.concatenate([starts, [E]]), "seg_dst": seg_dst,
        "rel_ptr": np.searchsorted(seg_rel, np.arange(R + 1), side="left"),
        "dptr": np.concatenate([[0], np.cumsum(np.bincount(seg_dst, minlength=N))]), "sperm": np.argsort(seg_dst, kind="stable"),
        "optr": np.concatenate([[0], np.cumsum(np.bincount(src, minlength=N))]), "operm": operm, "seg_by_src": seg_of_edge[operm],
    }
    out = {k: _i64(v) for k, v in out.items()}
    out["P"] = P
    out["rel_ptr_host"] = [int(v) for v in out["rel_ptr"]]
    out["seg_of_edge"] = seg_of_edge
    return out


def rel_index_naive(src, dst, et, N, R):
    """The same tables by per-edge Python loops (small inputs): what rel_index_ref is checked against."""
    E = len(src)
    order = sorted(range(E), key=lambda e: (int(et[e]), int(dst[e]), e))
    segs = []                                                       # [relation, destination, [edges in perm1 order]]
    for e in order:
        if segs and segs[-1][0] == int(et[e]) and segs[-1][1] == int(dst[e]):
            segs[-1][2].append(e)
        else:
            segs.append([int(et[e]), int(dst[e]), [e]])
    seg_ptr, seg_of_edge = [0], {}
    for p, (_, _, es) in enumerate(segs):
        seg_ptr.append(seg_ptr[-1] + len(es))
        for e in es:
            seg_of_edge[e] = p
    rel_ptr = [sum(1 for s in segs if s[0] < r) for r in range(R + 1)]
    dptr, sperm = [0], []
    for v in range(N):
        sperm += [p for p, s in enumerate(segs) if s[1] == v]       # ascending segment = ascending relation
        dptr.append(len(sperm))
    optr, operm = [0], []
    for u in range(N):
        operm += [e for e in range(E) if int(src[e]) == u]          # ascending edge id
        optr.append(len(operm))
    out = {"perm1": order, "src1": [int(src[e]) for e in order], "seg_ptr": seg_ptr, "seg_dst": [s[1] for s in segs], "rel_ptr": rel_ptr,
           "dptr": dptr, "sperm": sperm, "optr": optr, "operm": operm, "seg_by_src": [seg_of_edge[e] for e in operm]}
    out = {k: _i64(v) for k, v in out.items()}
    out["P"] = len(segs)
    out["rel_ptr_host"] = rel_ptr
    return out


def row_table_ref(rel_ptr, step, M):
    """dn_row_tables_build_i32 restated: ([M, 4] records {relation, first row, end row, 0}, piece_ptr [R + 1]); the unused tail holds
    empty pieces of the last relation."""
    R = len(rel_ptr) - 1
    rec, pp = [], [0]
    for r in range(R):
        a, b = int(rel_ptr[r]), int(rel_ptr[r + 1])
        while a < b:
            rec.append((r, a, min(a + step, b), 0))
            a += step
        pp.append(len(rec))
    assert len(rec) <= M
    rec += [(R - 1, int(rel_ptr[R]), int(rel_ptr[R]), 0)] * (M - len(rec))
    return _i64(rec).reshape(-1, 4), _i64(pp)


def check_row_table(table, rel_ptr, step, piece_ptr=None, what="row table"):
    """Decode a tile / chunk table as its consumers do ({relation, first row, end row, .} per piece; pieces [piece_ptr[r],
    piece_ptr[r + 1]) are relation r's) and require: every row 0 .. P-1 in exactly one piece; no piece across a relation boundary or
    longer than the step; piece_ptr delimiting each relation's pieces.  Raises AssertionError."""
    t = _i64(table).reshape(-1, 4)
    rel_ptr = _i64(rel_ptr)
    R, P = len(rel_ptr) - 1, int(rel_ptr[-1])
    rel, beg, end = t[:, 0], t[:, 1], t[:, 2]
    assert ((rel >= 0) & (rel < R)).all(), "%s: a relation id outside [0, %d)" % (what, R)
    assert ((0 <= beg) & (beg <= end) & (end <= P)).all(), "%s: a piece outside [0, %d]" % (what, P)
    full = end > beg
    assert (end - beg <= step).all(), "%s: a piece longer than %d rows" % (what, step)
    assert ((beg >= rel_ptr[rel]) & (end <= rel_ptr[rel + 1]))[full].all(), "%s: a piece crosses a relation boundary" % what
    cover = np.zeros(P + 1, dtype=np.int64)
    np.add.at(cover, beg[full], 1)
    np.add.at(cover, end[full], -1)
    cover = np.cumsum(cover)[:P]
    bad = np.flatnonzero(cover != 1)
    assert len(bad) == 0, "%s: row %d lies in %d pieces (%d rows off)" % (what, int(bad[0]), int(cover[bad[0]]), len(bad))
    if piece_ptr is not None:
        pp = _i64(piece_ptr)
        assert len(pp) == R + 1 and pp[0] == 0 and (np.diff(pp) >= 0).all() and pp[-1] <= len(t), "%s: piece_ptr %s" % (what, pp[:8])
        for r in range(R):
            mine = np.zeros(len(t), dtype=bool)
            mine[pp[r]:pp[r + 1]] = True
            assert (rel[mine] == r).all(), "%s: piece_ptr[%d] spans another relation's piece" % (what, r)
            assert not (full & ~mine & (rel == r)).any(), "%s: a piece of relation %d outside its piece_ptr range" % (what, r)
            rows = int((end - beg)[mine].sum())
            assert rows == int(rel_ptr[r + 1] - rel_ptr[r]), "%s: relation %d's pieces hold %d rows" % (what, r, rows)


def table_rows(P, R, step):
    """entries ops.build_row_tables allocates"""
    return int(P) // int(step) + int(R) + 1


def segment_graph(rng, N, sizes, seg_len=None, dst_pool=None, src_pool=None):
    """Edges of a graph whose relation r holds exactly sizes[r] (relation, destination) segments: distinct destinations from dst_pool
    (default all nodes), seg_len(r, k) edges in the k-th of them (default 1), sources from src_pool, edge order shuffled.
    -> (src, dst, etype) int64."""
    dst_pool = np.arange(N) if dst_pool is None else _i64(dst_pool)
    src_pool = np.arange(N) if src_pool is None else _i64(src_pool)
    src, dst, et = [], [], []
    for r, k in enumerate(sizes):
        if k == 0:
            continue
        assert k <= len(dst_pool)
        ds = rng.permutation(dst_pool)[:k]
        lens = _i64([seg_len(r, i) for i in range(k)]) if seg_len is not None else np.ones(k, dtype=np.int64)
        dst.append(np.repeat(ds, lens))
        et.append(np.full(int(lens.sum()), r, dtype=np.int64))
        src.append(rng.choice(src_pool, size=int(lens.sum())))
    if not src:
        z = np.zeros(0, dtype=np.int64)
        return z, z.copy(), z.copy()
    p = rng.permutation(sum(len(s) for s in src))
    return np.concatenate(src)[p], np.concatenate(dst)[p], np.concatenate(et)[p]


def _with_ends(rng, N, R, E, hi_key=True, lo_key=True):
    """E random edges plus three (parallel) edges each on the largest sort key (relation R-1, destination N-1) and on key 0, shuffled"""
    src, dst, et = rng.integers(0, N, size=E), rng.integers(0, N, size=E), rng.integers(0, R, size=E)
    if hi_key:
        src, dst, et = np.append(src, [0, N - 1, 5]), np.append(dst, [N - 1] * 3), np.append(et, [R - 1] * 3)
    if lo_key:
        src, dst, et = np.append(src, [N - 1, 0, 7]), np.append(dst, [0] * 3), np.append(et, [0] * 3)
    p = rng.permutation(len(src))
    return _i64(src[p]), _i64(dst[p]), _i64(et[p])


def _index_cases():
    rng = np.random.default_rng(20)
    z = np.zeros(0, dtype=np.int64)
    c = {}
    c["E0"] = (z, z, z, 5, 3)
    c["N1-R1-self-loops"] = (np.zeros(4, np.int64), np.zeros(4, np.int64), np.zeros(4, np.int64), 1, 1)
    c["R1"] = (rng.integers(0, 50, 200), rng.integers(0, 50, 200), np.zeros(200, np.int64), 50, 1)
    et = rng.choice([1, 2, 4], size=300)                            # relations 0 (first), 3 (middle) and 5 (last) hold no edge
    c["empty-relations"] = (rng.integers(0, 40, 300), rng.integers(0, 40, 300), et, 40, 6)
    c["one-segment"] = (rng.integers(0, 10, 300), np.full(300, 7), np.full(300, 1), 10, 3)      # 300 parallel-destination edges
    keys = rng.permutation(64 * 4)[:200]
    c["every-edge-its-own-segment"] = (rng.integers(0, 64, 200), keys % 64, keys // 64, 64, 4)
    s = rng.integers(0, 30, 120)
    d = np.where(rng.random(120) < 0.5, s, rng.integers(0, 30, 120))
    c["self-loops"] = (s, d, rng.integers(0, 3, 120), 30, 3)
    c["ends-without-in-edges"] = (rng.integers(0, 40, 150), rng.integers(1, 39, 150), rng.integers(0, 3, 150), 40, 3)
    c["ends-without-out-edges"] = (rng.integers(1, 39, 150), rng.integers(0, 40, 150), rng.integers(0, 3, 150), 40, 3)
    c["keys-2^12"] = _with_ends(rng, 1024, 4, 500) + (1024, 4)                                  # N R - 1 = 2^12 - 1: 12 key bits
    c["keys-2^12+1"] = _with_ends(rng, 1025, 4, 500) + (1025, 4)                                # N R - 1 = 2^12 + 3: 13 key bits
    c["keys-2^12-top-only"] = _with_ends(rng, 1024, 4, 0, lo_key=False) + (1024, 4)
    c["keys-2^12+1-top-only"] = _with_ends(rng, 1025, 4, 0, lo_key=False) + (1025, 4)
    lens = lambda r, i: (1, 1, 1, 2, 3)[(r + i) % 5]  # noqa: E731
    c["table-edges"] = segment_graph(rng, 4200, TABLE_EDGE_SIZES, lens) + (4200, len(TABLE_EDGE_SIZES))
    return {k: (_i64(v[0]), _i64(v[1]), _i64(v[2]), int(v[3]), int(v[4])) for k, v in c.items()}


INDEX_CASES = _index_cases()


def sweep_case(rng):
    """One build of the random sweep: mixed sizes, E up to 3,000, sometimes few destinations (long segments) or unused relations"""
    N, R = int(rng.integers(1, 400)), int(rng.integers(1, 9))
    E = int(rng.integers(0, 3001)) if rng.random() < 0.8 else int(rng.integers(0, 8))
    nd = N if rng.random() < 0.6 else int(rng.integers(1, N + 1))
    rels = rng.permutation(R)[:int(rng.integers(1, R + 1))]
    return _i64(rng.integers(0, N, E)), _i64(rng.integers(0, nd, E)), _i64(rng.choice(rels, size=E)), N, R


# ---- B. rel_agg_transform --------------------------------------------------------------------------------------------------------
ANY_SHAPES = [(7, 32), (16, 16), (48, 80), (200, 2)]           # rows_wgrad_any on 1,024-row chunks
SQUARE_SHAPES = [(64, 64), (128, 128), (256, 256)]             # the matrix-core rows_wgrad, idx_g = seg_dst, 4,096-row chunks
AGG_MODES = ("f32x", "f32s", "bf16")                           # fp32 under ops.f32_exact(True), fp32 on the default split, bf16
ANY_SIZES = [1023, 0, 1024, 1025, 1, 63, 64, 65]
SQUARE_SIZES = [4095, 0, 4096, 4097, 1, 65]
SEG_LENGTHS = (2, 8, 9, 300)                                   # besides 1


def is_square(fin, fout):
    return fin == fout and fin in (64, 128, 256)


def agg_ids():
    return ["%dx%d-%s-%s" % (fi, fo, m, "scaled" if sc else "plain") for fi, fo in ANY_SHAPES + SQUARE_SHAPES for m in AGG_MODES
            for sc in (False, True)]


def agg_params():
    return [(fi, fo, m, sc) for fi, fo in ANY_SHAPES + SQUARE_SHAPES for m in AGG_MODES for sc in (False, True)]


def _agg_graph(fin, fout):
    """The graph of one shape class (shared by its modes): node 0 has no in-edge, node N-1 no out-edge; in every relation of 60 segments
    or more one segment each of 2, 8 and 9 edges, and in the first relation one of 300; the rest single edges."""
    sq = is_square(fin, fout)
    sizes, N = (SQUARE_SIZES, 4200) if sq else (ANY_SIZES, 1100)
    rng = np.random.default_rng([31, int(sq)])

    def lens(r, i):
        if sizes[r] < 60:
            return 1 + (i % 2 if sizes[r] > 1 else 0)
        return {7: 2, 19: 8, 40: 9}.get(i, 300 if (r == 0 and i == 55) else 1)
    src, dst, et = segment_graph(rng, N, sizes, lens, dst_pool=np.arange(1, N), src_pool=np.arange(0, N - 1))
    return src, dst, et, N, len(sizes), sizes


class AggCase:
    """One exact rel_agg_transform problem (float64 CPU tensors): x [N, in], W [R, in, out], upstream g [N, out], edge_scale [E] or None;
    .out / .gx / .gW the references; .points the storage points {name: (reference, bound on |terms|, terms)}."""

    def __init__(self, fin, fout, mode, scaled):
        assert mode in AGG_MODES
        self.fin, self.fout, self.mode, self.scaled = fin, fout, mode, scaled
        self.dtype = BF16 if mode == "bf16" else F32
        self.square = is_square(fin, fout)
        self.split = mode == "f32s" and self.square            # the only product of this path that runs on the bf16 split
        src, dst, et, N, R, sizes = _agg_graph(fin, fout)
        self.src, self.dst, self.et, self.N, self.R, self.sizes = src, dst, et, N, R, sizes
        E = len(src)
        rng = np.random.default_rng([32, fin, fout, AGG_MODES.index(mode), int(scaled)])
        if mode == "bf16":
            x = X.sparse_rows(rng, N, fin, nnz=1 if fin < 16 else 2, max_exp=1)
            g = G.sparse_tri(rng, N, fout, density=0.25)
        elif self.split:
            x = X.split_rows(rng, N, fin, nnz=1)
            g = X.tri_coef(rng, N, fout)
        else:
            x = G.int_rows(rng, N, fin, F32)
            g = X.tri_coef(rng, N, fout)
        self.x, self.g = x, g
        self.W = torch.stack([X.signed_weight(rng, fin, fout, s=1 if (mode == "bf16" or fin == fout) else min(2, fin)) for _ in range(R)])
        self.scale = G.scales(rng, E) if scaled else None
        self.ix = rel_index_ref(src, dst, et, N, R)
        self.what = "rel_agg_transform %dx%d %s %s" % (fin, fout, mode, "scaled" if scaled else "plain")
        self._reference()

    def _reference(self):
        src, dst, et = (torch.from_numpy(a) for a in (self.src, self.dst, self.et))
        s = self.scale.view(-1, 1) if self.scale is not None else None
        x, W = X.leaf(self.x), X.leaf(self.W)
        out = agg_ref(x, W, src, dst, et, self.N, s)
        out.backward(self.g)
        self.out, self.gx, self.gW = out.detach(), x.grad, W.grad
        # the storage points, from the path's own factorisation over the restated index
        ix = self.ix
        P, rp = ix["P"], ix["rel_ptr_host"]
        soe, sd = torch.from_numpy(ix["seg_of_edge"]), torch.from_numpy(ix["seg_dst"])
        rows = self.x[src] * (s if s is not None else 1.0)
        z = lambda n, h: torch.zeros(n, h, dtype=torch.float64)  # noqa: E731
        A, Ab = z(P, self.fin).index_add(0, soe, rows), z(P, self.fin).index_add(0, soe, rows.abs())
        Wa = self.W.abs()
        Y, Yb = X.per_relation_linear(A, self.W, rp), X.per_relation_linear(Ab, Wa, rp)
        agg, aggb = z(self.N, self.fout).index_add(0, sd, Y), z(self.N, self.fout).index_add(0, sd, Yb)
        gY = self.g[sd]
        gA, gAb = X.per_relation_linear(gY, self.W, rp, transpose_w=True), X.per_relation_linear(gY.abs(), Wa, rp, transpose_w=True)
        grows = gA[soe] * (s if s is not None else 1.0)
        growsb = gAb[soe] * (s.abs() if s is not None else 1.0)
        gx, gxb = z(self.N, self.fin).index_add(0, src, grows), z(self.N, self.fin).index_add(0, src, growsb)
        gW = torch.stack([A[rp[r]:rp[r + 1]].t() @ gY[rp[r]:rp[r + 1]] for r in range(self.R)])
        gWb = torch.stack([Ab[rp[r]:rp[r + 1]].t() @ gY[rp[r]:rp[r + 1]].abs() for r in range(self.R)])
        # (the factorised form is the same function: the index restatement and the references agree before a GPU is asked)
        for a, b, n in ((agg, self.out, "out"), (gx, self.gx, "gx"), (gW, self.gW, "gW")):
            if not torch.equal(a, b):
                raise X.PremiseError("%s: the factorised %s differs from the per-edge reference" % (self.what, n))
        self.A, self.gY = A, gY
        self.points = {"A": (A, Ab, [rows]), "Y": (Y, Yb, [A]), "out": (agg, aggb, [Y]), "gY": (gY, gY.abs(), [gY]),
                       "gA": (gA, gAb, [gY]), "gx": (gx, gxb, [grows]), "gW": (gW, gWb, [A])}

    def premise(self):
        worst = {}
        for k, (ref, bound, terms) in self.points.items():
            worst[k] = G.check_premise(ref, bound, self.dtype, terms, self.what + " " + k)
        if self.split:                                          # rows_wgrad on the split: A wide, the gathered g rows narrow
            if X.sig_bits(self.A) > 16:
                raise X.PremiseError("%s: the aggregated rows hold %d significant bits (at most 16)" % (self.what, X.sig_bits(self.A)))
            if X.sig_bits(self.g) > 8:
                raise X.PremiseError("%s: the upstream gradient holds %d significant bits (at most 8)" % (self.what, X.sig_bits(self.g)))
            if X.sig_bits(self.x) <= 8:
                raise X.PremiseError("%s: the lo plane of the split carries no data" % self.what)
        if self.scale is not None:                              # scales that differ inside a segment: a wrong permutation changes bits
            seg = self.ix["seg_of_edge"]
            s = self.scale.numpy()
            lo, hi = np.full(self.ix["P"], np.inf), np.full(self.ix["P"], -np.inf)
            np.minimum.at(lo, seg, s)
            np.maximum.at(hi, seg, s)
            if int((hi > lo).sum()) < 4:
                raise X.PremiseError("%s: edge scales do not differ inside the segments" % self.what)
        lens = np.diff(self.ix["seg_ptr"])
        want = {1, 300} | set(SEG_LENGTHS)
        if not want <= set(int(v) for v in lens):
            raise X.PremiseError("%s: segment lengths %s missing" % (self.what, sorted(want - set(int(v) for v in lens))))
        if [b - a for a, b in zip(self.ix["rel_ptr_host"][:-1], self.ix["rel_ptr_host"][1:])] != list(self.sizes):
            raise X.PremiseError("%s: relation sizes %s" % (self.what, self.ix["rel_ptr_host"]))
        indeg, outdeg = np.bincount(self.dst, minlength=self.N), np.bincount(self.src, minlength=self.N)
        if indeg[0] != 0 or outdeg[self.N - 1] != 0:
            raise X.PremiseError("%s: node 0 has in-edges or node N-1 out-edges" % self.what)
        return worst


def agg_ref(x, W, src, dst, et, N, s=None):
    """out[v] = sum_{e -> v} s_e x[src_e] W[etype_e] (float64, per relation by index_add; differentiable)"""
    out = x.new_zeros(N, W.shape[2])
    for r in range(W.shape[0]):
        e = (et == r).nonzero().reshape(-1)
        if e.numel():
            rows = x[src[e]] if s is None else x[src[e]] * s[e]
            out = out.index_add(0, dst[e], rows @ W[r])
    return out


@functools.lru_cache(maxsize=None)
def agg_case(fin, fout, mode, scaled):
    return AggCase(fin, fout, mode, scaled)


def agg_naive(x, W, src, dst, et, N, s=None):
    """the same sum edge by edge (small inputs)"""
    out = torch.zeros(N, W.shape[2], dtype=torch.float64)
    for e in range(len(src)):
        row = x[int(src[e])] * (float(s[e]) if s is not None else 1.0)
        out[int(dst[e])] += row @ W[int(et[e])]
    return out


# ---- C. GC RGCNConv --------------------------------------------------------------------------------------------------------------
CONV_SHAPES = [(7, 32), (64, 64)]
POW2_LENS = (1, 2, 4, 8, 64)


def conv_params():
    return [(fi, fo, aggr, root, bias, dt) for fi, fo in CONV_SHAPES for aggr in ("mean", "add") for root in (True, False)
            for bias in (True, False) for dt in ("f32", "bf16")]


def conv_id(p):
    fi, fo, aggr, root, bias, dt = p
    return "%dx%d-%s-%s-%s-%s" % (fi, fo, aggr, "root" if root else "noroot", "bias" if bias else "nobias", dt)


def rgcn_conv_ref(x, src, dst, et, weight, root, bias, aggr):
    """RGCNConv restated: sum_r aggr_{j in N_r(i)} x_j W_r + x_i root + bias (float64; differentiable)"""
    N = x.shape[0]
    out = x.new_zeros(N, weight.shape[2])
    for r in range(weight.shape[0]):
        e = (et == r).nonzero().reshape(-1)
        h = x.new_zeros(N, x.shape[1]).index_add(0, dst[e], x[src[e]])
        if aggr == "mean":
            h = h / torch.bincount(dst[e], minlength=N).clamp(min=1).to(x.dtype).view(-1, 1)
        out = out + h @ weight[r]
    if root is not None:
        out = out + x @ root
    if bias is not None:
        out = out + bias
    return out


class ConvCase:
    """One exact RGCNConv problem: 4 relations (relation 2 empty), 330 nodes, (relation, destination) segments of 1, 2, 4, 8 and 64 edges,
    node 0 without in-edges and node N-1 without out-edges.  References: out, gx and the gradient of every parameter present."""

    def __init__(self, fin, fout, aggr, root, bias, dt):
        self.fin, self.fout, self.aggr, self.dtype = fin, fout, aggr, (F32 if dt == "f32" else BF16)
        self.what = "RGCNConv " + conv_id((fin, fout, aggr, root, bias, dt))
        rng = np.random.default_rng([41, fin, fout, int(aggr == "mean"), int(root), int(bias), int(dt == "f32")])
        N, R, sizes = 330, 4, [70, 130, 0, 90]
        lens = lambda r, i: POW2_LENS[i % 5] if i % 13 < 5 else 1  # noqa: E731
        self.src, self.dst, self.et = segment_graph(rng, N, sizes, lens, dst_pool=np.arange(1, N), src_pool=np.arange(0, N - 1))
        self.N, self.R = N, R
        # a fused fp32 conv (H = 64, add, root) multiplies on the bf16 split: rows with data in the lo plane; elsewhere small integers
        self.fused = aggr == "add" and root and fin == fout == 64
        if self.dtype == BF16:
            self.x = X.sparse_rows(rng, N, fin, nnz=1, max_exp=1)
            # (a mean's terms are multiples of 1 / 64: sparse gradients keep the sums of a few of them within bf16's eight bits)
            self.g = G.sparse_tri(rng, N, fout, density=0.04 if aggr == "mean" else 0.25)
        else:
            self.x = X.split_rows(rng, N, fin, nnz=1) if self.fused else G.int_rows(rng, N, fin, F32)
            self.g = X.tri_coef(rng, N, fout)
        self.p = {"weight": torch.stack([X.signed_weight(rng, fin, fout, 1) for _ in range(R)])}
        if root:
            self.p["root"] = X.signed_weight(rng, fin, fout, 1)
        if bias:
            self.p["bias"] = X.small_ints(rng, fout, lo=-1, hi=1)
        src, dst, et = (torch.from_numpy(a) for a in (self.src, self.dst, self.et))
        x = X.leaf(self.x)
        pr = {k: X.leaf(v) for k, v in self.p.items()}
        out = rgcn_conv_ref(x, src, dst, et, pr["weight"], pr.get("root"), pr.get("bias"), aggr)
        out.backward(self.g)
        self.out, self.gx, self.gp = out.detach(), x.grad, {k: v.grad for k, v in pr.items()}

    def premise(self):
        """Every storage point of the two-pass path (as AggCase, with s_e = 1 / |segment| for the mean), the torch terms behind it and
        every gradient: representable in the dtype, sum |terms| / quantum < 2^24."""
        ix = rel_index_ref(self.src, self.dst, self.et, self.N, self.R)
        lens = np.diff(ix["seg_ptr"])
        if not set(int(v) for v in lens) == set(POW2_LENS):
            raise X.PremiseError("%s: segment lengths %s" % (self.what, sorted(set(int(v) for v in lens))))
        src = torch.from_numpy(self.src)
        soe, sd = torch.from_numpy(ix["seg_of_edge"]), torch.from_numpy(ix["seg_dst"])
        P, rp = ix["P"], ix["rel_ptr_host"]
        s = (1.0 / torch.from_numpy(lens).double())[soe].view(-1, 1) if self.aggr == "mean" else torch.ones(len(self.src), 1, dtype=torch.float64)
        W, Wa = self.p["weight"], self.p["weight"].abs()
        z = lambda n, h: torch.zeros(n, h, dtype=torch.float64)  # noqa: E731
        rows = self.x[src] * s
        A, Ab = z(P, self.fin).index_add(0, soe, rows), z(P, self.fin).index_add(0, soe, rows.abs())
        Y, Yb = X.per_relation_linear(A, W, rp), X.per_relation_linear(Ab, Wa, rp)
        agg, aggb = z(self.N, self.fout).index_add(0, sd, Y), z(self.N, self.fout).index_add(0, sd, Yb)
        gY = self.g[sd]
        gA, gAb = X.per_relation_linear(gY, W, rp, transpose_w=True), X.per_relation_linear(gY.abs(), Wa, rp, transpose_w=True)
        grows, growsb = gA[soe] * s, gAb[soe] * s
        gxa, gxab = z(self.N, self.fin).index_add(0, src, grows), z(self.N, self.fin).index_add(0, src, growsb)
        gWb = torch.stack([Ab[rp[r]:rp[r + 1]].t() @ gY[rp[r]:rp[r + 1]].abs() for r in range(self.R)])
        pts = {"A": (A, Ab, [rows]), "Y": (Y, Yb, [A]), "agg": (agg, aggb, [Y]), "gA": (gA, gAb, [gY]), "gx pass": (gxa, gxab, [grows]),
               "gW": (self.gp["weight"], gWb, [A])}
        outb, gxb = aggb, gxab
        if "root" in self.p:
            xr, ra = self.x @ self.p["root"], self.p["root"].abs()
            pts["x root"] = (xr, self.x.abs() @ ra, [self.x])
            pts["g root^T"] = (self.g @ self.p["root"].t(), self.g.abs() @ ra.t(), [self.g])
            pts["g:root"] = (self.gp["root"], self.x.abs().t() @ self.g.abs(), [self.x])
            outb, gxb = outb + self.x.abs() @ ra, gxb + self.g.abs() @ ra.t()
        if "bias" in self.p:
            pts["g:bias"] = (self.gp["bias"], self.g.abs().sum(0), [self.g])
            outb = outb + self.p["bias"].abs()
        if "root" in self.p and "bias" in self.p:               # (the sum before the bias is stored too)
            pts["agg + x root"] = (self.out - self.p["bias"], outb, [Y, self.x])
        pts["out"] = (self.out, outb, [Y, self.x])
        pts["gx"] = (self.gx, gxb, [grows, self.g])
        for k, (ref, bound, terms) in pts.items():
            G.check_premise(ref, bound, self.dtype, terms, self.what + " " + k)
        if self.fused and self.dtype == BF16:                  # the row pipeline holds partial sums of a stage in bf16: 256 quanta
            for k, (ref, bound, terms) in pts.items():
                if k != "gW" and not k.startswith("g:") and float(bound.max()) > X.BF16_LIMIT * X.quantum(*terms):
                    raise X.PremiseError("%s %s: sum |terms| reaches %g (over 256 quanta)" % (self.what, k, float(bound.max())))
        if self.fused and self.dtype == F32:
            if X.sig_bits(self.x) > 16 or X.sig_bits(Ab) > 16 or X.sig_bits(self.g) > 8 or X.sig_bits(z(self.N, self.fout).index_add(0, src, self.g.abs()[torch.from_numpy(self.dst)])) > 8:
                raise X.PremiseError("%s: split operands too wide" % self.what)
        return pts


@functools.lru_cache(maxsize=None)
def conv_case(*p):
    return ConvCase(*p)


class MeanCase:
    """RGCNConv(aggr='mean') over segments of 3 and 5 edges (and 1, 2, 4), no root, no bias, shaped so that the 1-ulp rule of
    gc_exact_ref.assert_mean applies to the conv's output and input gradient element by element: every destination has ONE segment, every
    source ONE out-edge, the k-th source of a segment of n holds its nonzeros in the columns c with c % 5 == k (so every element of a
    segment's sum is one source's entry: the kernel's product with the rounded reciprocal is at most 1 ulp from the correctly rounded
    quotient, and a dropped or misplaced edge leaves a whole column class wrong), and every weight is a signed permutation."""
    LENS = (3, 5, 1, 2, 4, 5, 3)

    def __init__(self, H, dt):
        self.H, self.dtype = H, (F32 if dt == "f32" else BF16)
        rng = np.random.default_rng([43, H, int(dt == "f32")])
        R, nd = 3, 90
        lens = _i64([self.LENS[i % len(self.LENS)] for i in range(nd)])
        E = int(lens.sum())
        self.N, self.R = nd + E + 2, R                           # destinations, then sources, then two isolated nodes
        dst = np.repeat(np.arange(nd), lens)
        k = np.concatenate([np.arange(n) for n in lens])        # position of the edge in its segment
        src = nd + np.arange(E)
        rel_of_dst = rng.integers(0, R, size=nd)
        et = np.repeat(rel_of_dst, lens)
        p = rng.permutation(E)
        self.src, self.dst, self.et = _i64(src[p]), _i64(dst[p]), _i64(et[p])
        x = X.small_ints(rng, self.N, H, lo=-7, hi=7) if self.dtype == F32 else X.small_ints(rng, self.N, H, lo=-2, hi=2)
        col = np.arange(H) % 5
        keep = np.ones((self.N, H), dtype=bool)
        keep[src] = col[None, :] == k[:, None]
        self.x = x * torch.from_numpy(keep.astype(np.float64))
        self.g = X.tri_coef(rng, self.N, H)
        self.W = torch.stack([X.signed_weight(rng, H, H, 1) for _ in range(R)])
        srct, dstt = torch.from_numpy(src), torch.from_numpy(dst)
        Wd = self.W[torch.from_numpy(rel_of_dst)]                # [nd, H, H]: the weight of every destination's one segment
        tot = torch.zeros(nd, H, dtype=torch.float64).index_add(0, dstt, self.x[srct])
        self.out_total = torch.zeros(self.N, H, dtype=torch.float64)
        self.out_total[:nd] = torch.bmm(tot.unsqueeze(1), Wd).squeeze(1)
        self.out_lens = torch.zeros(self.N, dtype=torch.long)
        self.out_lens[:nd] = torch.from_numpy(lens)
        self.gx_total = torch.zeros(self.N, H, dtype=torch.float64)
        self.gx_total[srct] = torch.bmm(self.g[dstt].unsqueeze(1), Wd[dstt].transpose(1, 2)).squeeze(1)
        self.gx_lens = torch.zeros(self.N, dtype=torch.long)
        self.gx_lens[srct] = torch.from_numpy(lens)[dstt]

    def premise(self):
        """One source entry per element of a segment's sum; the totals representable; the float64 conv reference is the quotient."""
        srct, dstt = torch.from_numpy(self.src), torch.from_numpy(self.dst)
        nz = torch.zeros(self.N, self.H, dtype=torch.float64).index_add(0, dstt, (self.x[srct] != 0).double())
        if float(nz.max()) > 1:
            raise X.PremiseError("mean case: an element of a segment's sum has %d terms" % int(nz.max()))
        if np.bincount(self.src, minlength=self.N).max() > 1:
            raise X.PremiseError("mean case: a source with two out-edges")
        for t in (self.out_total, self.gx_total):
            if not torch.equal(t.to(self.dtype).double(), t):
                raise X.PremiseError("mean case: a total is not representable")
        x = X.leaf(self.x)
        out = rgcn_conv_ref(x, srct, dstt, torch.from_numpy(self.et), self.W, None, None, "mean")
        out.backward(self.g)
        want = self.out_total / self.out_lens.clamp(min=1).double().view(-1, 1)
        wantg = self.gx_total / self.gx_lens.clamp(min=1).double().view(-1, 1)
        if not (torch.allclose(out.detach(), want, rtol=1e-15, atol=0) and torch.allclose(x.grad, wantg, rtol=1e-15, atol=0)):
            raise X.PremiseError("mean case: totals / lengths are not the conv's reference")
        if not ({3, 5} <= set(int(v) for v in self.out_lens)):
            raise X.PremiseError("mean case: lengths 3 and 5 missing")


# ---- D. SI RGCNLayer ---------------------------------------------------------------------------------------------------------------
def norm_graph(rng, n, R, self_loop):
    """One graph whose every in-degree and out-degree d has d + 1 in {1, 4, 16} (self_loop) or d in {0, 1, 4, 16}: an in-degree sequence,
    a permutation of it as the out-degree sequence, shuffled stubs matched (multi-edges and self edges welcome), random relations."""
    choices = _i64([0, 3, 15]) if self_loop else _i64([0, 1, 4, 16])
    prob = [0.25, 0.6, 0.15] if self_loop else [0.15, 0.4, 0.35, 0.1]
    ind = rng.choice(choices, size=n, p=prob)
    outd = rng.permutation(ind)
    dst = rng.permutation(np.repeat(np.arange(n), ind))
    src = rng.permutation(np.repeat(np.arange(n), outd))
    et = rng.integers(0, R, size=len(src))
    return _i64(src), _i64(dst), _i64(et), np.array([0, n], dtype=np.int64), np.array([0, len(src)], dtype=np.int64)


def norm_batch(seed, R, self_loop, graphs=12, nmax=40):
    """Several norm_graph()s (a single-node graph among them) as one batch: (src, dst, etype, node_ptr, edge_ptr)"""
    rng = np.random.default_rng([51, seed, R, int(self_loop)])
    sizes = [int(rng.integers(8, nmax + 1)) for _ in range(graphs)] + [1]
    return X.concat_batches(*[norm_graph(rng, n, R, self_loop) for n in sizes])


def norms_ref(src, dst, N, self_loop):
    """float64: in_deg, out_deg, in_norm, out_norm (1 / (d + 1), or 1 / d with 0 for d = 0), edge norm 'in' and 'both'"""
    ind, outd = np.bincount(dst, minlength=N), np.bincount(src, minlength=N)

    def nrm(d):
        d = d.astype(np.float64)
        return 1.0 / (d + 1.0) if self_loop else np.where(d == 0, 0.0, 1.0 / np.maximum(d, 1.0))
    inn, outn = nrm(ind), nrm(outd)
    return dict(in_deg=ind, out_deg=outd, in_norm=torch.from_numpy(inn), out_norm=torch.from_numpy(outn),
                edge_in=torch.from_numpy(inn[dst]), edge_both=torch.from_numpy(np.sqrt(outn[src] * inn[dst])))


def rgcn_params(rng, fin, fout, R, self_loop, regularizer, num_bases):
    p = {"bias": X.small_ints(rng, fout, lo=-1, hi=1)}
    if self_loop:
        p["loop_weight"] = X.signed_weight(rng, fin, fout, 1)
    B = R if regularizer == "none" or num_bases is None or num_bases > R or num_bases <= 0 else num_bases
    if regularizer in ("none", "basis"):
        p["weight"] = torch.stack([X.signed_weight(rng, fin, fout, 1) for _ in range(B)])
        if B < R:
            wc = np.zeros((R, B))
            for r in range(R):
                wc[r, rng.integers(0, B)] = rng.choice([-1.0, 1.0])
            p["w_comp"] = torch.from_numpy(wc)
    else:
        si, so = fin // B, fout // B
        p["weight"] = torch.stack([torch.stack([X.signed_weight(rng, si, so, 1) for _ in range(B)]).reshape(-1) for _ in range(R)])
    return p


def rgcn_ref(x, src, dst, et, p, R, regularizer="basis", num_bases=-1, edge_norm="in", act="relu", stages=None, absolute=False):
    """oracle.layers.rgcn_layer restated per relation (no [E, in, out] weight gather), norms in float64; stages receives the stored
    stages of both formulations: 'a:xin' = sqrt(out_norm) x ('both'), 'a:pipe' = the sum before the destination factor (fused), 'agg' =
    the normed neighbour sum and 'a:loop' = the normed self-loop term (generic), 'h' = the pre-activation.  absolute: no activation."""
    N, fin = x.shape
    B = R if regularizer == "none" or num_bases is None or num_bases > R or num_bases <= 0 else num_bases
    fout = p["weight"].shape[2] if regularizer != "bdd" else p["weight"].shape[1] // (B * (fin // B)) * B
    W = OL.relation_weights(p["weight"], p.get("w_comp"), regularizer, R, B, fin, fout)
    self_loop = p.get("loop_weight") is not None
    nr = norms_ref(src.numpy(), dst.numpy(), N, self_loop)
    one = torch.ones(N, dtype=torch.float64)
    s_in, s_out = {"none": (one, one), "in": (nr["in_norm"], one), "both": (nr["in_norm"].sqrt(), nr["out_norm"].sqrt())}[edge_norm]
    xin = x * s_out.view(-1, 1)
    pipe = x.new_zeros(N, fout)
    for r in range(R):
        e = (et == r).nonzero().reshape(-1)
        if e.numel():
            pipe = pipe.index_add(0, dst[e], xin[src[e]] @ W[r])
    # (h through the fused factorisation, (sum + self loop) s_in, so that the gradient reaching the pipeline is a stage of the graph; the
    #  generic formulation's two terms are stages beside it -- on these operands every order of the exact float64 sums gives the same bits)
    st = {"a:xin": xin, "agg": pipe * s_in.view(-1, 1)}
    if W is not p["weight"]:
        st["W"] = W                                              # the dense relation weights (basis / bdd): their gradient is stored
    total = pipe
    if self_loop:
        loop_pipe = xin @ p["loop_weight"]
        st["a:loop"] = loop_pipe * s_in.view(-1, 1)
        total = pipe + loop_pipe
    st["a:pipe"] = total
    h = total * s_in.view(-1, 1)
    if p.get("bias") is not None:
        h = h + p["bias"]
    st["h"] = h
    if stages is not None:
        for v in st.values():
            if v.requires_grad:
                v.retain_grad()
        stages.update(st)
    return h if absolute else OL.act_fn(act)(h)


class LayerCase:
    """One exact RGCNLayer problem: batch of norm_graph()s, float64 parameters, rows (a quarter of them zero), upstream gradient; the
    reference and the premise of BOTH formulations' stages on absolute values (exact_ref.check_premise)."""

    def __init__(self, fin, fout, dt, edge_norm, self_loop, regularizer="basis", num_bases=-1, act="relu", R=5, seed=0):
        self.fin, self.fout, self.dtype, self.edge_norm, self.self_loop = fin, fout, (F32 if dt == "f32" else BF16), edge_norm, self_loop
        self.R, self.act, self.kw = R, act, dict(regularizer=regularizer, num_bases=num_bases)
        self.fused = fin == fout and fin in (64, 128, 256)
        self.split = self.fused and self.dtype == F32
        self.what = "RGCNLayer %dx%d %s %s loop=%d %s/%s %s" % (fin, fout, dt, edge_norm, self_loop, regularizer, num_bases, act)
        self.batch = norm_batch(seed, R, self_loop)
        src, dst, et, nptr, _ = self.batch
        N = int(nptr[-1])
        self.N = N
        rng = np.random.default_rng([52, fin, fout, int(dt == "f32"), ("none", "in", "both").index(edge_norm), int(self_loop), seed])
        self.p = rgcn_params(rng, fin, fout, R, self_loop, regularizer, num_bases)
        x = X.split_rows(rng, N, fin, nnz=1) if self.split else X.sparse_rows(rng, N, fin, nnz=2, max_exp=0)
        x[torch.from_numpy(rng.random(N) < 0.25)] = 0.0
        self.x = x
        # (48 -> 80: a weight row holds several nonzeros, so a dense upstream gradient would pass 256 quanta at the input)
        self.coef = G.sparse_tri(rng, N, fout, 0.25) if (self.dtype == BF16 and fin != fout) else X.tri_coef(rng, N, fout)
        self.graph_of_row = np.repeat(np.arange(len(nptr) - 1), np.diff(nptr))
        self.srct, self.dstt, self.ett = (torch.from_numpy(a) for a in (src, dst, et))
        xr, pr, st = X.leaf(self.x), {k: X.leaf(v) for k, v in self.p.items()}, {}
        out = rgcn_ref(xr, self.srct, self.dstt, self.ett, pr, R, edge_norm=edge_norm, act=act, stages=st, **self.kw)
        out.backward(self.coef)
        self.ref = (out.detach(), xr.grad, {k: v.grad for k, v in pr.items()})
        self.st = st
        self.ties = int((st["h"] == 0).sum())
        self.norms = norms_ref(src, dst, N, self_loop)

    def premise(self):
        st = self.st
        xa, pa, sa = X.leaf(self.x.abs()), {k: X.leaf(v.abs()) for k, v in self.p.items()}, {}
        out = rgcn_ref(xa, self.srct, self.dstt, self.ett, pa, self.R, edge_norm=self.edge_norm, stages=sa, absolute=True, **self.kw)
        out.backward(self.coef.abs())
        b = {k: v.detach() for k, v in sa.items()}
        b["out"] = out.detach()
        for k, v in sa.items():
            if v.grad is not None:
                b["g:" + k] = v.grad.detach()
        b["g:x"] = xa.grad.detach()
        for k, v in pa.items():
            b["g:" + k] = v.grad.detach()
        q_f = X.quantum(self.x, *self.p.values(), *st.values())
        q_b = X.quantum(self.coef, *(v.grad for v in st.values() if v.grad is not None), self.ref[1])
        worst = X.check_premise(b, "f32" if self.dtype == F32 else "bf16", q_fwd=q_f, q_bwd=q_b)
        for k, v in [("out", self.ref[0]), ("g:x", self.ref[1])] + [("g:" + k, v) for k, v in self.ref[2].items()]:
            if not torch.equal(v.to(self.dtype).double(), v):
                raise X.PremiseError("%s: the reference of %s is not representable" % (self.what, k))
        if self.split:                                           # the pipeline's products on the bf16 split (as test_gpu_exact.Case)
            N, R = self.N, self.R
            gp = st["a:pipe"].grad
            kf, kb = self.dstt * R + self.ett, self.srct * R + self.ett
            agg_f = torch.zeros(N * R, self.fin, dtype=torch.float64).index_add(0, kf, st["a:xin"].detach()[self.srct])
            agg_b = torch.zeros(N * R, self.fout, dtype=torch.float64).index_add(0, kb, gp[self.dstt])
            for t in (self.x, st["a:xin"], agg_f):
                if X.sig_bits(t) > 16:
                    raise X.PremiseError("%s: a split product's wide operand holds %d significant bits" % (self.what, X.sig_bits(t)))
            for t in (self.coef, gp, agg_b):
                if X.sig_bits(t) > 8:
                    raise X.PremiseError("%s: a split product's narrow operand holds %d significant bits" % (self.what, X.sig_bits(t)))
        ok = {1, 4, 16}
        ind, outd = self.norms["in_deg"], self.norms["out_deg"]
        off = 1 if self.self_loop else 0
        allowed = ok | ({0} if not self.self_loop else set())
        if not (set(int(v) + off for v in ind) <= allowed and set(int(v) + off for v in outd) <= allowed):
            raise X.PremiseError("%s: a degree outside the powers of four" % self.what)
        if not self.self_loop and not ((ind == 0).any() and (outd == 0).any()):
            raise X.PremiseError("%s: no node of degree 0" % self.what)
        if self.act == "relu" and self.ties == 0:
            raise X.PremiseError("%s: no pre-activation ties at 0" % self.what)
        return worst


LAYER_CASES = {}
for _H, _dt in [(64, "bf16"), (128, "bf16"), (256, "bf16"), (64, "f32"), (128, "f32"), (256, "f32"), (32, "bf16"), (32, "f32"), ((48, 80), "bf16"),
                ((48, 80), "f32")]:
    _fi, _fo = _H if isinstance(_H, tuple) else (_H, _H)
    for _en in ("none", "in", "both"):
        for _sl in (True, False):
            LAYER_CASES["%dx%d-%s-%s-%s" % (_fi, _fo, _dt, _en, "loop" if _sl else "noloop")] = (_fi, _fo, _dt, _en, _sl)
for _H, _dt in [(64, "bf16"), (128, "f32"), (32, "bf16"), (32, "f32")]:
    LAYER_CASES["%dx%d-%s-both-loop-basis2" % (_H, _H, _dt)] = (_H, _H, _dt, "both", True, "basis", 2)
    LAYER_CASES["%dx%d-%s-in-noloop-bdd4" % (_H, _H, _dt)] = (_H, _H, _dt, "in", False, "bdd", 4)


@functools.lru_cache(maxsize=None)
def layer_case(name):
    return LayerCase(*LAYER_CASES[name])


# ---- degrees / edge_norm directly ------------------------------------------------------------------------------------------------
def _degree_cases():
    rng = np.random.default_rng(61)
    z = np.zeros(0, dtype=np.int64)
    hub_s = np.concatenate([rng.integers(1, 300, 5000), rng.integers(0, 300, 400)])
    hub_d = np.concatenate([np.zeros(5000, np.int64), rng.integers(1, 299, 400)])        # node 0: in-degree 5,000; node 299: none
    p = rng.permutation(len(hub_s))
    b = norm_batch(3, 4, False)
    return {"hub-5000": (_i64(hub_s[p]), _i64(hub_d[p]), 300), "E0": (z, z, 7),
            "degree-0": (_i64(rng.integers(2, 20, 60)), _i64(rng.integers(0, 18, 60)), 20),
            "powers-of-four": (b[0], b[1], int(b[3][-1]))}


DEGREE_CASES = _degree_cases()
