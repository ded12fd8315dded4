"""Host-side operators over the dn_hip C ABI: raw launches + torch.autograd.Function wrappers.

Everything here runs on the GPU through libdn_hip.so; PyTorch only supplies device memory, the
current stream and autograd bookkeeping.  There is deliberately no CPU path.
"""
import contextlib as _contextlib
import ctypes
import os as _os
import threading as _threading
from typing import NamedTuple

import numpy as _np
import torch

from . import _lib
from ._lib import check, lib, ptr, require_gpu, stream_ptr

I32 = torch.int32


class KernelTimer:
    """Optional HIP-event timing of individual kernel launches on the current stream (bench.py's roofline leg).
    Events are recorded on the stream the kernel is launched on; elapsed times are read after a synchronize.
    `with KernelTimer() as t:` times the launches of the block: it installs t as ops.kernel_timer and puts back what it found."""

    def __init__(self):
        self.records = []  # (tag, start_event, end_event)
        self.enabled = True

    def __enter__(self):
        global kernel_timer
        self.found, kernel_timer = kernel_timer, self
        return self

    def __exit__(self, *exc):
        global kernel_timer
        kernel_timer = self.found
        return False

    def launch(self, tag, fn):
        if not self.enabled:
            return fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        r = fn()
        b.record()
        self.records.append((tag, a, b))
        return r

    def summary(self):
        torch.cuda.synchronize()
        out = {}
        for tag, a, b in self.records:
            ms = a.elapsed_time(b)
            cnt, tot = out.get(tag, (0, 0.0))
            out[tag] = (cnt + 1, tot + ms)
        return out

    def reset(self):
        self.records = []


kernel_timer = None  # set to a KernelTimer by bench.py


def launch_tagged(tag, fn):
    """fn() under kernel_timer's tag when a timer is set (read at call time: bench.py and the tests assign the module global).
    The benchmark counts launches by tag, so every kernel launch of a step goes through here; the table builders stay untagged."""
    if kernel_timer is not None:
        return kernel_timer.launch(tag, fn)
    return fn()


def _suffix(t):
    if t.dtype == torch.float32:
        return "f32"
    if t.dtype == torch.bfloat16:
        return "bf16"
    raise _lib.DnHipError("dn_hip kernels support float32 and bfloat16 features, got %s" % t.dtype)


def _i32(t, name):
    if t is not None and t.dtype != I32:
        raise _lib.DnHipError("%s must be int32 on the device (got %s)" % (name, t.dtype))
    return t


def _ws(nbytes, device):
    return torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device=device)


# ----------------------------------------------------------------------------------------------
# raw launches
# ----------------------------------------------------------------------------------------------
def gather_segsum(x, idx=None, ptr_=None, num_segments=None, scale=None, self_in=None, self_coef=0.0,
                  mean=False, out=None, tag="gather_segsum"):
    """out[s] = self_coef*self_in[s] + sum_{i in [ptr[s],ptr[s+1])} scale[i] * x[idx[i]]  (dn_gather_segsum_*)."""
    require_gpu(x, idx, ptr_, scale, self_in, out)
    assert x.dim() == 2
    _i32(idx, "idx"), _i32(ptr_, "ptr")
    # (the launch reads x.data_ptr() with x.shape[1] as the row stride and walks idx / ptr / scale / self_in element by element:
    #  require_gpu refuses a strided view -- x_wide[:, :H], idx[::2] -- that would be read as garbage)
    H = x.shape[1]
    M = idx.numel() if idx is not None else (x.shape[0] if ptr_ is None else None)
    if ptr_ is not None:
        S = ptr_.numel() - 1 if num_segments is None else int(num_segments)
        assert ptr_.numel() >= S + 1
        if M is None:
            M = 0  # contiguous rows: element i is row i; the kernel reads rows [ptr[0], ptr[S])
    else:
        S = M
    if scale is not None:
        assert scale.dtype == torch.float32 and idx is not None and scale.numel() == idx.numel()
    if self_in is not None:
        assert self_in.shape == (S, H) and self_in.dtype == x.dtype
    if out is None:
        out = torch.empty((S, H), dtype=x.dtype, device=x.device)
    else:
        assert out.shape == (S, H) and out.dtype == x.dtype and out.is_contiguous()
    fn = getattr(lib(), "dn_gather_segsum_" + _suffix(x))

    def _launch():
        check(fn(ptr(x), x.shape[0], H, ptr(idx), ptr(scale), ptr(ptr_), S, M, ptr(out), ptr(self_in),
                 float(self_coef), 1 if mean else 0, stream_ptr()), "dn_gather_segsum")

    launch_tagged(tag, _launch)
    return out


def graph_tiles(node_ptr, max_rows=64):
    """Greedy runs of whole graphs with at most max_rows rows each: (tiles [T, 2] int32 on the device, covered rows, rest) where
    rest = the rows of graphs larger than max_rows as a sorted int64 tensor (they keep the plain gather)."""
    npt = node_ptr.detach().cpu().tolist()
    tiles, rest, beg = [], [], None
    for g in range(len(npt) - 1):
        a, b = npt[g], npt[g + 1]
        if b - a > max_rows:
            if beg is not None:
                tiles.append((beg, a)); beg = None
            rest.append((a, b))
            continue
        if beg is None:
            beg = a
        elif b - beg > max_rows:
            tiles.append((beg, a)); beg = a
    if beg is not None:
        tiles.append((beg, npt[-1]))
    tiles = [(a, b) for a, b in tiles if b > a]
    t = torch.tensor(tiles, dtype=I32, device=node_ptr.device).reshape(-1, 2)
    covered = sum(b - a for a, b in tiles)
    r = (torch.cat([torch.arange(a, b) for a, b in rest]) if rest else torch.zeros(0, dtype=torch.long)).to(node_ptr.device)
    return t, covered, r


def graph_tile_records(tiles, ptr_):
    """[T, 4] int32 records {first row, end row, ptr[first row], ptr[end row]} of graph_tiles' row ranges for one CSR."""
    return torch.cat([tiles, ptr_[tiles.long()].to(I32)], 1).contiguous()


def gather_rows_sum(x, idx, ptr_, rows, workgroup_per_row, self_coef, out):
    """out[s] = self_coef * x[s] + sum of x[idx[i]] over s's list, for the listed rows only (dn_gather_rows_sum_f32)."""
    require_gpu(x, idx, ptr_, rows, out)
    assert x.dtype == torch.float32 and x.is_contiguous() and out.is_contiguous() and rows.dtype == I32 and rows.is_contiguous()
    records = rows.dim() == 2                                       # [n, 4] records {row, ptr[row], ptr[row + 1], 0}
    assert not records or rows.shape[1] == 4

    def _launch():
        check(lib().dn_gather_rows_sum_f32(ptr(x), int(x.shape[1]), ptr(ptr_), ptr(idx), ptr(rows), 1 if records else 0,
                                           int(rows.shape[0]), 1 if workgroup_per_row else 0, float(self_coef), ptr(out),
                                           stream_ptr()), "dn_gather_rows_sum_f32")
    launch_tagged("gather_rows_sum", _launch)
    return out


def graph_tile_sum(x, idx, ptr_, tiles, self_coef=0.0, out=None, seg=None, bad=None):
    """out[v] = self_coef * x[v] + sum of x[idx[i]] over v's list, for the rows of `tiles` only (dn_graph_tile_sum_f32: the tile's
    adjacency as a dense bf16 matrix, the rows as three bf16 planes, matrix cores).  Rows outside the tiles are left untouched.
    tiles: graph_tiles' [T, 2] row ranges or graph_tile_records' [T, 4]; seg (optional): the row of every index entry."""
    require_gpu(x, idx, ptr_, tiles)
    assert x.dtype == torch.float32 and x.is_contiguous() and x.shape[1] in (64, 128, 256)
    assert idx.dtype == I32 and ptr_.dtype == I32 and tiles.dtype == I32 and tiles.is_contiguous()
    if tiles.shape[1] == 2:
        tiles = graph_tile_records(tiles, ptr_)
    assert seg is None or (seg.dtype == I32 and seg.numel() == idx.numel())
    if out is None:
        out = torch.empty_like(x)
    if bad is None:                                                 # (a caller that launches repeatedly keeps ONE flag: the kernel only ORs)
        bad = torch.zeros(1, dtype=I32, device=x.device)

    def _launch():
        check(lib().dn_graph_tile_sum_f32(ptr(x), int(x.shape[0]), int(x.shape[1]), ptr(ptr_), ptr(idx),
                                          ptr(seg) if seg is not None else None, int(idx.numel()), ptr(tiles),
                                          int(tiles.shape[0]), float(self_coef), ptr(out), ptr(bad), stream_ptr()),
              "dn_graph_tile_sum_f32")
    launch_tagged("graph_tile_sum", _launch)
    return out, bad


def csr_build(key, num_keys):
    """Stable grouping by integer key: returns (ptr [num_keys+1], perm [M]) int32  (dn_csr_build_i32)."""
    require_gpu(key)
    _i32(key, "key")
    M = key.numel()
    p = torch.empty(num_keys + 1, dtype=I32, device=key.device)
    perm = torch.empty(M, dtype=I32, device=key.device)
    nbytes = lib().dn_csr_build_workspace_bytes(M, num_keys)
    if nbytes == 0:
        check(-2, "dn_csr_build_workspace_bytes")
    ws = _ws(nbytes, key.device)
    check(lib().dn_csr_build_i32(ptr(key), M, num_keys, ptr(p), ptr(perm), ptr(ws), ws.numel(), stream_ptr()),
          "dn_csr_build_i32")
    return p, perm


def degrees(src, dst, num_nodes):
    require_gpu(src, dst)
    ind = torch.empty(num_nodes, dtype=I32, device=src.device)
    outd = torch.empty(num_nodes, dtype=I32, device=src.device)
    check(lib().dn_degrees_i32(num_nodes, src.numel(), ptr(_i32(src, "src")), ptr(_i32(dst, "dst")), ptr(ind), ptr(outd),
                               stream_ptr()), "dn_degrees_i32")
    return ind, outd


def edge_norm(mode, self_loop, src, dst, in_deg, out_deg):
    """RGCN norms (rgcn.py:132-165).  mode 'in' | 'both'.  Returns (in_norm [N,1], out_norm [N,1]|None, edge_norm [E])."""
    require_gpu(src, dst, in_deg, out_deg)
    N, E = in_deg.numel(), src.numel()
    in_norm = torch.empty(N, dtype=torch.float32, device=src.device)
    out_norm = torch.empty(N, dtype=torch.float32, device=src.device) if mode == "both" else None
    en = torch.empty(E, dtype=torch.float32, device=src.device)
    check(lib().dn_edge_norm_f32(1 if mode == "in" else 2, 1 if self_loop else 0, N, E, ptr(src), ptr(dst), ptr(in_deg),
                                 ptr(out_deg), ptr(in_norm), ptr(out_norm), ptr(en), stream_ptr()), "dn_edge_norm_f32")
    return in_norm.view(-1, 1), (out_norm.view(-1, 1) if out_norm is not None else None), en


WGRAD_CHUNK_ROWS = int(_os.environ.get("DN_WGRAD_CHUNK", "4096"))            # step of the chunk tables cut without a look at the relation sizes
# Chunk tables cut WITH the relation sizes (wgrad_chunk_rows, the one-call index, the dense tables) take the smallest chunk for which
# the launch is ONE round of workgroups, up to this many rows (config 5: 775 chunks of 4,096 rows = 3.03 rounds of 256 workgroups and
# 203 MB of partial products became 245 chunks of 12,864 rows and 64 MB: conv weight gradient + reduce 534 -> 473 us, round 6)
WGRAD_CHUNK_CAP = max(WGRAD_CHUNK_ROWS, int(_os.environ.get("DN_WGRAD_CHUNK_CAP", "65536")))


class _ThreadSwitch:
    """The base of every path switch below (f32_exact, dual_fused, ..., attn_fused): a context manager that sets the calling THREAD's
    override in its class's slot to `on`, keeps the value it found and puts it back on exit, also when the body raises.  No override
    (None): the module default holds, read by the *_enabled() function of the switch when it is called.  A subclass with
    _inverse = True writes the opposite value into the slot it inherits (dual_composed / lrp_composed)."""
    _tls = _threading.local()            # one entry per slot in the thread's own dict (reading it there, a miss costs no AttributeError:
    _slot = None                         # f32_mode() runs in every autograd forward)
    _inverse = False

    def __init__(self, on=True):
        self.on = bool(on) != self._inverse

    def __enter__(self):
        mine = self._tls.__dict__
        self.old = mine.get(self._slot)
        mine[self._slot] = self.on
        return self

    def __exit__(self, *exc):
        self._tls.__dict__[self._slot] = self.old
        return False

    @classmethod
    def override(cls, default=None):
        """The calling thread's override of this switch, `default` when there is none."""
        m = cls._tls.__dict__.get(cls._slot)
        return default if m is None else m


# fp32 matrix products: False = 3-term bf16 split on the fast MFMA path (1e-5-level agreement with exact f32, inside the
# reference's 1e-4 bar), True = exact f32 MFMA (1/16 of the bf16 rate; the checker).  F32_EXACT is the PROCESS default (read once
# from the environment; assignable); `with f32_exact(...)` overrides it for the calling THREAD only, and every autograd function
# below records the mode its forward ran in and runs its backward in the same mode -- whatever thread autograd uses for it and
# whether or not the `with` block has been left by then.
F32_EXACT = _os.environ.get("DN_F32_EXACT", "0") == "1"


class f32_exact(_ThreadSwitch):
    """Context manager: run the fp32 matrix kernels inside it on the exact-f32 MFMA (True) or on the bf16 split (False).
    Thread-local; backward passes of work recorded inside it keep the mode (see F32_EXACT)."""
    _slot = "f32_exact"


def f32_mode():
    """The fp32 arithmetic a kernel launched NOW from this thread uses: the thread's f32_exact override, else ops.F32_EXACT."""
    return f32_exact.override(F32_EXACT)


def _backward_in_forward_mode(backward):
    """Decorator of an autograd backward: run it in the fp32 mode its forward recorded (ctx.f32_mode)."""
    def wrapped(ctx, *grads):
        with f32_exact(ctx.f32_mode):
            return backward(ctx, *grads)
    wrapped.__doc__ = backward.__doc__
    return wrapped


def make_row_chunks(rel_ptr_host, device, chunk_rows=None):
    """Split relation-major rows into chunks for dn_rows_wgrad_bf16: (chunks [C,4] int32, chunk_ptr [R+1] int32)."""
    chunk_rows = chunk_rows or WGRAD_CHUNK_ROWS
    chunks, cptr = [], [0]
    for r in range(len(rel_ptr_host) - 1):
        a, b = rel_ptr_host[r], rel_ptr_host[r + 1]
        while a < b:
            e = min(a + chunk_rows, b)
            chunks.append((r, a, e, 0))
            a = e
        cptr.append(len(chunks))
    ch = torch.tensor(chunks if chunks else [(0, 0, 0, 0)], dtype=I32).reshape(-1, 4)
    return ch.to(device), torch.tensor(cptr, dtype=I32).to(device), len(chunks)


INT32_MAX = 0x7fffffff


def rows_wgrad(A, G, chunk_table, num_rels, idx_a=None, idx_g=None, out_dtype=None, A2=None, G2=None, colsum_of=0,
               mask_a=None, a_out=None, mask_a_bits=None, colsum_lp=False, slope=0.0, colsum_rel=None):
    """out[r] = sum_{p in relation r} Acat[idx_a[p]]^T Gcat[idx_g[p]]  (dn_rows_wgrad_bf16; bf16 in, fp32 accumulate).
    Acat = [A; A2], Gcat = [G; G2] (virtual concatenations).  colsum_of = 1|2 additionally returns the fp32 per-relation
    column sums [R, H] of operand A|G (the bias gradient); colsum_lp: return them in out's dtype instead (bf16 output: written
    by the reduce launch itself, so the bias gradient needs no cast launch); colsum_rel (bf16): the column sums of that relation's
    rows only, the other rows of the result are zeros."""
    chunks, chunk_ptr, nchunks = chunk_table
    require_gpu(A, G, idx_a, idx_g, chunks, chunk_ptr, A2, G2, mask_a, a_out, mask_a_bits)
    assert A.dtype == G.dtype and A.dtype in (torch.bfloat16, torch.float32)
    is_f32 = A.dtype == torch.float32
    assert mask_a_bits is None or (not is_f32 and mask_a_bits.dtype == torch.uint8
                                   and mask_a_bits.shape == (A.shape[0], A.shape[1] // 8))
    if is_f32:
        out_dtype = torch.float32
    Hi, Ho = A.shape[1], G.shape[1]
    out_dtype = out_dtype or A.dtype
    out = torch.empty((num_rels, Hi, Ho), dtype=out_dtype, device=A.device)
    ws = _ws(lib().dn_rows_wgrad_workspace_bytes(nchunks, Hi, Ho), A.device)
    colsum = torch.empty((num_rels, Hi), dtype=torch.float32, device=A.device) if colsum_of else None
    # the column sums again in the output dtype (the bias gradient as the parameter wants it): written by the reduce launch
    colsum_lp = (torch.empty((num_rels, Hi), dtype=out_dtype, device=A.device)
                 if (colsum_lp and colsum_of and not is_f32 and out_dtype != torch.float32) else None)

    def _launch():
        na1 = A.shape[0] if A2 is not None else INT32_MAX
        ng1 = G.shape[0] if G2 is not None else INT32_MAX
        if is_f32:
            check(lib().dn_rows_wgrad_f32(ptr(A), ptr(A2), na1, ptr(idx_a), ptr(G), ptr(G2), ng1, ptr(idx_g), Hi, Ho, num_rels,
                                          ptr(chunks), nchunks, ptr(chunk_ptr), ptr(out), int(colsum_of), ptr(colsum),
                                          ptr(mask_a), ptr(a_out), 1 if f32_mode() else 0, float(slope), ptr(ws), ws.numel(), stream_ptr()),
                  "dn_rows_wgrad_f32")
        else:
            check(lib().dn_rows_wgrad_bf16(ptr(A), ptr(A2), na1, ptr(idx_a), ptr(G), ptr(G2), ng1, ptr(idx_g), Hi, Ho, num_rels,
                                           ptr(chunks), nchunks, ptr(chunk_ptr), ptr(out),
                                           1 if out_dtype == torch.float32 else 0,
                                           int(colsum_of) | (((int(colsum_rel) + 1) << 8) if (colsum_of and colsum_rel is not None) else 0),
                                           ptr(colsum), ptr(mask_a),
                                           ptr(a_out), ptr(mask_a_bits), ptr(colsum_lp), float(slope), ptr(ws), ws.numel(), stream_ptr()),
                  "dn_rows_wgrad_bf16")

    launch_tagged("rows_wgrad", _launch)
    if colsum_of:
        return out, (colsum_lp if colsum_lp is not None else colsum)
    return out


def rows_wgrad_multi(jobs, chunk_table, num_rels, H, out_dtype):
    """Several weight gradients in ONE launch + ONE reduce (dn_rows_wgrad_multi_bf16 / _f32 on the bf16 split, H = 64 / 128).  jobs: dicts with A, G
    (and optionally A2, G2, idx_a, idx_g, mask_a_bits, colsum_of, slope), first_rel, row0 -- relations numbered through, rows laid
    end to end in one virtual row space that chunk_table covers.  -> (out [num_rels, H, H], colsum [num_rels, H]) in out_dtype."""
    chunks, chunk_ptr, nchunks = chunk_table
    dev = jobs[0]["A"].device
    arr = (_lib.WgradJob * len(jobs))()
    keep = []
    for k, jb in enumerate(jobs):
        A, G = jb["A"], jb["G"]
        require_gpu(A, G, jb.get("A2"), jb.get("G2"), jb.get("idx_a"), jb.get("idx_g"), jb.get("mask_a_bits"))
        assert A.dtype == G.dtype == jobs[0]["A"].dtype and A.dtype in (torch.bfloat16, torch.float32)
        assert A.shape[1] == G.shape[1] == H and A.is_contiguous() and G.is_contiguous()
        keep.append(jb)
        pv = lambda t: (t.data_ptr() if t is not None else None)  # noqa: E731
        arr[k].A, arr[k].A2, arr[k].idx_a = pv(A), pv(jb.get("A2")), pv(jb.get("idx_a"))
        arr[k].G, arr[k].G2, arr[k].idx_g = pv(G), pv(jb.get("G2")), pv(jb.get("idx_g"))
        arr[k].mask_a_bits = pv(jb.get("mask_a_bits"))
        arr[k].na1 = A.shape[0] if jb.get("A2") is not None else INT32_MAX
        arr[k].ng1 = G.shape[0] if jb.get("G2") is not None else INT32_MAX
        arr[k].colsum_of, arr[k].first_rel, arr[k].row0 = int(jb.get("colsum_of", 0)), int(jb["first_rel"]), int(jb["row0"])
        arr[k].act_slope = float(jb.get("slope", 0.0))
    is_f32 = jobs[0]["A"].dtype == torch.float32
    if is_f32:                                                              # (a job's mask is then the saved activation itself: float [rows, H])
        assert out_dtype == torch.float32 and not f32_mode()
        assert all(jb.get("mask_a_bits") is None or (jb["mask_a_bits"].dtype == torch.float32 and jb["mask_a_bits"].shape == jb["A"].shape
                                                     and jb["mask_a_bits"].is_contiguous()) for jb in jobs)
    out = torch.empty((num_rels, H, H), dtype=out_dtype, device=dev)
    colsum = torch.empty((num_rels, H), dtype=torch.float32, device=dev)
    colsum_lp = torch.empty((num_rels, H), dtype=out_dtype, device=dev) if out_dtype != torch.float32 else None
    ws = _ws(lib().dn_rows_wgrad_workspace_bytes(nchunks, H, H), dev)

    def _launch():
        if is_f32:                                                          # fp32 rows on the 3-term bf16 split
            check(lib().dn_rows_wgrad_multi_f32(arr, len(jobs), H, num_rels, ptr(chunks), nchunks, ptr(chunk_ptr), ptr(out), ptr(colsum),
                                                ptr(ws), ws.numel(), stream_ptr()), "dn_rows_wgrad_multi_f32")
            return
        check(lib().dn_rows_wgrad_multi_bf16(arr, len(jobs), H, num_rels, ptr(chunks), nchunks, ptr(chunk_ptr), ptr(out),
                                             1 if out_dtype == torch.float32 else 0, ptr(colsum), ptr(colsum_lp), ptr(ws), ws.numel(),
                                             stream_ptr()), "dn_rows_wgrad_multi_bf16")
    launch_tagged("rows_wgrad_multi", _launch)
    return out, (colsum_lp if colsum_lp is not None else colsum)


# split-K chunks of the ONE weight-gradient launch of an H = 64 / 128 layer (_RginLayerSmallFn, _RginLayerF32Fn): two rounds' worth of
# workgroups -- a workgroup walks its chunk tile by tile, a dependent chain (22 tiles of 32 rows at config 3 with 256 chunks), and two
# of these small workgroups share a CU: config 3 fp32 0.105 -> 0.100 ms, bf16 0.069 -> 0.068 (1,024: the same)
_SMALL_WG = 512


def wgrad_chunk_rows(rel_ptr_host, workgroups=256):
    """Rows per split-K chunk of the weight gradient over relation-major rows: the smallest multiple of 64 (>= 256) for which the
    chunks of all relations -- every relation ends in a partial chunk -- fit ONE round of `workgroups`; batches too large for
    that (over 256 x WGRAD_CHUNK_CAP rows) keep WGRAD_CHUNK_CAP and run several rounds.  (A 1/8 shard of config 5 cut by rows / 256
    alone made 270 chunks: a second round for 14 workgroups, 138 us instead of 80.)"""
    sizes = [int(b) - int(a) for a, b in zip(rel_ptr_host[:-1], rel_ptr_host[1:]) if int(b) > int(a)]
    total = sum(sizes)
    if total == 0:
        return 256
    c = max(256, -(-total // workgroups // 64) * 64)
    while c < WGRAD_CHUNK_CAP and sum(-(-n // c) for n in sizes) > workgroups:
        c += 64
    return min(c, WGRAD_CHUNK_CAP)


def build_row_tables(rel_ptr_dev, num_rels, num_rows, step, want_ptr=False, skip_mask=0):
    """Tile (step = 32) / chunk tables of relation-major rows built ON THE DEVICE (dn_row_tables_build_i32): returns
    (table [M, 4] int32, M) or (table, piece_ptr [num_rels + 1], M) with M = the upper bound rows / step + num_rels --
    unused entries are empty pieces, which every consumer skips.  skip_mask: bit r leaves relation r out."""
    require_gpu(rel_ptr_dev)
    _i32(rel_ptr_dev, "rel_ptr")
    dev = rel_ptr_dev.device
    M = int(num_rows) // int(step) + int(num_rels) + 1
    table = torch.empty((M, 4), dtype=I32, device=dev)
    pptr = torch.empty(int(num_rels) + 1, dtype=I32, device=dev) if want_ptr else None
    check(lib().dn_row_tables_build_i32(int(num_rels), ptr(rel_ptr_dev), int(step), M, ptr(table), ptr(pptr), int(skip_mask),
                                        stream_ptr()), "dn_row_tables_build_i32")
    return (table, pptr, M) if want_ptr else (table, M)


SWEEP_ENABLED = _os.environ.get("DN_SWEEP", "1") != "0"
SWEEP_WG_PER_GROUP = 32                  # dn_rows_transform_bf16 at H = 256: 256 persistent workgroups = 8 XCDs x 32 CUs
SWEEP_MIN_TILES_PER_WG = 32              # smaller launches fit the L2s anyway


def build_sweep_tables(rel_ptr_dev, num_rels, row_in, row_out, num_nodes, num_rows, skip_mask=0, wg_per_group=SWEEP_WG_PER_GROUP,
                       want_info=False):
    """L2-blocked tile order of relation-major rows for the persistent transform launch (dn_sweep_tables_build_i32; see
    include/dn_hip.h): (table [8 * wg_per_group * S, 4] int32, 8 * wg_per_group * S) -- the pair rows_transform takes.  S is
    sized from what the host knows (rows / 32 + one partial tile per group and relation, 10 % head-room for uneven groups and the
    pure workgroups' quota); when
    a group needs more the builder writes the plain order into the same table (still valid), no read-back."""
    require_gpu(rel_ptr_dev, row_in, row_out)
    _i32(rel_ptr_dev, "rel_ptr"), _i32(row_in, "row_in"), _i32(row_out, "row_out")
    G = 8 * int(wg_per_group)
    S = int(1.10 * (int(num_rows) // 32 + 8 * int(num_rels)) / G) + 4     # (head-room: uneven groups, the pure workgroups' larger quota)
    table = torch.empty((G * S, 4), dtype=I32, device=rel_ptr_dev.device)
    info = torch.empty(2, dtype=I32, device=rel_ptr_dev.device) if want_info else None
    check(lib().dn_sweep_tables_build_i32(int(num_rels), ptr(rel_ptr_dev), ptr(row_in), ptr(row_out), int(num_nodes),
                                          int(wg_per_group), S, int(skip_mask), ptr(table), ptr(info), stream_ptr()),
          "dn_sweep_tables_build_i32")
    return ((table, G * S), info) if want_info else (table, G * S)


def make_row_tiles(rel_ptr_host, device, tile_rows=32):
    """Tile table for dn_rows_transform_bf16: [T,4] int32 rows {rel, beg, end, 0}, tiles never cross relations."""
    import numpy as np
    parts = []
    for r in range(len(rel_ptr_host) - 1):
        a, b = rel_ptr_host[r], rel_ptr_host[r + 1]
        if b > a:
            beg = np.arange(a, b, tile_rows, dtype=np.int64)
            parts.append(np.stack([np.full_like(beg, r), beg, np.minimum(beg + tile_rows, b), np.zeros_like(beg)], 1))
    tl = np.concatenate(parts, 0) if parts else np.zeros((0, 4), dtype=np.int64)
    return torch.from_numpy(tl.astype(np.int32)).to(device), int(tl.shape[0])


def rows_transform(X, Wn, tile_table, num_rows, idx=None, X2=None, bias=None, relu=False, mask_pos=None, tag="dense",
                   out=None, w_kn=False, slope=0.0, W_loop=None, loop_rel=-1, bias_rel=-1):
    """Y[p] = epi(Xcat[idx[p]] @ Wn[rel(p)]^T), zeroed where mask_pos[p] <= 0  (dn_rows_transform_bf16 / _f32).
    w_kn: Wn[r] is given [in][out] (the parameter's own layout; the bf16 H = 256 ring kernel and the fp32 kernels) instead of
    [out][in].  slope: `relu` / `mask_pos` as leaky ReLU (0 = ReLU): relu gives max(v, 0) + slope * min(v, 0), mask_pos
    multiplies by slope instead of zeroing.  fp32 only: W_loop [H, H] serves the tiles of relation `loop_rel` (the self-loop
    parameter, not concatenated behind Wn); bias_rel >= 0: `bias` is one row [H] added to that relation's tiles only."""
    tiles, ntiles = tile_table
    require_gpu(X, Wn, tiles, idx, X2, bias, mask_pos, W_loop)
    assert X.dtype == Wn.dtype and X.dtype in (torch.bfloat16, torch.float32) and Wn.dim() == 3
    assert bias is None or bias.dtype == X.dtype
    assert not w_kn or X.dtype == torch.float32 or (Wn.shape[1] == Wn.shape[2] and Wn.shape[1] in (64, 128, 256))
    assert (W_loop is None and bias_rel < 0) or X.dtype == torch.float32
    assert W_loop is None or (W_loop.dtype == X.dtype and W_loop.shape == Wn.shape[1:] and W_loop.is_contiguous() and loop_rel >= 0)
    assert Wn.is_contiguous() and (bias is None or bias.is_contiguous())
    Ho, Hi = Wn.shape[1], Wn.shape[2]
    assert X.shape[1] == Hi
    if out is None:
        Y = torch.empty((num_rows, Ho), dtype=X.dtype, device=X.device)
    else:
        assert out.is_contiguous() and out.dtype == X.dtype and out.shape[0] >= num_rows and out.shape[1] == Ho
        Y = out[:num_rows]

    def _launch():
        n1 = X.shape[0] if X2 is not None else INT32_MAX
        if X.dtype == torch.float32:
            check(lib().dn_rows_transform_f32(ptr(X), ptr(X2), n1, ptr(idx), Hi, Ho, ptr(Wn), ptr(bias), 1 if relu else 0,
                                              ptr(mask_pos), ptr(tiles), ntiles, ptr(Y), 1 if f32_mode() else 0, float(slope),
                                              ptr(W_loop), int(loop_rel) if W_loop is not None else -1, int(bias_rel),
                                              1 if w_kn else 0, stream_ptr()),
                  "dn_rows_transform_f32")
        else:
            check(lib().dn_rows_transform_bf16(ptr(X), ptr(X2), n1, ptr(idx), Hi, Ho, ptr(Wn), ptr(bias), 1 if relu else 0,
                                               ptr(mask_pos), ptr(tiles), ntiles, ptr(Y), 1 if w_kn else 0, float(slope), stream_ptr()),
                  "dn_rows_transform_bf16")

    launch_tagged("rows_transform:" + tag, _launch)
    return Y


MFMA_DTYPES = (torch.bfloat16, torch.float32)


SELFSUM_SLOTS = 6
SELFSUM_ENABLED = _os.environ.get("DN_SELFSUM", "1") != "0"


# DN_OVER_INSIDE_ROWS: up to this many nodes dn_rows_selfsum_bf16 finishes the nodes with more rows than slots itself (0: never).
# Config-3-shaped batches, H = 64 bf16, step with the walk inside / as its own launch: 25.6 k nodes 0.0985 / 0.1067 ms, 38 k 0.114 /
# 0.118, 51 k 0.123 / 0.127, 77 k 0.151 / 0.150, 102 k 0.182 / 0.175, 410 k 0.533 / 0.485
OVERFLOW_INSIDE_MAX_ROWS = int(_os.environ.get("DN_OVER_INSIDE_ROWS", "65536"))
# ... and only while no node's list is longer than this: the walk inside the slot kernel takes a list one entry at a time (dependent
# loads) while the rest of the workgroup waits at a barrier, so one hub node with thousands of rows would stall its tile's pipeline;
# dn_overflow_rows_add_bf16 ranks 64 entries per round trip
OVERFLOW_INSIDE_MAX_LIST = int(_os.environ.get("DN_OVER_INSIDE_LIST", "64"))


def rows_selfsum(x, Wn, bias, S, S2, slots, out=None, seg=None, lists=None, w_kn=False):
    """out[v] = x[v] @ Wn^T (+ bias) + sum_k Scat[slots[v, k]]  (dn_rows_selfsum_bf16; Scat = S rows then S2 rows).
    seg = (fold_info int32 [ceil(N/32), 12], seg_part fp32 [n_part, H]): also write the per-(segment, tile) column sums of x (the
    folded pre-aggregation, see the header).  lists = (list_ptr, list_rows, num_edge_rows, drop_beg, drop_end, overflow[, longest
    list]): the per-node row lists the slot table was built from -- nodes with more rows than slots (-2 in their last slot) are finished
    from them inside the launch (small batches whose longest list is known and short) or by a second small launch
    (dn_overflow_rows_add_bf16).  w_kn: Wn is given [in][out] (the parameter's own layout) instead."""
    require_gpu(x, Wn, bias, S, S2, slots)
    if seg is not None:
        require_gpu(*seg)
        assert seg[0].dtype == I32 and seg[0].shape == ((x.shape[0] + 31) // 32, 12) and seg[0].is_contiguous()
        assert seg[1].dtype == torch.float32 and seg[1].shape[1] == x.shape[1] and seg[1].is_contiguous()
    N, H = x.shape
    assert x.dtype == torch.bfloat16 and Wn.shape == (H, H) and slots.shape == (N, SELFSUM_SLOTS) and slots.dtype == I32
    x, Wn, slots = x.contiguous(), Wn.contiguous(), slots.contiguous()
    if out is None:
        out = torch.empty((N, H), dtype=x.dtype, device=x.device)
    n1 = int(S.shape[0]) if S2 is not None else 0x7fffffff

    # small batches: the nodes with more rows than slots are finished inside the launch (one launch less); large ones by the
    # overflow launch below (the in-kernel walk stalls the tile pipeline: + 130 us at config 5)
    inside = (lists is not None and N <= OVERFLOW_INSIDE_MAX_ROWS and S is not None and S.numel() > 0
              and len(lists) > 6 and lists[6] is not None and lists[6] <= OVERFLOW_INSIDE_MAX_LIST)
    lin = lists if inside else (None, None, 0, 0, 0, None)

    def _launch():
        check(lib().dn_rows_selfsum_bf16(ptr(x), H, ptr(Wn), ptr(bias), ptr(S) if S is not None and S.numel() else None,
                                         ptr(S2), n1, ptr(slots), SELFSUM_SLOTS, N, ptr(out),
                                         ptr(seg[0]) if seg else None, ptr(seg[1]) if seg else None, 1 if w_kn else 0,
                                         ptr(lin[0]), ptr(lin[1]), int(lin[2]), int(lin[3]), int(lin[4]), stream_ptr()),
              "dn_rows_selfsum_bf16")
    launch_tagged("rows_selfsum", _launch)
    if lists is not None and not inside:
        lp, lr, ner, db, de, over = lists[:6]
        require_gpu(lp, lr, over)
        _i32(lp, "list_ptr"), _i32(lr, "list_rows")
        assert lp.numel() >= N + 1 and S2 is None and over.dtype == torch.uint8 and over.numel() >= N

        def _launch2():
            check(lib().dn_overflow_rows_add_bf16(ptr(S) if S is not None and S.numel() else None, H, ptr(over), SELFSUM_SLOTS, N,
                                                  ptr(lp), ptr(lr), int(ner), int(db), int(de), ptr(out), stream_ptr()),
                  "dn_overflow_rows_add_bf16")
        launch_tagged("overflow_rows_add", _launch2)
    return out


CHAIN2_ENABLED = _os.environ.get("DN_CHAIN2", "1") != "0"


def rows_chain2(x, W1n, b1, relu1, W2n, b2, relu2, mask0_bits=None, mask1_bits=None, want_bits=False, w_kn=(False, False),
                slope=0.0):
    """(Y1, Y2[, bits1, bits2]) with Y1 = epi1(m0(x) @ W1n^T), Y2 = epi2(Y1 @ W2n^T) in one pass over the rows
    (dn_rows_chain2_bf16).  mask*_bits: uint8 [N, H/8] keep-masks (input / stage-1 output); want_bits: also return the
    "> 0" bit tensors of Y1 and Y2 (the ReLU masks the backward needs, 1/16 of the activations).  w_kn[i]: weight i is given
    [in][out] instead of [out][in] (the backward chain on the Linear weights as they are: no transposed copies)."""
    x, W1n, W2n = x.contiguous(), W1n.contiguous(), W2n.contiguous()
    require_gpu(x, W1n, b1, W2n, b2, mask0_bits, mask1_bits)
    N, H = x.shape
    assert x.dtype == torch.bfloat16 and W1n.shape == (H, H) and W2n.shape == (H, H)
    for m in (mask0_bits, mask1_bits):
        assert m is None or (m.dtype == torch.uint8 and m.shape == (N, H // 8))
    Y1, Y2 = torch.empty_like(x), torch.empty_like(x)
    bits1 = torch.empty((N, H // 8), dtype=torch.uint8, device=x.device) if want_bits else None
    bits2 = torch.empty((N, H // 8), dtype=torch.uint8, device=x.device) if want_bits else None

    def _launch():
        check(lib().dn_rows_chain2_bf16(ptr(x), H, ptr(W1n), ptr(b1), 1 if relu1 else 0, ptr(mask0_bits), ptr(mask1_bits),
                                        ptr(W2n), ptr(b2), 1 if relu2 else 0, N, ptr(Y1), ptr(Y2), ptr(bits1), ptr(bits2),
                                        (1 if w_kn[0] else 0) | (2 if w_kn[1] else 0), float(slope), stream_ptr()),
              "dn_rows_chain2_bf16")
    launch_tagged("rows_chain2", _launch)
    return (Y1, Y2, bits1, bits2) if want_bits else (Y1, Y2)


def rows_chain2_f32(x, W1n, b1, relu1, W2n, b2, relu2, mask0=None, mask1=None, w_kn=(False, False), slope=0.0, residual=None):
    """(Y1, Y2) of two dense layers in one pass over fp32 rows (dn_rows_chain2_f32, 3-term split, H = 64 / 128): Y1 = epi1(m0(x) @ W1n^T)
    masked by mask1, Y2 = epi2(Y1 @ W2n^T); mask0 / mask1: float [N, H] saved activations (keep where > 0, else x slope)."""
    x, W1n, W2n = x.contiguous(), W1n.contiguous(), W2n.contiguous()
    require_gpu(x, W1n, b1, W2n, b2, mask0, mask1)
    N, H = x.shape
    require_gpu(residual)
    assert x.dtype == torch.float32 and H in (64, 128) and W1n.shape == (H, H) and W2n.shape == (H, H) and not f32_mode()
    for m in (mask0, mask1):
        assert m is None or (m.dtype == torch.float32 and m.shape == (N, H) and m.is_contiguous())
    Y1, Y2 = torch.empty_like(x), torch.empty_like(x)
    assert residual is None or (residual.dtype == torch.float32 and residual.shape == x.shape and residual.is_contiguous())
    Ysum = torch.empty_like(x) if residual is not None else None      # residual given: also returns Y2 + residual

    def _launch():
        check(lib().dn_rows_chain2_f32(ptr(x), H, ptr(W1n), ptr(b1), 1 if relu1 else 0, ptr(mask0), ptr(mask1), ptr(W2n), ptr(b2),
                                       1 if relu2 else 0, N, ptr(Y1), ptr(Y2), (1 if w_kn[0] else 0) | (2 if w_kn[1] else 0), float(slope),
                                       ptr(residual), ptr(Ysum), stream_ptr()), "dn_rows_chain2_f32")
    launch_tagged("rows_chain2", _launch)
    return (Y1, Y2, Ysum) if residual is not None else (Y1, Y2)


def build_slot_table(list_ptr, list_rows, num_nodes, num_edge_rows, K=SELFSUM_SLOTS, drop=(0, 0), drop_enable=None):
    """Fixed-width view of per-node row lists for dn_rows_selfsum_bf16 (dn_slot_table_build_i32: one launch, no read-back):
    (slots [N, K] int32, overflow [N] uint8).  Rows >= num_edge_rows (the self-loop rows) and rows in drop = (beg, end) are left out (drop_enable: a
    device flag that switches the range off when 0); a node with more than K rows keeps its first K-1 and gets -2 in its last
    slot and 1 in its overflow byte -- a small launch after the closing launch finishes it from the list (pass lists to rows_selfsum)."""
    require_gpu(list_ptr, list_rows)
    dev = list_rows.device
    N, P = int(num_nodes), int(num_edge_rows)
    list_ptr, list_rows = list_ptr.to(I32).contiguous(), list_rows.to(I32).contiguous()
    slots = torch.empty((N, K), dtype=I32, device=dev)
    over = torch.empty(max(N, 1), dtype=torch.uint8, device=dev)
    check(lib().dn_slot_table_build_i32(N, P, K, ptr(list_ptr), ptr(list_rows), int(drop[0]), int(drop[1]), ptr(drop_enable),
                                        ptr(slots), ptr(over), stream_ptr()), "dn_slot_table_build_i32")
    return slots, over


# The closing launch at H = 256 as a stream of 32-row units (csrc/dn_close.hip): no slot limit, no overflow launch.
# DN_CLOSE_RING=0 keeps dn_rows_selfsum_bf16 + dn_overflow_rows_add_bf16 at every width (e.g. to trace a non-finite row: the
# unit kernel turns a NaN / Inf of one product row into NaN for that column of the whole 32-node tile).
CLOSE_RING_ENABLED = _os.environ.get("DN_CLOSE_RING", "1") != "0"


class CloseUnits:
    """Tables of dn_rows_close_bf16 for one direction of a RowIndex (dn_close_units_build_i32)."""
    __slots__ = ("unit_ptr", "units", "ent_row", "ent_mask", "num_wg", "num_nodes", "num_tiles", "agg", "order", "num_segments")


# DN_CLOSE_ORDER=0: the closing launch walks the batch upwards as one front (workgroup w: tiles w, w + G, ...) instead of every XCD
# walking its eighth of the batch downwards -- towards the rows the transform launch in front of it handled last
CLOSE_XCD_ORDER = _os.environ.get("DN_CLOSE_ORDER", "1") != "0"


def _close_order(num_wg):
    return 1 if (CLOSE_XCD_ORDER and num_wg % 8 == 0) else 0


def _num_cus(dev):
    return int(torch.cuda.get_device_properties(dev).multi_processor_count)


def build_graph_tiles(seg_ptr, seg_nodes, num_nodes, ok=None, add_idx=None):
    """Tiles = the graphs of a batch, for the absorbed fold (dn_fold_graph_tiles_build_i32, one launch, no read-back):
    -> (tile_ptr [S + 1], fold_info [S, 12], ok [1] device flag: non-zero when every graph has at most 32 nodes, the
    segments are contiguous ascending runs and -- add_idx [S] given -- every segment's target row lies inside its own tile:
    the AGG unit of a tile is a read-modify-write by the workgroup that stored the tile)."""
    require_gpu(seg_ptr, seg_nodes, add_idx)
    dev = seg_ptr.device
    S = int(seg_ptr.numel()) - 1
    tile_ptr = torch.empty(S + 1, dtype=I32, device=dev)
    info = torch.empty((max(S, 1), 12), dtype=I32, device=dev)
    if ok is None:
        ok = torch.zeros(1, dtype=I32, device=dev)
    assert add_idx is None or (add_idx.dtype == I32 and add_idx.numel() == S and add_idx.is_contiguous())
    check(lib().dn_fold_graph_tiles_build_i32(int(num_nodes), S, ptr(seg_ptr), ptr(seg_nodes), ptr(add_idx), ptr(tile_ptr),
                                              ptr(info), ptr(ok), stream_ptr()), "dn_fold_graph_tiles_build_i32")
    return tile_ptr, info[:S], ok


# DN_CLOSE_SINGLE=0 (experiments): never use the graphs-as-tiles tables of round 4, also where every graph fits one tile
CLOSE_SINGLE_ENABLED = _os.environ.get("DN_CLOSE_SINGLE", "1") != "0"
# DN_CLOSE_MULTI=0: graphs over 32 nodes keep the fp32 partial rows + dn_fold_tail_bf16 (rounds 4-5) instead of the multi-tile absorbed fold
CLOSE_MULTI_ENABLED = _os.environ.get("DN_CLOSE_MULTI", "1") != "0"


# DN_CLOSE_CHUNK_TILES: 32-node tiles per chunk of the chunked closing launch (a chunk = a run of whole graphs that one workgroup
# takes in one piece; every workgroup gets the same number of chunks, dealt in the front order of the single-tile tables)
CLOSE_CHUNK_TILES = int(_os.environ.get("DN_CLOSE_CHUNK_TILES", "16"))


def close_chunks(num_nodes, num_wg):
    """Chunks of a batch for the chunked closing launch: K per workgroup, about CLOSE_CHUNK_TILES tiles each."""
    k = int(round(num_nodes / 32.0 / num_wg / max(CLOSE_CHUNK_TILES, 1)))
    return num_wg * max(1, min(k, 16383 // num_wg))


def build_graph_tiles_multi(seg_ptr, seg_nodes, num_nodes, ok=None, add_idx=None, num_chunks=None):
    """Tiles of a batch of graphs of ANY size for the absorbed fold (dn_fold_graph_tiles_multi_build_i32: three launches, no
    read-back): the batch cut into num_chunks chunks at graph boundaries (one per workgroup of the closing launch), every chunk
    into consecutive 32-node tiles that run across its graphs.
    -> (tile_ptr [cap + 1], fold_info [cap, 12], chunk_tile [C + 1], chunk_graph [C + 1], cap, ok [1] device flag); the number of
    tiles that exist is chunk_tile[C], on the device; cap bounds it."""
    require_gpu(seg_ptr, seg_nodes, add_idx)
    dev = seg_ptr.device
    S, N = int(seg_ptr.numel()) - 1, int(num_nodes)
    C = int(num_chunks) if num_chunks else close_chunks(N, _num_cus(dev))
    cap = int(lib().dn_fold_graph_tiles_multi_capacity(N, C))
    chunk_tile = torch.empty(C + 1, dtype=I32, device=dev)
    chunk_graph = torch.empty(C + 1, dtype=I32, device=dev)
    tile_ptr = torch.empty(cap + 1, dtype=I32, device=dev)
    info = torch.empty((cap, 12), dtype=I32, device=dev)
    if ok is None:
        ok = torch.zeros(1, dtype=I32, device=dev)
    assert add_idx is None or (add_idx.dtype == I32 and add_idx.numel() == S and add_idx.is_contiguous())
    check(lib().dn_fold_graph_tiles_multi_build_i32(N, S, ptr(seg_ptr), ptr(seg_nodes), ptr(add_idx), C, ptr(chunk_tile), ptr(chunk_graph),
                                                    ptr(tile_ptr), ptr(info), cap, ptr(ok), stream_ptr()),
          "dn_fold_graph_tiles_multi_build_i32")
    return tile_ptr, info, chunk_tile, chunk_graph, cap, ok


def build_close_units(list_ptr, list_rows, num_nodes, num_edge_rows, drop=(0, 0), drop_enable=None, num_wg=None, tile_ptr=None,
                      agg=False, order=None, multi=None):
    """Per tile (32-node windows, or the node ranges tile_ptr gives) the distinct kept rows of its nodes' lists + membership
    masks, and the per-workgroup unit records the closing launch streams (three launches, no read-back).  Same filter as
    build_slot_table.  agg: append every workgroup's AGG units (the absorbed fold, tile_ptr from build_graph_tiles).  order: 0 =
    workgroup w takes tiles w, w + G, ...; 1 = every XCD walks its eighth of the batch downwards (include/dn_hip.h); None = 1 when
    the number of workgroups allows it.  multi = (chunk_tile, chunk_graph, cap, num_segments) of build_graph_tiles_multi (with its
    tile_ptr; its num_chunks = K num_wg): orders 2 / 3 -- the chunks are dealt to the workgroups as orders 0 / 1 deal tiles, so a
    graph's tiles stay in one workgroup's stream."""
    require_gpu(list_ptr, list_rows, tile_ptr)
    dev = list_rows.device
    N, P, L = int(num_nodes), int(num_edge_rows), int(list_rows.numel())
    list_ptr, list_rows = list_ptr.to(I32).contiguous(), list_rows.to(I32).contiguous()
    cu = CloseUnits()
    cu.num_wg = int(num_wg) if num_wg else _num_cus(dev)
    cu.num_nodes, cu.agg = N, bool(agg)
    cu.order = _close_order(cu.num_wg) if order is None else int(order)
    cu.num_tiles = T = (int(tile_ptr.numel()) - 1) if tile_ptr is not None else (N + 31) // 32
    cu.num_segments = T
    tg = tf = None
    kper = 0
    if multi is not None:
        tg, tf, cap_t, nseg = multi
        require_gpu(tg, tf)
        kper = (int(tg.numel()) - 1) // cu.num_wg
        assert agg and tile_ptr is not None and cap_t == T and tg.numel() == kper * cu.num_wg + 1 == tf.numel() and kper >= 1
        cu.order, cu.num_segments = 2 + _close_order(cu.num_wg), int(nseg)
    assert not agg or tile_ptr is not None
    cap = int(lib().dn_close_units_capacity(T, L, cu.num_wg))
    cu.unit_ptr = torch.empty(cu.num_wg + 1, dtype=I32, device=dev)
    cu.units = torch.empty((cap, 4), dtype=I32, device=dev)
    cu.ent_row = torch.empty(max(L, 1), dtype=I32, device=dev)
    cu.ent_mask = torch.empty(max(L, 1), dtype=I32, device=dev)
    ws = _ws(lib().dn_close_units_workspace_bytes(T, cu.num_wg), dev)
    check(lib().dn_close_units_build_i32(N, P, cu.num_wg, ptr(tile_ptr), T, 1 if agg else 0, cu.order, ptr(list_ptr), ptr(list_rows), L,
                                         int(drop[0]), int(drop[1]), ptr(drop_enable), ptr(cu.unit_ptr), ptr(cu.units), cap,
                                         ptr(cu.ent_row), ptr(cu.ent_mask), ptr(tg), ptr(tf), kper, ptr(ws), ws.numel(), stream_ptr()),
          "dn_close_units_build_i32")
    return cu


def rows_close(x, W, bias, S, cu, out=None, seg=None, w_kn=False, agg=None):
    """out[v] = x[v] @ W_loop (+ bias) + sum of the rows of S that cu lists for v  (dn_rows_close_bf16, H = 256).
    W: [out, in] (w_kn False, the transposed copy) or [in, out] as the parameter stores it (w_kn True).  seg as in rows_selfsum
    (fp32 partial rows for dn_fold_tail_bf16).  agg = (fold_info [T, 12], W_agg [H, H] in W's layout, aux [S, H] out, agg_idx [S]):
    the absorbed fold -- cu built with build_graph_tiles' (or build_graph_tiles_multi's) tiles and agg=True; aux[j] = the column sum
    of segment j (bf16), out[agg_idx[j]] += aux[j] @ W_agg inside the same launch."""
    require_gpu(x, W, bias, S, cu.unit_ptr, cu.units, cu.ent_row, cu.ent_mask)
    N, H = x.shape
    assert H == 256 and x.dtype == torch.bfloat16 and W.shape == (H, H) and W.dtype == x.dtype and N == cu.num_nodes
    assert S is None or (S.dtype == x.dtype and S.shape[1] == H and S.is_contiguous())
    assert (agg is not None) == cu.agg and not (agg is not None and seg is not None)
    x, W = x.contiguous(), W.contiguous()
    fi = sp = wa = ax = ai = None
    if seg is not None:
        require_gpu(*seg)
        fi, sp = seg
        assert fi.dtype == I32 and fi.shape == (cu.num_tiles, 12) and fi.is_contiguous()
        assert sp.dtype == torch.float32 and sp.shape[1] == H and sp.is_contiguous()
    if agg is not None:
        require_gpu(*agg)
        fi, wa, ax, ai = agg
        assert fi.dtype == I32 and fi.shape == (cu.num_tiles, 12) and fi.is_contiguous()
        assert wa.dtype == x.dtype and wa.shape == (H, H) and wa.is_contiguous()
        assert ax.dtype == x.dtype and ax.shape == (cu.num_segments, H) and ax.is_contiguous()
        assert ai.dtype == I32 and ai.numel() == cu.num_segments and ai.is_contiguous()
    if out is None:
        out = torch.empty((N, H), dtype=x.dtype, device=x.device)

    def _launch():
        check(lib().dn_rows_close_bf16(ptr(x), H, ptr(W), 1 if w_kn else 0, ptr(bias), ptr(S) if S is not None and S.numel() else None,
                                       ptr(cu.unit_ptr), ptr(cu.units), cu.num_wg, ptr(cu.ent_row), ptr(cu.ent_mask), N, ptr(out),
                                       ptr(fi), ptr(sp), ptr(wa), ptr(ax), ptr(ai), stream_ptr()), "dn_rows_close_bf16")
    launch_tagged("rows_close", _launch)
    return out


def wgrad_supported(A, G):
    return A.dtype == G.dtype and A.dtype in MFMA_DTYPES and A.shape[1] == G.shape[1] and A.shape[1] in (64, 128, 256)


# ----------------------------------------------------------------------------------------------
# index structures
# ----------------------------------------------------------------------------------------------
HUB_SPLIT = 64   # segments longer than this are split into chunks summed by separate lane groups


class _SplitCSR:
    """CSR whose long segments ("hubs": the dummy node of a big graph has in-degree n) are taken out of the main pass and
    summed in HUB_SPLIT-entry chunks by separate lane groups, then folded in chunk order (deterministic).  One lane group
    walking a 600-entry segment would otherwise outlast the whole launch (cdna_hip_programming.md, scatter/gather:
    'split lists longer than ... into chunks summed by separate waves')."""

    def __init__(self, ptr, idx, num_segments):
        self.ptr, self.idx, self.num_segments = ptr, idx, int(num_segments)
        self.hub_ids = None
        if idx.numel() == 0:
            return
        deg = (ptr[1:] - ptr[:-1]).long()
        if int(deg.max()) <= HUB_SPLIT:
            return
        dev = ptr.device
        hub = deg > HUB_SPLIT
        hub_ids = torch.nonzero(hub).reshape(-1)
        seg_of_entry = torch.repeat_interleave(torch.arange(self.num_segments, device=dev), deg)
        keep = ~hub[seg_of_entry]
        # main pass: hubs become empty segments
        deg_main = torch.where(hub, torch.zeros_like(deg), deg)
        self.ptr_main = torch.cat([deg_main.new_zeros(1), torch.cumsum(deg_main, 0)]).to(I32)
        self.keep = keep
        # (positions once, so that a scaled sum has no boolean indexing per call: nonzero + host sync, not capturable)
        self.keep_pos, self.hub_pos = torch.nonzero(keep).reshape(-1), torch.nonzero(~keep).reshape(-1)
        self.idx_main = idx[keep].contiguous()
        # hub pass: entries of hub h in HUB_SPLIT-sized chunks
        hdeg = deg[hub_ids]
        nchunk = (hdeg + HUB_SPLIT - 1) // HUB_SPLIT
        self.idx_hub = idx[~keep].contiguous()
        hub_base = torch.cat([hdeg.new_zeros(1), torch.cumsum(hdeg, 0)])[:-1]
        chunk_hub = torch.repeat_interleave(torch.arange(hub_ids.numel(), device=dev), nchunk)
        first_chunk = torch.cat([nchunk.new_zeros(1), torch.cumsum(nchunk, 0)])
        chunk_in_hub = torch.arange(int(first_chunk[-1]), device=dev) - first_chunk[:-1][chunk_hub]
        cbeg = hub_base[chunk_hub] + chunk_in_hub * HUB_SPLIT
        cend = torch.minimum(cbeg + HUB_SPLIT, (hub_base + hdeg)[chunk_hub])
        self.chunk_ptr = torch.cat([cbeg, cend[-1:]]).to(I32)                 # chunks are contiguous in idx_hub
        self.fold_ptr = first_chunk.to(I32)                                   # chunk ranges per hub
        self.hub_ids = hub_ids

    def segsum(self, x, scale=None, self_in=None, self_coef=0.0):
        if self.hub_ids is None:
            return gather_segsum(x, self.idx, self.ptr, self.num_segments, scale=scale, self_in=self_in, self_coef=self_coef)
        sc_main = sc_hub = None
        if scale is not None:
            sc_main, sc_hub = scale.index_select(0, self.keep_pos), scale.index_select(0, self.hub_pos)
        out = gather_segsum(x, self.idx_main, self.ptr_main, self.num_segments, scale=sc_main, self_in=self_in,
                            self_coef=self_coef)
        part = gather_segsum(x, self.idx_hub, self.chunk_ptr, self.chunk_ptr.numel() - 1, scale=sc_hub)
        hub = gather_segsum(part, None, self.fold_ptr)                        # per-hub sum of its chunk partials
        out.index_add_(0, self.hub_ids, hub)                                  # distinct rows: order-independent
        return out


class EdgeIndex:
    """CSR by destination + CSC by source of one batched COO (int32, device resident).
    The one-shot build DGL / torch-scatter hide behind update_all / scatter."""

    def __init__(self, src, dst, num_nodes, node_ptr=None):
        """node_ptr (optional, [G + 1]): the batch's graph boundaries -- with it, fp32 neighbour sums of small graphs run on the
        matrix cores (tile_plan / dn_graph_tile_sum_f32)."""
        require_gpu(src, dst)
        self.num_nodes, self.num_edges = int(num_nodes), int(src.numel())
        self._node_ptr, self._plan = node_ptr, None
        src, dst = src.to(I32).contiguous(), dst.to(I32).contiguous()
        self.src, self.dst = src, dst
        self.in_ptr, self.in_perm = csr_build(dst, num_nodes)
        self.out_ptr, self.out_perm = csr_build(src, num_nodes)
        # neighbour id lists in segment order (row gather of an int column == index_select plumbing)
        self.src_by_dst = gather_rows_i32(src, self.in_perm)
        self.dst_by_src = gather_rows_i32(dst, self.out_perm)
        self.fwd = _SplitCSR(self.in_ptr, self.src_by_dst, num_nodes)
        self.bwd = _SplitCSR(self.out_ptr, self.dst_by_src, num_nodes)
        self._max_bwd = None

    @classmethod
    def from_parts(cls, src, dst, num_nodes, node_ptr, in_ptr, in_perm, src_by_dst, out_ptr, out_perm, dst_by_src, splits=None):
        """The index of a batch whose CSR by destination / CSC by source already exist (loader.PackedGraphs.assemble copies them out
        of the dataset's own, re-based): the six tensors are taken as they are -- int32, what __init__ would have built from
        (src, dst) -- and the hub split and the tile plan are derived from them exactly as there."""
        require_gpu(src, dst, in_ptr, in_perm, src_by_dst, out_ptr, out_perm, dst_by_src)
        self = cls.__new__(cls)
        self.num_nodes, self.num_edges = int(num_nodes), int(src.numel())
        for name, t, n in (("in_ptr", in_ptr, self.num_nodes + 1), ("out_ptr", out_ptr, self.num_nodes + 1), ("in_perm", in_perm, self.num_edges),
                           ("out_perm", out_perm, self.num_edges), ("src_by_dst", src_by_dst, self.num_edges),
                           ("dst_by_src", dst_by_src, self.num_edges)):
            if _i32(t, name).numel() != n:
                raise _lib.DnHipError("%s has %d entries, expected %d" % (name, t.numel(), n))
        self._node_ptr, self._plan = node_ptr, None
        self.src, self.dst = src.to(I32).contiguous(), dst.to(I32).contiguous()
        self.in_ptr, self.in_perm, self.out_ptr, self.out_perm = in_ptr, in_perm, out_ptr, out_perm
        self.src_by_dst, self.dst_by_src = src_by_dst, dst_by_src
        if splits is not None:                                      # (fwd, bwd) hub splits that exist for these very lists: no read-back
            self.fwd, self.bwd = splits
        else:
            self.fwd = _SplitCSR(self.in_ptr, self.src_by_dst, self.num_nodes)
            self.bwd = _SplitCSR(self.out_ptr, self.dst_by_src, self.num_nodes)
        self._max_bwd = None
        return self

    def tile_plan(self):
        """Plan of the matrix-core neighbour sum (dn_graph_tile_sum_f32) for this batch, or None: tiles = greedy runs of whole
        graphs with at most 64 rows (packed by dn_graph_tiles_host from one small copy of the graph boundaries), the rows of larger
        graphs as two row lists per direction for dn_gather_rows_sum_f32 (lists of up to 64 entries: a lane group per row; hubs: a
        workgroup per row).  Built once per batch."""
        if self._plan is None:
            self._plan = _build_tile_plan(self) or False
        return self._plan or None

    def max_backward_index(self):
        """(tptr, tslot, seg_of_slot): CSR slots grouped by the row they gather, and each slot's destination."""
        if self._max_bwd is None:
            tptr, tslot = csr_build(self.src_by_dst, self.num_nodes)
            deg = (self.in_ptr[1:] - self.in_ptr[:-1]).long()
            seg = torch.repeat_interleave(torch.arange(self.num_nodes, device=deg.device, dtype=I32), deg,
                                          output_size=self.num_edges)
            self._max_bwd = (tptr, tslot, seg.contiguous())
        return self._max_bwd


def gather_rows_i32(values, perm):
    return values.index_select(0, perm.long()) if values.numel() else values.clone()


def _check_edge_types(etype, num_rels):
    """Edge types outside [0, num_rels) would index past the mode table / alias another relation's sort key inside the
    index builds (the reference raises IndexError from weight.index_select(0, etype), rgin.py:109): fail loudly instead.
    One fused reduction + a single scalar read-back per index build."""
    if etype.numel() == 0:
        return
    lo, hi = torch.aminmax(etype)
    lo, hi = int(lo), int(hi)
    if lo < 0 or hi >= int(num_rels):
        raise _lib.DnHipError("edge type out of [0, %d): min %d, max %d (with dummy edges the relation count grows by the "
                              "dummy labels, e.g. max_ngel + 2 in the SI flow)" % (int(num_rels), lo, hi))


class RelIndex:
    """(rel, dst)-segment index for aggregate-then-transform RGCN/RGIN (dn_rel_index_build_i32)."""

    def __init__(self, src, dst, etype, num_nodes, num_rels):
        require_gpu(src, dst, etype)
        dev = src.device
        N, R, E = int(num_nodes), int(num_rels), int(src.numel())
        self.num_nodes, self.num_rels, self.num_edges = N, R, E
        _check_edge_types(etype, R)
        src, dst, etype = (t.to(I32).contiguous() for t in (src, dst, etype))
        e32 = lambda n: torch.empty(max(n, 1), dtype=I32, device=dev)  # noqa: E731
        self.perm1, self.src1, seg_ptr, seg_dst = e32(E), e32(E), e32(E + 1), e32(E)
        self.rel_ptr, self.dptr, sperm = e32(R + 1), e32(N + 1), e32(E)
        self.optr, self.operm, self.seg_by_src = e32(N + 1), e32(E), e32(E)
        nbytes = lib().dn_rel_index_workspace_bytes(N, R, E)
        if nbytes == 0:
            check(-2, "dn_rel_index_workspace_bytes")
        ws = _ws(nbytes, dev)
        host_P = ctypes.c_int64(0)
        host_rel = (ctypes.c_int32 * (R + 1))()
        check(lib().dn_rel_index_build_i32(N, R, E, ptr(src), ptr(dst), ptr(etype), ptr(self.perm1), ptr(self.src1),
                                           ptr(seg_ptr), ptr(seg_dst), ptr(self.rel_ptr), ptr(self.dptr), ptr(sperm),
                                           ptr(self.optr), ptr(self.operm), ptr(self.seg_by_src), ctypes.byref(host_P),
                                           host_rel, ptr(ws), ws.numel(), stream_ptr()), "dn_rel_index_build_i32")
        P = int(host_P.value)
        self.num_segments = P
        self.seg_ptr, self.seg_dst, self.sperm = seg_ptr[:P + 1], seg_dst[:P], sperm[:P]
        self.rel_ptr_host = [int(v) for v in host_rel]
        self.perm1, self.src1 = self.perm1[:E], self.src1[:E]
        self.operm, self.seg_by_src = self.operm[:E], self.seg_by_src[:E]
        # chunk / tile tables on the device: split-K chunks of the matrix-core weight gradient, and the tables of the any-width
        # grouped products (dn_rows_gemm_* / dn_rows_wgrad_any_*)
        rel_ptr_d = torch.tensor(self.rel_ptr_host, dtype=I32).to(dev, non_blocking=True)
        self.chunk_table = build_row_tables(rel_ptr_d, R, P, WGRAD_CHUNK_ROWS, want_ptr=True)
        self.gemm_tiles = build_row_tables(rel_ptr_d, R, P, 64)
        self.gemm_chunks = build_row_tables(rel_ptr_d, R, P, 1024, want_ptr=True)


# ----------------------------------------------------------------------------------------------
# autograd operators
# ----------------------------------------------------------------------------------------------
# DN_TILE_SUM=0: graph-local neighbour sums always take the plain gather (dn_gather_segsum_*)
TILE_SUM_ENABLED = _os.environ.get("DN_TILE_SUM", "1") != "0"
TILE_SUM_ROWS = 64
TILE_SUM_MIN_ROWS = int(_os.environ.get("DN_TILE_SUM_MIN_ROWS", "4096"))


class _TilePlan:
    __slots__ = ("dirs", "bad", "checked", "covered")


def _build_tile_plan(index):
    import numpy as np
    node_ptr = index._node_ptr
    if node_ptr is None or int(node_ptr.numel()) < 2 or index.num_nodes == 0:
        return None
    dev = index.src.device
    npt = np.ascontiguousarray(node_ptr.detach().cpu().numpy().astype(np.int32))
    G, N = int(npt.shape[0]) - 1, index.num_nodes
    if int(npt[0]) != 0 or int(npt[-1]) != N or np.any(np.diff(npt) < 0):
        return None
    sizes = np.diff(npt)
    small = sizes <= TILE_SUM_ROWS
    if not np.any(small & (sizes > 0)):
        return None
    buf = np.empty((max(G, 1), 2), dtype=np.int32)
    n = ctypes.c_int64(0)
    check(lib().dn_graph_tiles_host(npt.ctypes.data_as(ctypes.c_void_p), G, TILE_SUM_ROWS, buf.ctypes.data_as(ctypes.c_void_p),
                                    max(G, 1), ctypes.byref(n)), "dn_graph_tiles_host")
    tl = buf[:int(n.value)]
    beg, end = tl[:, 0], tl[:, 1]
    keep = end > beg
    tiles = torch.from_numpy(tl.copy()).to(dev)
    rest = torch.from_numpy(np.flatnonzero(np.repeat(~small, sizes)).astype(np.int32)).to(dev)
    plan = _TilePlan()
    plan.bad = torch.zeros(1, dtype=I32, device=dev)
    plan.checked = False
    plan.covered = int((end[keep] - beg[keep]).sum())
    assert plan.covered + int(rest.numel()) == N
    plan.dirs = {}
    for d, ptr_, idx in (("f", index.in_ptr, index.src_by_dst), ("b", index.out_ptr, index.dst_by_src)):
        rec = graph_tile_records(tiles, ptr_)
        if rest.numel():
            rl = rest.long()
            deg = ptr_[rl + 1] - ptr_[rl]
            recs = torch.stack([rest, ptr_[rl], ptr_[rl + 1], torch.zeros_like(rest)], 1)       # {row, first entry, end entry, 0}
            short, long_ = recs[deg <= 64].contiguous(), recs[deg > 64].contiguous()
        else:
            short = long_ = rest.reshape(0, 4)
        plan.dirs[d] = (rec, short, long_, ptr_, idx)
    return plan


def _tile_sum_ok(x, index, edge_scale):
    # (batches of a few hundred rows are launch-bound: the plain kernel's one launch beats tile + row-list launches there --
    #  config 1, 617 rows: 0.45 vs 0.51 ms per GIN step; config 2, 20 k rows: 0.86 vs 0.83)
    return (TILE_SUM_ENABLED and edge_scale is None and x.dtype == torch.float32 and x.dim() == 2 and x.shape[1] in (64, 128, 256)
            and x.shape[0] == index.num_nodes and index.num_nodes >= TILE_SUM_MIN_ROWS and index.tile_plan() is not None)


def _tile_neighbor_sum(x, index, direction, self_coef):
    """self_coef * x[v] + sum over v's list of x rows: tiles of small graphs on the matrix cores, the rows of larger graphs from
    their row lists.  Same sums as the plain gather up to fp32 summation order (2e-6)."""
    plan = index.tile_plan()
    rec, short, long_, ptr_, idx = plan.dirs[direction]
    out = torch.empty_like(x)
    graph_tile_sum(x, idx, ptr_, rec, self_coef=self_coef, out=out, bad=plan.bad)
    if short.numel():
        gather_rows_sum(x, idx, ptr_, short, False, self_coef, out)
    if long_.numel():
        gather_rows_sum(x, idx, ptr_, long_, True, self_coef, out)
    if not plan.checked:                                            # once per batch: an edge that leaves its tile?
        if int(plan.bad.item()) != 0:
            index._plan = False
            return None
        plan.checked = True
    return out


class _NeighborSum(torch.autograd.Function):
    """agg[v] = self_coef * x[v] + sum_{e: dst(e)=v} w_e x[src(e)]; backward = same kernel on the CSC."""

    @staticmethod
    def forward(ctx, x, index, self_coef, edge_scale):
        x = x.contiguous()
        ctx.index, ctx.self_coef = index, float(self_coef)
        sc_in = sc_out = None
        if edge_scale is not None:
            sc_in = edge_scale.index_select(0, index.in_perm.long())
            sc_out = edge_scale.index_select(0, index.out_perm.long())
        ctx.sc_out = sc_out
        ctx.save_for_backward(x if (edge_scale is not None and ctx.needs_input_grad[3]) else x.new_empty(0))
        if _tile_sum_ok(x, index, edge_scale):
            out = _tile_neighbor_sum(x, index, "f", float(self_coef))
            if out is not None:
                return out
        return index.fwd.segsum(x, scale=sc_in, self_in=x if self_coef != 0.0 else None, self_coef=self_coef)

    @staticmethod
    def backward(ctx, g):
        g = g.contiguous()
        ix = ctx.index
        gx = None
        if ctx.needs_input_grad[0]:
            gx = _tile_neighbor_sum(g, ix, "b", ctx.self_coef) if _tile_sum_ok(g, ix, ctx.sc_out) else None
            if gx is None:
                gx = ix.bwd.segsum(g, scale=ctx.sc_out, self_in=g if ctx.self_coef != 0.0 else None, self_coef=ctx.self_coef)
        gs = None
        if ctx.needs_input_grad[3]:
            (x,) = ctx.saved_tensors
            gs = edge_dot(x, ix.src, g, ix.dst)                 # d out / d w_e = < x[src_e], g[dst_e] >
        return gx, None, None, gs


def neighbor_sum(x, index, self_coef=0.0, edge_scale=None):
    """(self_coef) x_i + sum_{j->i} w_ij x_j  (GIN aggregation gconv.py:212; GCN propagate with w = gcn norm).
    edge_scale [E] fp32 in original edge order; it receives a gradient (dn_edge_dot_*) when it requires one."""
    return _NeighborSum.apply(x, index, self_coef, edge_scale)


class _EdgeSum(torch.autograd.Function):
    """agg[v] = sum_{e: dst(e)=v} w_e ef[e]   (edge rows summed onto their destination: the reduce half of a dual
    message pass, compgcn.py:272 / dmpnn.py:163); backward: g_ef[e] = w_e g[dst(e)] (a row gather)."""

    @staticmethod
    def forward(ctx, ef, index, edge_scale):
        ef = ef.contiguous()
        ctx.index = index
        sc_in = edge_scale.index_select(0, index.in_perm.long()) if edge_scale is not None else None
        ctx.save_for_backward(edge_scale if edge_scale is not None else ef.new_empty(0))
        ctx.has_scale = edge_scale is not None
        return gather_segsum(ef, index.in_perm, index.in_ptr, index.num_nodes, scale=sc_in)

    @staticmethod
    def backward(ctx, g):
        (scale,) = ctx.saved_tensors
        return gather_segsum(g.contiguous(), ctx.index.dst, None, scale=scale if ctx.has_scale else None), None, None


def edge_sum(ef, index, edge_scale=None):
    """sum of (scaled) edge rows per destination node; edge_scale [E] fp32 (no gradient) in edge order."""
    return _EdgeSum.apply(ef, index, edge_scale)


class _GatherRows(torch.autograd.Function):
    """out[i] = x[idx[i]]; backward = deterministic segment sum over the rows that gathered each x row (CSR of idx)."""

    @staticmethod
    def forward(ctx, x, idx, csr):
        ctx.csr, ctx.n = csr, x.shape[0]
        return gather_segsum(x.contiguous(), idx, None)

    @staticmethod
    def backward(ctx, g):
        ptr_, perm = ctx.csr
        return gather_segsum(g.contiguous(), perm, ptr_, ctx.n), None, None


def gather_rows(x, idx, csr=None):
    """x[idx] with a reproducible backward.  csr = csr_build(idx, x.shape[0]) may be passed in when it is cached."""
    idx = idx.to(I32).contiguous()
    if csr is None:
        csr = csr_build(idx, x.shape[0])
    return _GatherRows.apply(x, idx, csr)


def edge_dot(a, ia, b, ib):
    """out[e] = <a[ia[e]], b[ib[e]]>  (dn_edge_dot_*), fp32."""
    require_gpu(a, ia, b, ib)
    assert a.dim() == 2 and b.dim() == 2 and a.shape[1] == b.shape[1] and a.dtype == b.dtype
    _i32(ia, "ia"), _i32(ib, "ib")
    E = ia.numel() if ia is not None else a.shape[0]
    assert (ib.numel() == E) if ib is not None else (b.shape[0] >= E)
    out = torch.empty(E, dtype=torch.float32, device=a.device)
    check(getattr(lib(), "dn_edge_dot_" + _suffix(a))(ptr(a), ptr(ia), ptr(b), ptr(ib), a.shape[1], E, ptr(out), stream_ptr()),
          "dn_edge_dot")
    return out


class _NeighborMax(torch.autograd.Function):
    """out[v, h] = max_{j->v} x[j, h] (0 for isolated v); backward routes each gradient entry to its arg-max source."""

    @staticmethod
    def forward(ctx, x, index):
        x = x.contiguous()
        N, H = index.num_nodes, x.shape[1]
        out = torch.empty((N, H), dtype=x.dtype, device=x.device)
        arg = torch.empty((N, H), dtype=I32, device=x.device)
        check(getattr(lib(), "dn_gather_segmax_" + _suffix(x))(ptr(x), ptr(index.src_by_dst), ptr(index.in_ptr), N, H,
                                                               ptr(out), ptr(arg), stream_ptr()), "dn_gather_segmax")
        ctx.index, ctx.rows = index, x.shape[0]
        ctx.save_for_backward(arg)
        return out

    @staticmethod
    def backward(ctx, g):
        g = g.contiguous()
        (arg,) = ctx.saved_tensors
        tptr, tslot, seg = ctx.index.max_backward_index()
        gin = torch.empty((ctx.rows, g.shape[1]), dtype=g.dtype, device=g.device)
        check(getattr(lib(), "dn_gather_segmax_bwd_" + _suffix(g))(ptr(g), ptr(arg), ptr(tptr), ptr(tslot), ptr(seg),
                                                                   ctx.rows, g.shape[1], ptr(gin), stream_ptr()),
              "dn_gather_segmax_bwd")
        return gin, None


def neighbor_max(x, index):
    require_gpu(x)
    return _NeighborMax.apply(x, index)


def rows_gemm(A, W, tile_table, transpose_w=False, bias=None):
    """Y[rows of relation r] = A[rows] @ W[r] (or W[r]^T) (+ bias[r]) for ANY widths in one launch (dn_rows_gemm_*; rows
    relation-major, 64-row tiles from build_row_tables).  W: [R, K, N], or [R, N, K] with transpose_w; bias: [R, N]."""
    tiles, ntiles = tile_table
    A, W = A.contiguous(), W.contiguous()
    require_gpu(A, W, tiles, bias)
    if bias is not None:
        bias = bias.contiguous()
        assert bias.dtype == A.dtype and bias.numel() == W.shape[0] * (W.shape[1] if transpose_w else W.shape[2])
    K = A.shape[1]
    N = W.shape[1] if transpose_w else W.shape[2]
    assert A.dtype == W.dtype and (W.shape[2] if transpose_w else W.shape[1]) == K
    Y = torch.empty((A.shape[0], N), dtype=A.dtype, device=A.device)
    if A.shape[0] == 0:
        return Y

    def _launch():
        check(getattr(lib(), "dn_rows_gemm_" + _suffix(A))(ptr(A), ptr(W), ptr(bias), K, N, 1 if transpose_w else 0, ptr(tiles),
                                                          ntiles, ptr(Y), stream_ptr()), "dn_rows_gemm")
    launch_tagged("rows_gemm", _launch)
    return Y


def rows_wgrad_any(A, G, chunk_table, num_rels, want_colsum=False):
    """out[r] = sum_{p in relation r} A[p]^T G[p] for ANY widths (dn_rows_wgrad_any_*); want_colsum: also the fp32 column sums
    of A per relation ([R, K]: the bias gradient when A is a Linear layer's output gradient), from the same launches."""
    chunks, chunk_ptr, nchunks = chunk_table
    A, G = A.contiguous(), G.contiguous()
    require_gpu(A, G, chunks, chunk_ptr)
    K, N = A.shape[1], G.shape[1]
    out = torch.empty((num_rels, K, N), dtype=A.dtype, device=A.device)
    cs = torch.empty((num_rels, K), dtype=torch.float32, device=A.device) if want_colsum else None
    ws = _ws(lib().dn_rows_wgrad_any_workspace_bytes(nchunks, K, N), A.device)
    check(getattr(lib(), "dn_rows_wgrad_any_" + _suffix(A))(ptr(A), ptr(G), K, N, num_rels, ptr(chunks), nchunks, ptr(chunk_ptr),
                                                           ptr(out), ptr(cs), ptr(ws), ws.numel(), stream_ptr()), "dn_rows_wgrad_any")
    return (out, cs) if want_colsum else out


class _RelAggTransform(torch.autograd.Function):
    """agg[v] = sum_r ( sum_{e in r, dst=v} s_e x[src_e] ) W_r   (two gather passes + one relation-grouped GEMM launch)."""

    @staticmethod
    def forward(ctx, x, W, index, edge_scale):
        ctx.f32_mode = f32_mode()
        x = x.contiguous()
        W = W.contiguous()
        ix = index
        sc1 = sc_src = None
        if edge_scale is not None:
            sc1 = edge_scale.index_select(0, ix.perm1.long())
            sc_src = edge_scale.index_select(0, ix.operm.long())
        A = gather_segsum(x, ix.src1, ix.seg_ptr, ix.num_segments, scale=sc1)          # [P, in]
        Y = rows_gemm(A, W, ix.gemm_tiles)                                              # [P, out]
        agg = gather_segsum(Y, ix.sperm, ix.dptr, ix.num_nodes)                         # [N, out]
        ctx.index, ctx.sc_src = ix, sc_src
        ctx.save_for_backward(A, W)
        return agg

    @staticmethod
    @_backward_in_forward_mode
    def backward(ctx, g):
        g = g.contiguous()
        A, W = ctx.saved_tensors
        ix = ctx.index
        gY = gather_segsum(g, ix.seg_dst, None)                                         # [P, out] row gather
        gx = gW = None
        if ctx.needs_input_grad[0]:
            gA = rows_gemm(gY, W, ix.gemm_tiles, transpose_w=True)                      # [P, in]
            gx = gather_segsum(gA, ix.seg_by_src, ix.optr, ix.num_nodes, scale=ctx.sc_src)
        if ctx.needs_input_grad[1]:
            if wgrad_supported(A, g):
                # MFMA split-K kernel; gathers the g rows itself (idx_g = segment destinations)
                gW = rows_wgrad(A, g, ix.chunk_table, W.shape[0], idx_g=ix.seg_dst, out_dtype=W.dtype)
            else:
                gW = rows_wgrad_any(A, gY, ix.gemm_chunks, W.shape[0])
        return gx, gW, None, None


def rel_agg_transform(x, W, index, edge_scale=None):
    """Relation-wise message pass: sum over in-edges of x[src] @ W[etype] (rgin.py:102-120,159)."""
    return _RelAggTransform.apply(x, W, index, edge_scale)


class _SegmentReduce(torch.autograd.Function):
    """Per-graph readout over contiguous rows: sum | mean | max."""

    @staticmethod
    def forward(ctx, x, ptr_, kind):
        x = x.contiguous()
        require_gpu(x, ptr_)
        S, H = ptr_.numel() - 1, x.shape[1]
        out = torch.empty((S, H), dtype=x.dtype, device=x.device)
        sfx = _suffix(x)
        ctx.kind, ctx.rows = kind, x.shape[0]
        if kind == "max":
            arg = torch.empty((S, H), dtype=I32, device=x.device)
            check(getattr(lib(), "dn_segment_max_" + sfx)(ptr(x), H, ptr(ptr_), S, ptr(out), ptr(arg), stream_ptr()),
                  "dn_segment_max")
            ctx.save_for_backward(ptr_, arg)
        else:
            check(getattr(lib(), "dn_segment_%s_%s" % (kind, sfx))(ptr(x), H, ptr(ptr_), S, ptr(out), stream_ptr()),
                  "dn_segment_" + kind)
            ctx.save_for_backward(ptr_)
        return out

    @staticmethod
    def backward(ctx, g):
        g = g.contiguous()
        if ctx.kind == "max":
            ptr_, arg = ctx.saved_tensors
            gin = torch.empty((ctx.rows, g.shape[1]), dtype=g.dtype, device=g.device)
            check(getattr(lib(), "dn_segment_max_bwd_" + _suffix(g))(ptr(g), ptr(arg), g.shape[1], ptr(ptr_),
                                                                     ptr_.numel() - 1, ptr(gin), stream_ptr()),
                  "dn_segment_max_bwd")
            return gin, None, None
        (ptr_,) = ctx.saved_tensors
        # broadcast each graph's row back to its nodes: a row gather keyed by the node's graph id (+ 1 / count for the mean)
        seg_of_row, scale = _segment_rows(ptr_, ctx.rows, ctx.kind == "mean")
        gin = gather_segsum(g, seg_of_row, None, scale=scale)
        return gin, None, None


_segment_rows_cache = {}


def _segment_rows(ptr_, rows, want_scale):
    """(graph id of every row [rows] int32, 1 / rows-of-its-graph per row or None) for a batch's graph_ptr -- five small launches,
    kept per ptr tensor (id, version): every readout of every layer and step over the same batch object reuses them."""
    key = (id(ptr_), ptr_._version, int(rows), ptr_.data_ptr())
    hit = _segment_rows_cache.get(key)
    if hit is None or hit[0]() is not ptr_:
        S = ptr_.numel() - 1
        lens = ptr_[1:] - ptr_[:-1]
        seg = torch.repeat_interleave(torch.arange(S, device=ptr_.device, dtype=I32), lens.long(), output_size=int(rows))
        if len(_segment_rows_cache) > 64:
            _segment_rows_cache.clear()
        import weakref
        hit = [weakref.ref(ptr_), seg, None]
        _segment_rows_cache[key] = hit
    if want_scale and hit[2] is None:
        cnt = (ptr_[1:] - ptr_[:-1]).to(torch.float32).clamp(min=1.0)
        hit[2] = (1.0 / cnt).index_select(0, hit[1].long())
    return hit[1], (hit[2] if want_scale else None)


def segment_reduce(x, graph_ptr, kind="sum"):
    """global_add_pool / global_mean_pool / global_max_pool over the batch's contiguous node ranges."""
    assert kind in ("sum", "mean", "max")
    return _SegmentReduce.apply(x, graph_ptr, kind)


# ----------------------------------------------------------------------------------------------
# fused relation-wise message pass on the matrix cores (bf16): row factorisation + MFMA kernels
# ----------------------------------------------------------------------------------------------
# DN_LOCAL_INDEX=0: always the general (sort-based) row-index builder, also for batches with graph boundaries
LOCAL_INDEX_ENABLED = _os.environ.get("DN_LOCAL_INDEX", "1") != "0"
# DN_CONV_INDEX=0: never dn_conv_index_build_i32 -- row index, closing tables, sweep orders and chunk table by their own calls
CONV_INDEX_ENABLED = _os.environ.get("DN_CONV_INDEX", "1") != "0"


class RowDirection(NamedTuple):
    """The tables ONE direction of a pass over a RowIndex reads ('f': the forward pass, 'b': its mirror image)."""
    aux_ptr: torch.Tensor        # pre-aggregation lists of the collapsed relations (AGG forward / TF backward): [n_aux + 1]
    aux_idx: torch.Tensor        # ... their entries
    n_aux: int
    rows_in: torch.Tensor        # the row every row of the set gathers (row_in forward, row_out backward)
    rows_out: torch.Tensor       # ... and the row its product is added to
    list_ptr: torch.Tensor       # per node, the rows added to it: [N + 1]
    list_rows: torch.Tensor


class _Absorbed(NamedTuple):
    """What the graph-local builders report per direction on the ABSORBED fold (a graph = a segment of the collapsed relation)."""
    tile_ptr: torch.Tensor       # [G + 1] graph tiles
    fold_info: torch.Tensor      # [G, 12]
    verdict: int                 # bit 0: every block within 32 nodes; bit 1: valid without that limit


class _ConvPlan(NamedTuple):
    """What dn_conv_index_build_i32 left behind beside the row index (RowIndex._adopt_plan hands it on to _fold / _units)."""
    units: list                  # CloseUnits of 'f' / 'b': the unit streams of both closing launches
    sweeps: list                 # per direction the sweep order (tiles, #tiles), or None
    chunk_table: tuple           # (chunks, chunk_ptr, #chunks) of the weight gradient
    served: tuple                # per direction 0: not served, 1: every graph within one tile, 2: the chunked (multi-tile) form
    multi_views: object          # k -> (chunk_tile, chunk_graph, tile_ptr, fold_info) of direction k's chunked form
    multi_tiles: int             # ... and its tile count


class _IndexBuffers:
    """Output tables of the row-index builders, allocated ONCE: whichever builder serves the batch fills the same buffers.  G (a batch
    with graph boundaries): also what the graph-local builders write on top -- their status, the relation offsets as they leave them
    on the device, the absorbed-fold verdicts + graph tiles of both directions (same call, same read-back)."""

    def __init__(self, N, R, E, dev, G=None):
        self.e32 = e32 = lambda n: torch.empty(max(int(n), 1), dtype=I32, device=dev)  # noqa: E731
        self.row_in, self.row_out = e32(E + N), e32(E + N)
        self.aux_f_ptr, self.aux_f_idx, self.aux_b_ptr, self.aux_b_idx = e32(E + 1), e32(E), e32(E + 1), e32(E)
        self.dst_ptr, self.dst_rows, self.src_ptr, self.src_rows = e32(N + 2), e32(2 * E + N), e32(N + 2), e32(2 * E + N)
        self.counts = (ctypes.c_int64 * 5)()
        self.host_rel = (ctypes.c_int32 * (R + 1))()
        self.host_modes = (ctypes.c_int32 * R)()
        if G is not None:
            self.rel_dev = e32(R + 2)
            self.graph_tiles = [(e32(G + 1), torch.empty((max(G, 1), 12), dtype=I32, device=dev)) for _ in range(2)]
            self.host_absorb = (ctypes.c_int32 * 4)()              # fold verdicts f / b, the largest graph's nodes / edges
            self.status, gt = ctypes.c_int32(0), self.graph_tiles
            self.local_args = (ctypes.byref(self.status), ptr(self.rel_dev), ptr(gt[0][0]), ptr(gt[0][1]), ptr(gt[1][0]), ptr(gt[1][1]),
                               self.host_absorb)
        # the tables in the order every builder takes them
        self.args = (ptr(self.row_in), ptr(self.row_out), ptr(self.aux_f_ptr), ptr(self.aux_f_idx), ptr(self.aux_b_ptr), ptr(self.aux_b_idx),
                     ptr(self.dst_ptr), ptr(self.dst_rows), ptr(self.src_ptr), ptr(self.src_rows), self.counts, self.host_rel, self.host_modes)


class RowIndex:
    """Relation-major ROW FACTORISATION of  out[v] = sum_{e: dst(e)=v} x[src(e)] W[etype(e)]  (+ x[v] W_loop).

    Every row p has ONE input row and its product Y[p] = in_row(p) @ W[rel(p)] is added to one or more outputs:
      EDGE relation (few shared endpoints):  one row per edge          in = x[src],            out -> dst
      AGG  relation (few distinct dst, e.g. u -> dummy):  row per dst   in = sum_e x[src_e] (aux, pre-aggregated), out -> dst
      TF   relation (few distinct src, e.g. dummy -> u):  row per src   in = x[src],            out -> every dst_e
      self loop (optional, relation id R):   row per node              in = x[v],              out -> v
    so the matrix cores transform min(#edges, #distinct dst, #distinct src) rows per relation, and the dummy
    relations (2n of the m+2n edges of a dummy-augmented graph) collapse to one row per graph each.
    The backward pass is the mirror image (in <-> out lists, W transposed)."""

    EDGE, AGG, TF = 0, 1, 2

    def __init__(self, src, dst, etype, num_nodes, num_rels, self_loop=True, edge_frac=0.75, node_ptr=None, edge_ptr=None,
                 closing_hint=None):
        """One C-ABI call + device-side tile tables.  With the batch's graph boundaries (node_ptr / edge_ptr, [G+1] each) a
        graph-local builder runs -- _build_one_call where closing_hint, the (H, dtype) of the rows the index will serve, is
        (256, bfloat16), else _build_local; without them, or when the batch does not qualify (a graph of 8192 edges or more, more
        than 64 relations), the general one (_build_general).  All produce the same tables bit for bit."""
        require_gpu(src, dst, etype)
        N, R, E = int(num_nodes), int(num_rels), int(src.numel())
        self.num_nodes, self.num_rels, self.num_edges, self.self_loop = N, R, E, bool(self_loop)
        self.built_by = "general"                                     # which builder served the batch: "local" (either graph-local call) / "general"
        self.max_graph = None                                         # local builders: (nodes, edges) of the batch's largest graph
        self.raw = None                                               # ... and (src, dst, etype, node_ptr, edge_ptr) int32
        self._absorb = None                                           # ... and {direction: _Absorbed}
        self._cg_err = None                                           # error / statistics words of the whole-graph launches (_graphs_err)
        self._layer_chunks = {}                                       # virtual-row chunk tables of the layer functions, by cut (layer_wgrad)
        try_local = node_ptr is not None and edge_ptr is not None and R <= 64 and LOCAL_INDEX_ENABLED
        G = int(node_ptr.numel()) - 1 if try_local else None
        if try_local:                                                 # (graphs over the LDS limit: do not even try)
            try_local = E == 0 or E < 8192 * G
        if not try_local:
            _check_edge_types(etype, R)                               # (the local builders validate on the device)
        src, dst, etype = (t.to(I32).contiguous() for t in (src, dst, etype))
        bufs, plan = _IndexBuffers(N, R, E, src.device, G if try_local else None), None
        if try_local:
            require_gpu(node_ptr, edge_ptr)
            batch = (src, dst, etype, node_ptr.to(I32).contiguous(), edge_ptr.to(I32).contiguous())
            assert G >= 0 and int(batch[4].numel()) == G + 1
            if self._one_call_wanted(closing_hint, G):                # (a batch this call turns down goes to the general builder)
                plan = self._build_one_call(bufs, batch, edge_frac)
                served = plan is not None
            else:
                served = self._build_local(bufs, batch, edge_frac)
            if not served:
                _check_edge_types(etype, R)
        if self.built_by == "general":
            self._build_general(bufs, src, dst, etype, edge_frac)
        self._publish(bufs)
        # one workgroup per CU (the LDS-DMA ring fills a CU's LDS) for the split-K weight gradient whatever the batch size:
        # the smallest chunk that keeps ALL relations' chunks (each relation ends in a partial one) within one round of 256
        if plan is not None:
            self._adopt_plan(plan)
        else:
            self.chunk_table = build_row_tables(self.rel_ptr_dev, self.num_all_rels, self.num_rows, wgrad_chunk_rows(self.rel_ptr_host),
                                                want_ptr=True)

    def _one_call_wanted(self, closing_hint, G):
        return (CONV_INDEX_ENABLED and CLOSE_SINGLE_ENABLED and closing_hint is not None and closing_hint[0] == 256
                and closing_hint[1] == torch.bfloat16 and self.self_loop and G >= 1 and self.num_nodes >= 1 and CLOSE_RING_ENABLED
                and CLOSE_AGG_ENABLED and FOLD_ENABLED)

    def _served_by_local(self, bufs, batch):
        """Did the graph-local builder that just ran serve the batch?  If so: what either leaves on the index beside the tables."""
        if bufs.status.value != 0:
            return False
        self.built_by = "local"
        self._absorb = {d: _Absorbed(bufs.graph_tiles[k][0], bufs.graph_tiles[k][1], int(bufs.host_absorb[k]))
                        for k, d in enumerate(("f", "b"))}
        self.max_graph = (int(bufs.host_absorb[2]), int(bufs.host_absorb[3]))
        self.raw = batch                                              # the batch itself, for the launches that take graphs whole
        return True

    def _build_one_call(self, bufs, batch, edge_frac):
        """dn_conv_index_build_i32: the WHOLE per-batch index of the H = 256 bf16 conv -- row index, unit streams of both closing
        launches, sweep orders, weight-gradient chunk table -- in one call with one read-back; whatever it could not serve is built on
        first use.  -> the _ConvPlan it left behind, or None where it did not serve the batch."""
        src, dst, etype, node_ptr, edge_ptr = batch
        N, R, E, dev, e32 = self.num_nodes, self.num_rels, self.num_edges, src.device, bufs.e32
        G = int(node_ptr.numel()) - 1
        num_wg = _num_cus(dev)
        # (a graph over 32 nodes: the same call builds the chunked tiles and their unit streams instead; which, is decided on the device)
        kper = close_chunks(N, num_wg) // num_wg if CLOSE_MULTI_ENABLED else 0
        tcap = int(lib().dn_fold_graph_tiles_multi_capacity(N, kper * num_wg)) if kper else 0
        nbytes = lib().dn_conv_index_workspace_bytes(G, N, R, E, num_wg, tcap)
        if not nbytes:
            return None
        cap = int(lib().dn_close_units_capacity(max(G, tcap), E + N, num_wg))
        # the chunked form's eight tables out of ONE allocation (most batches never look at them: views are made on demand)
        mt_sizes = (kper * num_wg + 1, kper * num_wg + 1, tcap + 1, 12 * max(tcap, 1))
        mt_off, acc = [], 0
        for _ in range(2):
            for n_ in mt_sizes:
                mt_off.append(acc)
                acc += (n_ + 3) // 4 * 4                                # (16-byte aligned pieces)
        mt_arena = e32(acc) if kper else None
        mt_ptr = [ctypes.c_void_p(mt_arena.data_ptr() + 4 * o) if kper else None for o in mt_off]

        def mt_views(k):
            o = mt_off[4 * k:4 * k + 4]
            return (mt_arena[o[0]:o[0] + mt_sizes[0]], mt_arena[o[1]:o[1] + mt_sizes[1]], mt_arena[o[2]:o[2] + mt_sizes[2]],
                    mt_arena[o[3]:o[3] + mt_sizes[3]].view(max(tcap, 1), 12))
        cus = []
        for _ in range(2):
            cu = CloseUnits()
            cu.num_wg, cu.num_nodes, cu.agg, cu.num_tiles, cu.order, cu.num_segments = num_wg, N, True, G, _close_order(num_wg), G
            cu.unit_ptr, cu.units = e32(num_wg + 1), torch.empty((cap, 4), dtype=I32, device=dev)
            cu.ent_row, cu.ent_mask = e32(E + N), e32(E + N)
            cus.append(cu)
        Gw = 8 * SWEEP_WG_PER_GROUP
        want_sweep = SWEEP_ENABLED and E // 32 >= Gw * SWEEP_MIN_TILES_PER_WG
        S = int(1.10 * (E // 32 + 8 * R) / Gw) + 4 if want_sweep else 0
        sweeps = [torch.empty((Gw * S, 4), dtype=I32, device=dev) for _ in range(2)] if want_sweep else [None, None]
        chunk_cap = (E + N) // 256 + R + 3
        chunk_tab, chunk_pp = torch.empty((chunk_cap, 4), dtype=I32, device=dev), e32(R + 2)
        host_plan = (ctypes.c_int32 * 6)()                             # [0], [1]: served f / b; [3]: #chunks; [4], [5]: sweep slots f / b
        ws = _ws(nbytes, dev)
        check(lib().dn_conv_index_build_i32(
            G, N, R, E, ptr(node_ptr), ptr(edge_ptr), ptr(src), ptr(dst), ptr(etype), 1, float(edge_frac), *bufs.args,
            *bufs.local_args, num_wg, cus[0].order, cap, ptr(cus[0].unit_ptr),
            ptr(cus[0].units), ptr(cus[0].ent_row), ptr(cus[0].ent_mask), ptr(cus[1].unit_ptr), ptr(cus[1].units),
            ptr(cus[1].ent_row), ptr(cus[1].ent_mask), kper, tcap, *mt_ptr, SWEEP_WG_PER_GROUP, S, ptr(sweeps[0]), ptr(sweeps[1]), 256,
            WGRAD_CHUNK_CAP, chunk_cap, ptr(chunk_tab), ptr(chunk_pp), host_plan, ptr(ws), ws.numel(), stream_ptr()),
            "dn_conv_index_build_i32")
        if not self._served_by_local(bufs, batch):
            return None
        # (the sweep tables were sized by a bound; the builder laid them out with the slots they need)
        sw = [(sweeps[k][:Gw * host_plan[4 + k]], Gw * int(host_plan[4 + k])) if want_sweep and host_plan[4 + k] > 0 else None
              for k in range(2)]
        return _ConvPlan(units=cus, sweeps=sw, chunk_table=(chunk_tab, chunk_pp, int(host_plan[3])),
                         served=(int(host_plan[0]), int(host_plan[1])), multi_views=mt_views, multi_tiles=tcap)

    def _build_local(self, bufs, batch, edge_frac):
        """dn_row_index_build_local_i32: one wavefront rank-sorts one graph in LDS, one scan.  -> did it serve the batch?"""
        src, dst, etype, node_ptr, edge_ptr = batch
        N, R, E = self.num_nodes, self.num_rels, self.num_edges
        G = int(node_ptr.numel()) - 1
        nbytes = lib().dn_row_index_local_workspace_bytes(G, N, R, E)
        if not nbytes:
            return False
        ws = _ws(nbytes, src.device)
        check(lib().dn_row_index_build_local_i32(G, N, R, E, ptr(node_ptr), ptr(edge_ptr), ptr(src), ptr(dst), ptr(etype),
                                                 1 if self.self_loop else 0, float(edge_frac), *bufs.args, *bufs.local_args,
                                                 ptr(ws), ws.numel(), stream_ptr()),
              "dn_row_index_build_local_i32")
        return self._served_by_local(bufs, batch)

    def _build_general(self, bufs, src, dst, etype, edge_frac):
        """dn_row_index_build_i32: stable radix sorts + scans over the whole batch; serves every batch (edge types checked on the host)."""
        N, R, E = self.num_nodes, self.num_rels, self.num_edges
        nbytes = lib().dn_row_index_workspace_bytes(N, R, E)
        if nbytes == 0:
            check(-2, "dn_row_index_workspace_bytes")
        ws = _ws(nbytes, src.device)
        check(lib().dn_row_index_build_i32(N, R, E, ptr(src), ptr(dst), ptr(etype), 1 if self.self_loop else 0, float(edge_frac),
                                           *bufs.args, ptr(ws), ws.numel(), stream_ptr()), "dn_row_index_build_i32")

    def _publish(self, bufs):
        """The builder's tables, cut to the sizes it reported, as the index's attributes."""
        N, R, E, self_loop = self.num_nodes, self.num_rels, self.num_edges, self.self_loop
        P, n_agg, n_tf, n_agg_e, n_tf_e = (int(v) for v in bufs.counts)
        self.modes = [int(m) for m in bufs.host_modes]
        rel_ptr = [int(v) for v in bufs.host_rel]
        P_all = P + (N if self_loop else 0)
        if self_loop:
            rel_ptr.append(P_all)
        self.num_aux_f, self.num_aux_b = n_agg, n_tf
        self.aux_f_ptr, self.aux_f_idx = bufs.aux_f_ptr[:n_agg + 1], bufs.aux_f_idx[:max(n_agg_e, 1)][:n_agg_e]
        self.aux_b_ptr, self.aux_b_idx = bufs.aux_b_ptr[:n_tf + 1], bufs.aux_b_idx[:max(n_tf_e, 1)][:n_tf_e]
        n_f = (E - n_agg_e) + n_agg + (N if self_loop else 0)      # forward list entries; the rest sits in the discard segment
        n_b = (E - n_tf_e) + n_tf + (N if self_loop else 0)
        self.dst_ptr, self.dst_rows = bufs.dst_ptr[:N + 1], bufs.dst_rows[:n_f]
        self.src_ptr, self.src_rows = bufs.src_ptr[:N + 1], bufs.src_rows[:n_b]
        self.row_in, self.row_out = bufs.row_in[:P_all], bufs.row_out[:P_all]
        self.num_rows, self.num_edge_rows = P_all, P
        self.num_all_rels = R + (1 if self_loop else 0)
        self.rel_ptr_host = rel_ptr
        # tile / chunk tables on the device (the 18 relation offsets go up in one small copy; no host loops)
        if self.built_by == "local":                                 # (already on the device: no upload)
            self.rel_ptr_dev = bufs.rel_dev[:len(rel_ptr)]
        else:
            self.rel_ptr_dev = torch.tensor(rel_ptr, dtype=I32).to(self.row_in.device, non_blocking=True)
        #                                                              (reused by the fold tables: one upload per batch)
        self._tile_table = self._edge_tile_table = None             # built on first use: the folded bf16 path needs neither
        self._slots, self._units, self._fold = {}, {}, {}
        self.dirs = {"f": RowDirection(self.aux_f_ptr, self.aux_f_idx, n_agg, self.row_in, self.row_out, self.dst_ptr, self.dst_rows),
                     "b": RowDirection(self.aux_b_ptr, self.aux_b_idx, n_tf, self.row_out, self.row_in, self.src_ptr, self.src_rows)}

    @property
    def tile_table(self):
        """Tile table of ALL rows (the self loop as relation R): the path without the fused closing launch."""
        if self._tile_table is None:
            self._tile_table = build_row_tables(self.rel_ptr_dev, self.num_all_rels, self.num_rows, 32)
        return self._tile_table

    @property
    def edge_tile_table(self):
        """Tile table of the edge rows (relations 0 .. R-1): closing launch without a folded relation."""
        if not self.self_loop:
            return self.tile_table
        if self._edge_tile_table is None:
            self._edge_tile_table = build_row_tables(self.rel_ptr_dev, self.num_rels, self.num_edge_rows, 32)
        return self._edge_tile_table

    def slots(self, direction):
        """Slot tables for the fused closing launch ('f': rows into each destination, 'b': rows out of each source).
        The rows of a FOLDED relation (_row_index_fold) are left out: they are added by the tail launches."""
        _closing_tables(self, "slots")
        return self._slots[direction]

    def close_units(self, direction):
        """The same lists as the unit stream of dn_rows_close_bf16 (H = 256)."""
        _closing_tables(self, "units")
        return self._units[direction]

    def _adopt_plan(self, plan):
        """The one-call plan as the index's own tables: the chunk table always; the fold verdicts (_fold) and unit streams (_units)
        where the call served BOTH directions -- nothing is then left for the first step."""
        self.chunk_table = plan.chunk_table
        if not (plan.served[0] and plan.served[1]):
            return
        G = int(self.raw[3].numel()) - 1
        cands = {d: _fold_candidate(self, d) for d in ("f", "b")}
        assert cands["f"] is not None and cands["b"] is not None and cands["f"][3] == cands["b"][3] == G
        for k, d in enumerate(("f", "b")):
            info, cu = _Fold(self, d, cands[d]), plan.units[k]
            if plan.served[k] == 2:                                  # a graph over 32 nodes: the call left the chunked form behind
                ct, cg, tpm, fim = plan.multi_views(k)
                info.graph_tiles = (tpm, fim)
                info.multi = (ct, cg, plan.multi_tiles, G)
                cu.order, cu.num_tiles = 2 + _close_order(cu.num_wg), plan.multi_tiles
            else:
                info.graph_tiles = (self._absorb[d].tile_ptr, self._absorb[d].fold_info)
            if plan.sweeps[k] is not None and _sweep_wanted(self):
                info.sweep_tiles = plan.sweeps[k]
            self._fold[d] = info
            self._units[d] = cu


def _sweep_wanted(ix):
    """Is the batch large enough for the L2-blocked order to matter (smaller launches fit the L2s anyway)?"""
    return (SWEEP_ENABLED and ix.num_rels <= 64
            and ix.num_edge_rows // 32 >= 8 * SWEEP_WG_PER_GROUP * SWEEP_MIN_TILES_PER_WG)


def _conv_tiles_for(ix, fold, H, dtype):
    """Tile table of the edge rows (minus the folded relation) for the conv's transform launch: the L2-blocked sweep order when
    the persistent H = 256 bf16 launch will walk it and the batch is large enough for the order to matter (built once per
    index and direction, on first use), else the plain relation-major tiles."""
    P, R = ix.num_edge_rows, ix.num_rels
    if not (dtype == torch.bfloat16 and H == 256 and _sweep_wanted(ix)):
        if fold.main_tiles is None:                                  # (built on first use: a batch on the sweep order never needs them)
            fold.main_tiles = build_row_tables(ix.rel_ptr_dev, ix.num_rels, ix.num_edge_rows, 32, skip_mask=1 << fold.rel)
        return fold.main_tiles
    if fold.sweep_tiles is None:
        fold.sweep_tiles = build_sweep_tables(ix.rel_ptr_dev, R, ix.row_in, ix.row_out, ix.num_nodes, P, skip_mask=1 << fold.rel)
    return fold.sweep_tiles


def prepare_closing(ix, H, dtype):
    """Every table message_pass would build lazily on a batch's first step -- the closing tables of both directions (slot tables
    or unit streams, fold tables) and the sweep tile orders -- so that a loop can account the per-batch index cost outside the
    step (bench.py's index_build_ms, the overlapped fresh-batch leg)."""
    _closing_tables(ix, _close_kind(H, dtype))
    for d in ("f", "b"):
        if ix._fold[d] is not None:
            _conv_tiles_for(ix, ix._fold[d], H, dtype)


def _fold_candidate(ix, direction):
    """(relation, first row, end row, #aux lists) of the one collapsed relation whose pre-aggregation the closing launch could
    absorb in this direction (AGG forward / TF backward), or None -- decided from what the host already knows."""
    mode = RowIndex.AGG if direction == "f" else RowIndex.TF
    n_aux = ix.dirs[direction].n_aux
    rels = [r for r, m in enumerate(ix.modes) if m == mode and ix.rel_ptr_host[r + 1] > ix.rel_ptr_host[r]]
    if not (FOLD_ENABLED and ix.self_loop and len(rels) == 1 and ix.num_rels <= 64 and n_aux > 0):
        return None
    r = rels[0]
    beg, end = ix.rel_ptr_host[r], ix.rel_ptr_host[r + 1]
    return (r, beg, end, n_aux) if end - beg == n_aux else None


# DN_CLOSE_AGG=0: keep the fp32 partial rows + dn_fold_tail_bf16 even where every graph fits one tile of the unit stream
CLOSE_AGG_ENABLED = _os.environ.get("DN_CLOSE_AGG", "1") != "0"


def _fold_add_idx(ix, direction, cand):
    """The node every segment's product is added to: the folded relation's rows' outputs (forward) / inputs (backward)."""
    return ix.dirs[direction].rows_out[cand[1]:cand[2]].contiguous()


def _queue_fold_tables(ix, direction, n_aux, flag):
    """dn_fold_tables_build_async_i32 for one direction (32-node tiles, fp32 partial rows): -> (fold_info, part_ptr); verdict in flag."""
    N, dev = ix.num_nodes, ix.row_in.device
    fold_info = torch.empty(((N + 31) // 32, 12), dtype=I32, device=dev)
    part_ptr = torch.empty(n_aux + 1, dtype=I32, device=dev)
    ws = _ws(lib().dn_fold_tables_workspace_bytes(n_aux), dev)
    check(lib().dn_fold_tables_build_async_i32(N, n_aux, ptr(ix.dirs[direction].aux_ptr), ptr(ix.dirs[direction].aux_idx), ptr(fold_info), ptr(part_ptr),
                                               ptr(flag), ptr(ws), ws.numel(), stream_ptr()), "dn_fold_tables_build_async_i32")
    return fold_info, part_ptr


def _late_fold_tables(ix, direction, info):
    """The 32-node-tile fold tables (fp32 partial rows) of a direction whose fold had been ABSORBED so far (a second closing kind on
    the same index).  The builder repeats the contiguity test the graph tiles passed, so its verdict must be "valid": it is read back
    and checked here instead of being handed on as a device flag that the slot builder honours and the overflow finishers (which drop
    the folded rows unconditionally) would not."""
    flag = torch.zeros(1, dtype=I32, device=ix.row_in.device)
    info.fold_info, info.part_ptr = _queue_fold_tables(ix, direction, info.n, flag)
    if int(flag.item()) == 0:
        raise _lib.DnHipError("fold tables of direction %r are invalid although the graph tiles of the same segments were valid" % direction)


def _decide_folds(ix, kind, before_readback=None):
    """The fold of BOTH directions, decided on the first closing kind an index serves: fills ix._fold[d] with the tables of the
    outcome each direction got (None where there is no candidate or every builder turned it down):
      absorbed, single tile   every graph within one 32-node tile (kind "units"): the verdict of the graph-local index builder
                              (ix._absorb), else dn_fold_graph_tiles_build_i32 and one read-back
      absorbed, multi tile    a graph over 32 nodes whose segments pass the same test without the size limit (kind "units")
      partial rows            32-node-tile fold tables, fp32 partial rows + dn_fold_tail_bf16 (dn_fold_tables_build_async_i32)
    before_readback(cands, flags), if given, runs when every builder is queued and before the host reads the last verdicts: the
    slot tables read theirs on the device."""
    N, dev, dirs = ix.num_nodes, ix.row_in.device, ("f", "b")
    cands = {d: _fold_candidate(ix, d) for d in dirs}
    flags = torch.zeros(4, dtype=I32, device=dev)                    # [parts_f, parts_b, graph_tiles_f, graph_tiles_b]
    absorb = kind == "units" and CLOSE_AGG_ENABLED
    single_tiles, single = {}, {d: False for d in dirs}
    if absorb and ix._absorb is not None:
        # the graph-local index builder answered "can the fold be absorbed?" itself (same candidate rule, same test) and its
        # verdicts came back with its one read-back: no launch, no synchronisation here
        for d in dirs:
            if cands[d] is not None:
                a, n = ix._absorb[d], cands[d][3]
                single_tiles[d] = (a.tile_ptr[:n + 1], a.fold_info[:n])
                single[d] = bool(a.verdict & 1)
    elif absorb:
        for k, d in enumerate(dirs):
            if cands[d] is not None:
                single_tiles[d] = build_graph_tiles(ix.dirs[d].aux_ptr[:cands[d][3] + 1].contiguous(), ix.dirs[d].aux_idx, N,
                                                    ok=flags[2 + k:], add_idx=_fold_add_idx(ix, d, cands[d]))
        if single_tiles:
            seen = flags.cpu().tolist()                              # synchronisation 1: can the fold be absorbed?
            single = {d: cands[d] is not None and seen[2 + k] != 0 for k, d in enumerate(dirs)}
    if not CLOSE_SINGLE_ENABLED:
        single = {d: False for d in dirs}
    need_parts = [d for d in dirs if cands[d] is not None and not single[d]]
    multi = {}
    if absorb and CLOSE_MULTI_ENABLED and need_parts:
        # a graph over 32 nodes: the absorbed fold over MULTI-TILE graphs (every graph's tiles in one workgroup's stream) where the
        # segments pass the same test without the size limit; one read-back for both directions
        mflags = torch.zeros(2, dtype=I32, device=dev)
        for k, d in enumerate(dirs):
            if d in need_parts:
                multi[d] = build_graph_tiles_multi(ix.dirs[d].aux_ptr[:cands[d][3] + 1].contiguous(), ix.dirs[d].aux_idx, N,
                                                   ok=mflags[k:], add_idx=_fold_add_idx(ix, d, cands[d]))
        seen = mflags.cpu().tolist()
        multi = {d: multi[d] for k, d in enumerate(dirs) if d in multi and seen[k] != 0}
        need_parts = [d for d in need_parts if d not in multi]
    parts = {d: _queue_fold_tables(ix, d, cands[d][3], flags[dirs.index(d):]) for d in need_parts}
    if before_readback is not None:
        before_readback(cands, flags)
    seen = flags.cpu().tolist() if need_parts else [0, 0]         # synchronisation 2 (the only one for kind "slots")
    parts_valid = {d: d in parts and seen[k] != 0 for k, d in enumerate(dirs)}
    for d in dirs:
        info = _Fold(ix, d, cands[d]) if (single[d] or d in multi or parts_valid[d]) else None
        if single[d]:                                                # absorbed, single tile
            info.graph_tiles = single_tiles[d]
        elif d in multi:                                             # absorbed, multi tile
            info.graph_tiles = (multi[d][0], multi[d][1])
            info.multi = (multi[d][2], multi[d][3], multi[d][4], cands[d][3])
        elif parts_valid[d]:                                         # partial rows
            info.fold_info, info.part_ptr = parts[d]
        ix._fold[d] = info


def _build_slot_tables(ix):
    """ix._slots of both directions (dn_rows_selfsum_bf16): on an index's first closing kind the fold tables and the slot tables
    (which read the fold's verdict on the device) are queued in front of ONE read-back; after the unit streams, a fold absorbed so
    far gets its partial-row tables first."""
    N, P, K, dirs = ix.num_nodes, ix.num_edge_rows, SELFSUM_SLOTS, ("f", "b")
    lists = {d: (ix.dirs[d].list_ptr, ix.dirs[d].list_rows) for d in dirs}
    tabs = {}
    if not ix._fold:
        def queue_slot_tables(cands, flags):
            for k, d in enumerate(dirs):
                drop, enable = ((cands[d][1], cands[d][2]), flags[k:]) if cands[d] is not None else ((0, 0), None)
                tabs[d] = build_slot_table(*lists[d], N, P, K, drop=drop, drop_enable=enable)
        _decide_folds(ix, "slots", before_readback=queue_slot_tables)
    else:
        for d in dirs:
            info = ix._fold[d]
            if info is not None and info.fold_info is None:          # absorbed so far: the slot kernel needs the partial-row tables
                _late_fold_tables(ix, d, info)
            drop = (info.beg, info.end) if info is not None else (0, 0)
            tabs[d] = build_slot_table(*lists[d], N, P, K, drop=drop)
    longest = {d: None for d in dirs}
    if 0 < N <= OVERFLOW_INSIDE_MAX_ROWS:
        # the longest list of each direction (one small read-back per batch, small batches only): rows_selfsum walks overflowing
        # lists inside the launch only while they are short
        mx = torch.stack([(lists[d][0][1:N + 1] - lists[d][0][:N]).max() for d in dirs]).tolist()
        longest = {d: int(mx[k]) for k, d in enumerate(dirs)}
    for d in dirs:
        info = ix._fold[d]
        drop = (info.beg, info.end) if info is not None else (0, 0)
        slots, over = tabs[d]
        ix._slots[d] = (slots, (*lists[d], P, drop[0], drop[1], over, longest[d]))


def _build_unit_streams(ix):
    """ix._units of both directions (dn_rows_close_bf16, H = 256), built behind the fold's verdicts: their tiles depend on them."""
    N, P = ix.num_nodes, ix.num_edge_rows
    if not ix._fold:
        _decide_folds(ix, "units")
    for d in ("f", "b"):
        info, lists = ix._fold[d], (ix.dirs[d].list_ptr, ix.dirs[d].list_rows)
        drop = (info.beg, info.end) if info is not None else (0, 0)
        if (info is not None and info.graph_tiles is None and CLOSE_AGG_ENABLED and CLOSE_SINGLE_ENABLED
                and ix._absorb is not None and (ix._absorb[d].verdict & 1)):     # (the slot tables came first: the builder's verdict still stands)
            info.graph_tiles = (ix._absorb[d].tile_ptr[:info.n + 1], ix._absorb[d].fold_info[:info.n])
        if info is not None and info.graph_tiles is not None:       # every graph inside one tile: the fold is absorbed
            ix._units[d] = build_close_units(*lists, N, P, drop=drop, tile_ptr=info.graph_tiles[0], agg=True, multi=info.multi)
        else:
            if info is not None and info.fold_info is None:
                _late_fold_tables(ix, d, info)
            ix._units[d] = build_close_units(*lists, N, P, drop=drop)


def _closing_tables(ix, kind="slots"):
    """Tables of the closing launches of BOTH directions of a RowIndex: kind "units" (_build_unit_streams) or "slots"
    (_build_slot_tables).  The first kind an index serves decides the folds (_decide_folds); a second kind on the same index reuses
    the verdicts and builds only what it misses."""
    if kind == "slots" and not ix._slots:
        _build_slot_tables(ix)
    elif kind != "slots" and not ix._units:
        _build_unit_streams(ix)


def _close_kind(H, dtype):
    """Which closing launch serves rows of this width: the unit stream (H = 256) or the slot kernel."""
    return "units" if (CLOSE_RING_ENABLED and H == 256 and dtype == torch.bfloat16) else "slots"


# The collapsed relation of a dummy-augmented batch (u -> dummy forward, dummy -> u backward) needs the SUM of a graph's rows as
# its input row.  As a launch of its own (gather_segsum over the aux lists) that is a second full read of x (config 5: 0.5 GB,
# ~100 us per direction); the closing launch reads every x row anyway, so it can produce those sums on the side.
FOLD_ENABLED = _os.environ.get("DN_FOLD", "1") != "0"


class _Fold:
    """Tables of one folded relation: rows [beg, end) of the row set, one per segment (graph)."""
    __slots__ = ("rel", "beg", "end", "n", "fold_info", "part_ptr", "num_parts", "main_tiles", "sweep_tiles", "add_idx",
                 "graph_tiles", "multi", "seg_tiles")

    def __init__(self, ix, direction, cand):
        self.rel, self.beg, self.end, self.n = cand
        self.fold_info = self.part_ptr = self.graph_tiles = self.multi = self.seg_tiles = None
        self.num_parts = int(2 * self.n + ix.num_nodes // 32 + 1)   # upper bound of part_ptr[-1] without a read-back: every segment
        #                                                             starts one partial row, every tile boundary inside one another
        self.main_tiles = None                               # plain relation-major tiles, built on first use (_conv_tiles_for)
        self.sweep_tiles = None                              # built on the first H = 256 launch (_conv_tiles_for)
        self.add_idx = _fold_add_idx(ix, direction, cand)


def _row_index_fold(ix, direction, kind="slots"):
    """The relation whose pre-aggregation the closing launch can absorb, or None: exactly ONE collapsed relation in this
    direction (AGG forward / TF backward), its aux lists contiguous ascending node ranges (a graph's nodes), bf16 self-loop path
    (checked on the device by dn_fold_tables_build_async_i32; the verdict comes back with the closing tables of `kind`)."""
    _closing_tables(ix, kind)
    return ix._fold[direction]


class RowIndexSet:
    """Holder of a batch's ONE RowIndex (`index`) and of the Y buffers its launches share.  `parts` = [(0, N, index)] is the form
    the benchmark and the tools read.  (Cutting a batch into cache-resident sub-batches lost more to under-filled launches than the
    Infinity Cache returned at every split -- DESIGN.md section 4.)"""

    def __init__(self, src=None, dst=None, etype=None, num_nodes=None, num_rels=None, self_loop=None, node_ptr=None, edge_ptr=None,
                 closing_hint=None, index=None):
        """RowIndexSet(index=ix) holds a RowIndex that exists already; else the index is built from the batch."""
        self.index = ix = index if index is not None else RowIndex(
            src, dst, etype, int(num_nodes), num_rels, self_loop=self_loop, node_ptr=node_ptr, edge_ptr=edge_ptr, closing_hint=closing_hint)
        self.num_nodes, self.num_rels, self.self_loop = ix.num_nodes, ix.num_rels, ix.self_loop
        self.parts = [(0, ix.num_nodes, ix)]
        self.max_rows = self.num_rows = ix.num_rows
        self.num_all_rels = ix.num_all_rels
        self._ybuf = {}

    def ybuf(self, H, dtype, dev):
        key = (H, dtype, str(dev))
        b = self._ybuf.get(key)
        if b is None:
            b = torch.empty((self.max_rows, H), dtype=dtype, device=dev)
            self._ybuf[key] = b
        return b


def _selfsum_ok(ix, x):
    return SELFSUM_ENABLED and ix.self_loop and x.dtype == torch.bfloat16


def fold_tail(part, part_ptr, num_segments, Wn, idx, out, w_kn=False):
    """aux[j] = sum of partial rows part_ptr[j] .. part_ptr[j+1] in order;  out[idx[j]] += aux[j] @ Wn^T  (dn_fold_tail_bf16;
    w_kn: Wn given [in][out] instead).  Returns aux (bf16)."""
    require_gpu(part, part_ptr, Wn, idx, out)
    H = part.shape[1]
    assert part.dtype == torch.float32 and part_ptr.dtype == I32 and idx.dtype == I32 and idx.numel() == num_segments
    assert out.dtype == torch.bfloat16 and Wn.dtype == torch.bfloat16 and Wn.shape == (H, H) and out.shape[1] == H
    assert out.is_contiguous() and Wn.is_contiguous() and part.is_contiguous()
    aux = torch.empty((num_segments, H), dtype=torch.bfloat16, device=part.device)

    def _launch():
        check(lib().dn_fold_tail_bf16(ptr(part), ptr(part_ptr), int(num_segments), H, ptr(Wn), ptr(idx), ptr(aux), ptr(out),
                                      1 if w_kn else 0, stream_ptr()), "dn_fold_tail_bf16")
    launch_tagged("fold_tail", _launch)
    return aux


class PassWeights:
    """Weights of ONE direction of a message pass: rel [R, H, H] for the edge relations, loop [H, H] for the self loop (or None).
    kn = False: every matrix is [n][k] (rows = output columns, the form the MFMA kernels read contiguously: W^T for the forward
    pass, W itself for the input-gradient pass); kn = True: [k][n] -- the forward pass straight on the parameters `weight` /
    `loop_weight` as the reference stores them (rgin.py:61-67), which the H = 256 bf16 kernels gather themselves, so the step
    has no `cat` / `transpose().contiguous()` launches."""
    __slots__ = ("rel", "loop", "kn", "_all")

    def __init__(self, rel, loop, kn=False):
        self.rel, self.loop, self.kn, self._all = rel.contiguous(), (loop.contiguous() if loop is not None else None), bool(kn), None

    def all_nk(self):
        """[R (+1), n, k] in one contiguous tensor (loop last): the kernels without a kn mode (fp32, H != 256, no closing launch)."""
        if self._all is None:
            w = self.rel if self.loop is None else torch.cat([self.rel, self.loop.unsqueeze(0)], 0)
            self._all = w.transpose(1, 2).contiguous() if self.kn else w.contiguous()
        return self._all

    def nk(self):
        """The same weights with kn = False."""
        if not self.kn:
            return self
        a = self.all_nk()
        return PassWeights(a if self.loop is None else a[:-1], None if self.loop is None else a[-1], False)


# DN_KN_SMALL=0: at H = 64 / 128 (bf16) the weights are concatenated and transposed in front of the forward launches, as before round 5
KN_SMALL_ENABLED = _os.environ.get("DN_KN_SMALL", "1") != "0"


def _kn_ok(xs):
    """The launches that take [k][n] weights: bf16 H = 256 (ring transform, unit-stream closing launch, fold tail), bf16 H = 64 /
    128 (register-staged transform, slot kernel, fold tail) and the fp32 transform (any of its widths; it also takes the self-loop
    matrix and the bias where the parameters lie)."""
    if xs.dtype == torch.float32:
        return xs.shape[1] in (64, 128, 256)
    if xs.dtype == torch.bfloat16 and xs.shape[1] in (64, 128):
        return KN_SMALL_ENABLED                      # round 5: the register-staged transform and the slot kernel read [k][n] too
    return xs.dtype == torch.bfloat16 and xs.shape[1] == 256 and CLOSE_RING_ENABLED


def _closing_launch(xs, W_loop, bias, Y, ix, direction, out, seg=None, w_kn=False):
    """The closing launch over one RowIndex: the unit stream at H = 256 (dn_rows_close_bf16), else the slot kernel + its
    overflow launch (dn_rows_selfsum_bf16, dn_overflow_rows_add_bf16)."""
    if _close_kind(xs.shape[1], xs.dtype) == "units":
        return rows_close(xs, W_loop, bias, Y, ix.close_units(direction), out=out, seg=seg, w_kn=w_kn)
    slots, lists = ix.slots(direction)
    return rows_selfsum(xs, W_loop, bias, Y, None, slots, out=out, seg=seg, lists=lists, w_kn=w_kn)


def _message_pass_folded(xs, pw, bias, ix, direction, ybuf, out, idx_rows):
    """message_pass with the collapsed relation's pre-aggregation absorbed by the closing launch: transform of every other
    relation -> closing launch (+ per-graph column sums of xs) -> tail launch (combine the sums, transform the one row per graph,
    add each product to its node).  Where every graph fits one tile of the unit stream (H = 256) the closing launch does the
    tail's work itself (its AGG units): two launches per direction.  Same sums as the unfolded path up to bf16 rounding of the
    collapsed rows."""
    kind = _close_kind(xs.shape[1], xs.dtype)
    fold = _row_index_fold(ix, direction, kind)
    P, H = ix.num_edge_rows, xs.shape[1]
    Y = rows_transform(xs, pw.rel, _conv_tiles_for(ix, fold, H, xs.dtype), P, idx=idx_rows, tag="conv", out=ybuf, w_kn=pw.kn)
    if kind == "units" and ix.close_units(direction).agg:
        aux = torch.empty((fold.n, H), dtype=xs.dtype, device=xs.device)
        rows_close(xs, pw.loop, bias, Y[:P], ix.close_units(direction), out=out, w_kn=pw.kn,
                   agg=(fold.graph_tiles[1], pw.rel[fold.rel], aux, fold.add_idx))
        return aux
    part = torch.empty((fold.num_parts, H), dtype=torch.float32, device=xs.device)
    _closing_launch(xs, pw.loop, bias, Y[:P], ix, direction, out, seg=(fold.fold_info, part), w_kn=pw.kn)
    return fold_tail(part, fold.part_ptr, fold.n, pw.rel[fold.rel], fold.add_idx, out, w_kn=pw.kn)


# DN_CONV_GRAPHS=0: H = 64 bf16 batches of small graphs keep the row-factorised launches (transform, closing launch, fold tail)
CONV_GRAPHS_ENABLED = _os.environ.get("DN_CONV_GRAPHS", "1") != "0"


def conv_graphs_ok(xs, pw, ix):
    """Can dn_conv_graphs_bf16 take this pass?  bf16 rows of width 64, square weights with a self loop, a batch the graph-local
    index builder has seen (it reports the largest graph), every graph within 64 nodes / 1024 edges, at most 16 relations."""
    if not (CONV_GRAPHS_ENABLED and xs.dtype == torch.bfloat16 and xs.shape[1] == 64 and pw.loop is not None and ix.self_loop
            and ix.raw is not None and ix.max_graph is not None and ix.num_rels <= 16 and tuple(pw.rel.shape[1:]) == (64, 64)):
        return False
    return 0 < ix.max_graph[0] <= 64 and ix.max_graph[1] <= 1024 and ix.num_edges > 0       # (no edges: nothing to point the launch at)


def conv_graphs(xs, pw, bias, ix, direction, out):
    """One direction of the conv over ix's batch as ONE launch (dn_conv_graphs_bf16, one workgroup per graph, every relation edge
    by edge).  Returns the pre-aggregated rows the weight gradient's collapsed relation takes (per-graph column sums of xs, written
    by the same launch where the direction's aux lists are the graphs' segments; else one gather launch)."""
    src, dst, etype, node_ptr, edge_ptr = ix.raw
    key_in, key_out = (src, dst) if direction == "f" else (dst, src)
    v = ix.dirs[direction]
    G, N, H = int(node_ptr.numel()) - 1, ix.num_nodes, 64
    require_gpu(xs, pw.rel, pw.loop, bias, out)
    assert xs.is_contiguous() and out.is_contiguous() and out.shape == xs.shape and pw.rel.is_contiguous() and pw.loop.is_contiguous()
    err = _graphs_err(ix, xs.device)
    inside, aux, sp, sn = _graphs_aux(ix, direction, xs)

    def _launch():
        check(lib().dn_conv_graphs_bf16(ptr(xs), H, ptr(pw.rel), 1 if pw.kn else 0, ptr(pw.loop), ptr(bias), ix.num_rels, ptr(node_ptr),
                                        ptr(edge_ptr), ptr(key_in), ptr(key_out), ptr(etype), G, N, ptr(out), ptr(sp),
                                        ptr(sn), ptr(aux), ptr(err), stream_ptr()),
              "dn_conv_graphs_bf16")
    launch_tagged("conv_graphs", _launch)
    if v.n_aux and not inside:
        aux = gather_segsum(xs, v.aux_idx, v.aux_ptr, v.n_aux)
    return aux


def _graphs_err(ix, dev):
    """The error / statistics words the whole-graph launches of an index OR into (one buffer per index, made on first use)."""
    if ix._cg_err is None:
        ix._cg_err = torch.zeros(16, dtype=I32, device=dev)
    return ix._cg_err


def _graphs_aux(ix, direction, xs):
    """(inside, aux tensor or None, seg_ptr or None, seg_nodes or None) for the whole-graph launches: the direction's aux lists are the
    graphs' segments (one collapsed relation, one row per graph) -> the launch writes the column sums itself."""
    v = ix.dirs[direction]
    G = int(ix.raw[3].numel()) - 1
    cand = _fold_candidate(ix, direction) if v.n_aux else None
    inside = (cand is not None and cand[3] == G and v.n_aux == G and ix._absorb is not None and ix._absorb[direction].verdict != 0)
    if not inside:
        return False, None, None, None
    return True, torch.empty((v.n_aux, xs.shape[1]), dtype=xs.dtype, device=xs.device), v.aux_ptr[:v.n_aux + 1].contiguous(), v.aux_idx


def layer_graphs_fwd(x, W, W_loop, bias, w1, b1, w2, b2, slope, ix):
    """A whole RGIN layer forward on ix's batch of small graphs in ONE launch (dn_layer_graphs_fwd_bf16).
    -> (h conv rows, h1, h2, bits1, bits2, aux)."""
    src, dst, etype, node_ptr, edge_ptr = ix.raw
    G, N, H = int(node_ptr.numel()) - 1, ix.num_nodes, 64
    require_gpu(x, W, W_loop, bias, w1, b1, w2, b2)
    assert x.is_contiguous() and W.is_contiguous() and W_loop.is_contiguous() and w1.is_contiguous() and w2.is_contiguous()
    err = _graphs_err(ix, x.device)
    inside, aux, sp, sn = _graphs_aux(ix, "f", x)
    h, h1, h2 = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)
    bits1 = torch.empty((N, H // 8), dtype=torch.uint8, device=x.device)
    bits2 = torch.empty((N, H // 8), dtype=torch.uint8, device=x.device)

    def _launch():
        check(lib().dn_layer_graphs_fwd_bf16(ptr(x), H, ptr(W), ptr(W_loop), ptr(bias), ix.num_rels, ptr(w1), ptr(b1), ptr(w2), ptr(b2),
                                             float(slope), ptr(node_ptr), ptr(edge_ptr), ptr(src), ptr(dst), ptr(etype), G, N, ptr(h), ptr(h1),
                                             ptr(h2), ptr(bits1), ptr(bits2), ptr(sp), ptr(sn), ptr(aux), ptr(err), stream_ptr()),
              "dn_layer_graphs_fwd_bf16")
    launch_tagged("layer_graphs_fwd", _launch)
    if ix.num_aux_f and not inside:
        aux = gather_segsum(x, ix.aux_f_idx, ix.aux_f_ptr, ix.num_aux_f)
    return h, h1, h2, bits1, bits2, aux


def layer_graphs_bwd(g, W, W_loop, w1, w2, slope, bits1, bits2, ix):
    """... and its input gradients in ONE launch (dn_layer_graphs_bwd_bf16).  -> (g1, g0, gx, aux_b)."""
    src, dst, etype, node_ptr, edge_ptr = ix.raw
    G, N, H = int(node_ptr.numel()) - 1, ix.num_nodes, 64
    require_gpu(g, W, W_loop, w1, w2, bits1, bits2)
    assert g.is_contiguous() and W.is_contiguous() and W_loop.is_contiguous() and w1.is_contiguous() and w2.is_contiguous()
    g1, g0, gx = torch.empty_like(g), torch.empty_like(g), torch.empty_like(g)
    inside, aux_b, sp, sn = _graphs_aux(ix, "b", g)

    def _launch():
        check(lib().dn_layer_graphs_bwd_bf16(ptr(g), H, ptr(W), ptr(W_loop), ix.num_rels, ptr(w1), ptr(w2), float(slope), ptr(bits1),
                                             ptr(bits2), ptr(node_ptr), ptr(edge_ptr), ptr(src), ptr(dst), ptr(etype), G, N, ptr(g1), ptr(g0),
                                             ptr(gx), ptr(sp), ptr(sn), ptr(aux_b), ptr(ix._cg_err), stream_ptr()),
              "dn_layer_graphs_bwd_bf16")
    launch_tagged("layer_graphs_bwd", _launch)
    if ix.num_aux_b and not inside:
        aux_b = gather_segsum(g0, ix.aux_b_idx, ix.aux_b_ptr, ix.num_aux_b)
    return g1, g0, gx, aux_b


def message_pass(xs, pw, bias, ix, direction, ybuf, out, add_in=None):
    """One direction of the row-factorised pass over one RowIndex -- the launches that ARE the layer's gather-scatter:
         'f':  out[v] = sum_{rows p -> v} (in_row(p) @ W[rel p])          pw = the weights (PassWeights), [k][n] or W^T
         'b':  out[u] = sum_{rows p <- u} (g_row(p)  @ W[rel p]^T)        pw = W per relation as it is ([n = in][k = out])
       = pre-aggregation of the collapsed relations (gather_segsum) -> gathered-row transform on the matrix cores ->
       closing launch.  With a self loop in bf16 the closing launch is dn_rows_close_bf16 / dn_rows_selfsum_bf16 (self-loop
       transform + bias + per-node sum of the edge rows in one pass); otherwise the self-loop rows go through the transform like
       any relation and a per-node gather_segsum closes.  Returns the pre-aggregated rows (kept for the weight gradient)."""
    v = ix.dirs[direction]
    f32_direct = xs.dtype == torch.float32 and _kn_ok(xs) and pw.rel.shape[1] == pw.rel.shape[2]
    assert add_in is None or f32_direct        # (add_in: rows added to the result by the closing gather -- the fp32 path only)
    if conv_graphs_ok(xs, pw, ix):
        return conv_graphs(xs, pw, bias, ix, direction, out)
    if pw.kn and not (f32_direct or (_kn_ok(xs) and _selfsum_ok(ix, xs))):
        pw = pw.nk()
    if _selfsum_ok(ix, xs) and _row_index_fold(ix, direction, _close_kind(xs.shape[1], xs.dtype)) is not None:
        return _message_pass_folded(xs, pw, bias, ix, direction, ybuf, out, v.rows_in)
    aux = gather_segsum(xs, v.aux_idx, v.aux_ptr, v.n_aux) if v.n_aux else None
    if _selfsum_ok(ix, xs):
        P = ix.num_edge_rows
        Y = (rows_transform(xs, pw.rel, ix.edge_tile_table, P, idx=v.rows_in, X2=aux, tag="conv", out=ybuf, w_kn=pw.kn)
             if P else ybuf[:0])
        _closing_launch(xs, pw.loop, bias, Y[:P], ix, direction, out, w_kn=pw.kn)
        return aux
    if f32_direct:
        # fp32: the transform reads weight / loop_weight / h_bias where the parameters lie (no cat, no transposed copy, no padded
        # bias matrix); the self-loop rows are relation R of the tile table
        R = pw.rel.shape[0]
        Y = rows_transform(xs, pw.rel, ix.tile_table, ix.num_rows, idx=v.rows_in, X2=aux, bias=bias, tag="conv", out=ybuf,
                           w_kn=pw.kn, W_loop=pw.loop, loop_rel=R, bias_rel=R if bias is not None else -1)
        gather_segsum(Y, v.list_rows, v.list_ptr, ix.num_nodes, out=out, self_in=add_in, self_coef=1.0 if add_in is not None else 0.0)
        return aux
    Wmat = pw.all_nk()
    bias_all = None
    if bias is not None:
        bias_all = torch.zeros((Wmat.shape[0], Wmat.shape[1]), dtype=xs.dtype, device=xs.device)
        bias_all[-1] = bias                                                  # only self-loop rows carry the bias
    Y = rows_transform(xs, Wmat, ix.tile_table, ix.num_rows, idx=v.rows_in, X2=aux, bias=bias_all, tag="conv", out=ybuf)
    gather_segsum(Y, v.list_rows, v.list_ptr, ix.num_nodes, out=out)
    return aux


class _RowTransformFn(torch.autograd.Function):
    """out = sum over in-edges of x[src] @ W[etype]  (+ x @ W_loop + bias when the index has the self loop), evaluated
    over a RowIndexSet's index.  W [R, in, out] and W_loop [in, out] are the layer's own tensors: nothing is
    concatenated or transposed on the bf16 H = 256 path."""

    @staticmethod
    def forward(ctx, x, W, W_loop, bias, index_set):
        ctx.f32_mode = f32_mode()
        x = x.contiguous()
        H_out = W.shape[2]
        pw = PassWeights(W, W_loop, kn=True)
        if not _kn_ok(x):
            pw = pw.nk()                                                     # [R', out, in], one cat + transposed copy
        out = torch.empty((x.shape[0], H_out), dtype=x.dtype, device=x.device)
        ybuf = index_set.ybuf(H_out, x.dtype, x.device)
        aux = message_pass(x, pw, bias, index_set.index, "f", ybuf, out)
        ctx.index_set, ctx.has_bias, ctx.has_loop = index_set, bias is not None, W_loop is not None
        ctx.save_for_backward(x, W, W_loop if W_loop is not None else x.new_empty(0),
                              aux if aux is not None else x.new_empty(0))    # a few MB: kept for the weight gradient
        return out

    @staticmethod
    @_backward_in_forward_mode
    def backward(ctx, g):
        iset, ix = ctx.index_set, ctx.index_set.index
        g = g.contiguous()
        x, W, W_loop, aux = ctx.saved_tensors
        R_all = W.shape[0] + (1 if ctx.has_loop else 0)
        pw = PassWeights(W, W_loop if ctx.has_loop else None, kn=False)     # the input-gradient pass reads W as it is
        need_x = ctx.needs_input_grad[0]
        need_w = ctx.needs_input_grad[1] or ctx.needs_input_grad[2] or (ctx.has_bias and ctx.needs_input_grad[3])
        gx = torch.empty_like(x) if need_x else None
        if need_x:
            aux_b = message_pass(g, pw, None, ix, "b", iset.ybuf(W.shape[1], g.dtype, g.device), gx)
        else:
            aux_b = gather_segsum(g, ix.aux_b_idx, ix.aux_b_ptr, ix.num_aux_b) if ix.num_aux_b else None
        gW = gL = gb = None
        if need_w:
            # bias gradient = column sum of g over the self-loop rows (one per node), folded into the same kernel
            gAll, cs = rows_wgrad(x, g, ix.chunk_table, R_all, idx_a=ix.row_in, idx_g=ix.row_out, A2=aux if ix.num_aux_f else None,
                                  G2=aux_b, out_dtype=W.dtype, colsum_of=2, colsum_lp=True,
                                  colsum_rel=R_all - 1)                      # (gb = cs[-1] below: the other relations' sums are not used)
            gW = gAll[:W.shape[0]]                                           # [R (+1), in, out]: the two gradients are views of it
            if ctx.has_loop:
                gL = gAll[W.shape[0]]
            if ctx.has_bias:
                gb = cs[-1].to(g.dtype)
        return gx, gW, gL, gb, None


class _BddDenseFn(torch.autograd.Function):
    """Block-diagonal relation weights [R, B * si * so] -> dense [R, B * si, B * so] (dn_bdd_compose), gradient = the diagonal
    blocks of the dense gradient (dn_bdd_extract): one launch each way (rgin.py:114-120's per-block products as dense ones)."""

    @staticmethod
    def forward(ctx, weight, R, B, si, so):
        w = weight.contiguous()
        require_gpu(w)
        assert w.numel() == R * B * si * so and w.dtype in (torch.bfloat16, torch.float32)
        dense = torch.empty((R, B * si, B * so), dtype=w.dtype, device=w.device)
        check(lib().dn_bdd_compose(ptr(w), R, B, si, so, w.element_size(), ptr(dense), stream_ptr()), "dn_bdd_compose")
        ctx.dims, ctx.shape = (R, B, si, so), weight.shape
        return dense

    @staticmethod
    def backward(ctx, g):
        R, B, si, so = ctx.dims
        g = g.contiguous()
        gb = torch.empty(ctx.shape, dtype=g.dtype, device=g.device)
        check(lib().dn_bdd_extract(ptr(g), R, B, si, so, g.element_size(), ptr(gb), stream_ptr()), "dn_bdd_extract")
        return gb, None, None, None, None


def bdd_dense(weight, num_rels, num_bases, submat_in, submat_out):
    """Dense [R, B * si, B * so] view of block-diagonal relation weights, differentiable (GPU, bf16 / fp32)."""
    return _BddDenseFn.apply(weight, int(num_rels), int(num_bases), int(submat_in), int(submat_out))


def fused_path_supported(x, W):
    """bf16 (storage bf16 / fp32 accumulate) and fp32 (exact-f32 MFMA) run the row-factorised matrix-core pipeline when the
    layer is square with H in {64, 128, 256}; everything else takes the generic two-pass path."""
    return (x.is_cuda and x.dtype == W.dtype and x.dtype in MFMA_DTYPES and W.dim() == 3
            and W.shape[1] == W.shape[2] and W.shape[1] in (64, 128, 256) and x.shape[1] == W.shape[1])


def rel_transform_fused(x, W, bias, index_set, W_loop=None):
    """Fused row-factorised path.  Either W = [R, in, out] with the self-loop weight given separately (W_loop [in, out] -- the
    layer's own parameters, nothing concatenated), or, without W_loop, W = [R (+1), in, out] with the self-loop weight LAST when
    index_set.self_loop.  bias is added on the self-loop rows (requires the self loop).  index_set: RowIndexSet (or a RowIndex)."""
    if isinstance(index_set, RowIndex):
        index_set = RowIndexSet(index=index_set)
    assert bias is None or index_set.self_loop
    if W_loop is None and index_set.self_loop:
        assert W.shape[0] == index_set.num_all_rels
        W, W_loop = W[:-1], W[-1]                                            # views: their gradients flow back into W's
    assert W.shape[0] == index_set.num_rels and (W_loop is not None) == index_set.self_loop
    return _RowTransformFn.apply(x, W, W_loop, bias, index_set)


# ----------------------------------------------------------------------------------------------
# dense Linear(+ReLU) of the post-aggregate MLP on the same MFMA kernels (bf16)
# ----------------------------------------------------------------------------------------------
_dense_tables = {}


def _dense_table(n_rows, dev):
    """Tile / chunk tables of a single-relation, identity-indexed row set (cached per size and device)."""
    key = (int(n_rows), str(dev))
    t = _dense_tables.get(key)
    if t is None:
        # split-K chunks sized for ONE round of 256 workgroups whatever the row count (a 20 k-row GC batch with 4096-row chunks
        # would run its weight gradient on five workgroups; 378 chunks of a 1 M-row batch would run one and a half rounds)
        # (at least 128 rows a chunk, not 256: a 16 k-row GC batch then has 125 workgroups walking 4 tiles each instead of 63 walking
        #  8 -- GIN steps under replay 0.334 -> 0.318 / 0.636 -> 0.625 / 0.812 -> 0.787 ms; 64 rows: the H = 256 partial tiles cost more)
        chunk = max(128, min(WGRAD_CHUNK_CAP, -(-int(n_rows) // 256 // 64) * 64))
        t = (make_row_tiles([0, int(n_rows)], dev), make_row_chunks([0, int(n_rows)], dev, chunk_rows=chunk))
        if len(_dense_tables) > 8:
            _dense_tables.clear()
        _dense_tables[key] = t
    return t


class _LinearActFn(torch.autograd.Function):
    """y = relu?(x @ weight^T + bias) with weight [out, in] (nn.Linear layout): forward and both backward products on
    dn_rows_transform_bf16 / dn_rows_wgrad_bf16, bias and ReLU fused in the forward epilogue."""

    @staticmethod
    def forward(ctx, x, weight, bias, relu, exact=None):
        x = x.contiguous()
        tiles, _ = _dense_table(x.shape[0], x.device)
        # exact: None = module default, True / False, or "fwd" = exact products where errors propagate (forward, input
        # gradient), the 3-term split for the weight gradient (a leaf: its 1e-5 relative error goes nowhere)
        ctx.exact = f32_mode() if exact is None else bool(exact)
        ctx.exact_w = False if exact == "fwd" else ctx.exact
        with f32_exact(ctx.exact):
            y = rows_transform(x, weight.contiguous().unsqueeze(0), tiles, x.shape[0],
                               bias=None if bias is None else bias.contiguous().view(1, -1), relu=relu)
        ctx.relu, ctx.has_bias = bool(relu), bias is not None
        ctx.save_for_backward(x, weight, y if relu else x.new_empty(0))
        return y

    @staticmethod
    def backward(ctx, g):
        with f32_exact(ctx.exact):
            return _LinearActFn._backward(ctx, g) + (None,)

    @staticmethod
    def _backward(ctx, g):
        x, weight, y = ctx.saved_tensors
        g = g.contiguous()
        tiles, chunks = _dense_table(x.shape[0], x.device)
        gx = gw = gb = None
        need_w = ctx.needs_input_grad[1] or (ctx.has_bias and ctx.needs_input_grad[2])
        if ctx.relu and not need_w:
            g = relu_bwd(g, y)
        if need_w:
            # g^T x -> [out, in] and colsum(g); the ReLU mask is applied while the rows are staged and the masked rows are
            # written out for the input-gradient launch (no separate elementwise pass)
            gm = torch.empty_like(g) if ctx.relu else None
            with f32_exact(ctx.exact_w):
                gw, cs = rows_wgrad(g, x, chunks, 1, out_dtype=weight.dtype, colsum_of=1, mask_a=y if ctx.relu else None,
                                    a_out=gm)
            g = gm if ctx.relu else g
            gw = gw[0]
            if ctx.has_bias:
                gb = cs[0].to(g.dtype)
        if ctx.needs_input_grad[0]:
            kn = g.dtype == torch.float32                       # the fp32 kernels read Linear.weight [out = k][in = n] as it is
            gx = rows_transform(g, (weight if kn else weight.t()).contiguous().unsqueeze(0), tiles, x.shape[0], w_kn=kn)  # g @ weight
        return gx, gw, gb, None


def relu_bwd(g, y, slope=0.0):
    """(y > 0) ? g : slope * g  (dn_relu_bwd_bf16 / _f32; slope 0 = ReLU)."""
    require_gpu(g, y)
    out = torch.empty_like(g)
    fn = lib().dn_relu_bwd_f32 if g.dtype == torch.float32 else lib().dn_relu_bwd_bf16
    check(fn(ptr(g), ptr(y), ptr(out), g.numel(), float(slope), stream_ptr()), "dn_relu_bwd")
    return out


# DN_MLP_BWD_FUSED=0: the bf16 two-layer MLP at H = 256 keeps its three backward launches (weight gradient 2, the input-gradient chain,
# weight gradient 1) instead of dn_mlp_bwd_fused_bf16 twice -- for A/B runs and for tracing (results are bit-identical either way)
MLP_BWD_FUSED_ENABLED = _os.environ.get("DN_MLP_BWD_FUSED", "1") != "0"
# ... from this many rows on.  Smaller batches keep the three launches: the fused launches were built for and measured on the
# HBM-bound whole batch (1 M rows: step 3.18 -> 3.08 ms); an H = 256 layer on a small batch is _RginLayerWideFn's (one weight-gradient
# launch for the whole layer), and where that is switched off its separate functions stay what they were
MLP_BWD_FUSED_MIN_ROWS = int(_os.environ.get("DN_MLP_BWD_FUSED_MIN_ROWS", str(1 << 18)))


def mlp_bwd_fused_supported(g, a, w):
    return (g.dtype == torch.bfloat16 and a.dtype == torch.bfloat16 and w.dtype == torch.bfloat16 and g.dim() == 2
            and g.shape[0] > 0 and g.shape[1] == 256 and a.shape == g.shape and tuple(w.shape) == (256, 256))


def mlp_bwd_fused(g, a, w, chunk_table, mask_in_bits=None, mask_out_bits=None, slope=0.0):
    """One Linear's backward in one pass over its rows (dn_mlp_bwd_fused_bf16, bf16, H = 256): with gm = g masked by mask_in_bits,
    returns (gw = gm^T a [H, H], gb = colsum(gm) [H], g_next = gm @ w masked by mask_out_bits [N, H]).  w: Linear.weight as stored
    ([out, in]); masks: the uint8 [N, H/8] bit tensors of rows_chain2 (both or neither); chunk_table: a one-relation row-chunk table
    over the N rows (_dense_table).  Bit-identical to rows_wgrad (mask_a_bits) + rows_chain2 (w_kn) + rows_wgrad on the same table."""
    chunks, chunk_ptr, nchunks = chunk_table
    g, a, w = g.contiguous(), a.contiguous(), w.contiguous()
    require_gpu(g, a, w, chunks, chunk_ptr, mask_in_bits, mask_out_bits)
    assert mlp_bwd_fused_supported(g, a, w) and nchunks > 0
    N, H = g.shape
    assert (mask_in_bits is None) == (mask_out_bits is None)
    for m in (mask_in_bits, mask_out_bits):
        assert m is None or (m.dtype == torch.uint8 and m.shape == (N, H // 8) and m.is_contiguous())
    gw = torch.empty((H, H), dtype=w.dtype, device=g.device)
    colsum = torch.empty((H,), dtype=torch.float32, device=g.device)
    gb = torch.empty((H,), dtype=w.dtype, device=g.device)
    g_next = torch.empty_like(g)
    ws = _ws(lib().dn_rows_wgrad_workspace_bytes(nchunks, H, H), g.device)

    def _launch():
        check(lib().dn_mlp_bwd_fused_bf16(ptr(g), ptr(a), ptr(w), ptr(mask_in_bits), ptr(mask_out_bits), N, H, ptr(chunks), nchunks,
                                          ptr(chunk_ptr), ptr(gw), 0, ptr(colsum), ptr(gb), ptr(g_next), float(slope), ptr(ws),
                                          ws.numel(), stream_ptr()), "dn_mlp_bwd_fused_bf16")
    launch_tagged("mlp_bwd_fused", _launch)
    return gw, gb, g_next


class _ReluMlpFn(torch.autograd.Function):
    """y_L = act(lin_L(... act(lin_1(x)))) with every Linear followed by the activation -- ReLU (slope 0) or leaky ReLU (the
    reference MLP + final activation, rgin.py:50-57,147-151, for act_func "relu" and for its CLI default "leaky_relu", slope
    1 / 5.5: config.py:329-335, utils/act.py:466).
    Two layers in bf16 (the reference default): ONE forward launch (dn_rows_chain2_bf16) that also emits both activation masks
    as bit tensors (sign of the output = sign of the pre-activation for either activation).  Backward at H = 256 from
    MLP_BWD_FUSED_MIN_ROWS rows on: TWO launches
    (dn_mlp_bwd_fused_bf16 per layer: outer mask, weight + bias gradient and the masked input gradient in one pass over the layer's
    rows; the weight gradient alone for layer 1 when the input needs no gradient), each followed by its reduce.  Other widths, smaller batches and
    DN_MLP_BWD_FUSED=0: three launches -- weight gradient of layer 2 (outer mask applied from its bits while the rows are staged),
    the whole input-gradient chain (mask, dgrad 2, mask, dgrad 1), weight gradient of layer 1 -- with bit-identical results.
    Otherwise: one fused Linear+bias+activation launch per layer forward; per layer backward a weight/bias-gradient launch and
    an input-gradient launch whose epilogue applies the activation mask of the layer below."""

    @staticmethod
    def forward(ctx, x, slope, *wb):
        ctx.f32_mode = f32_mode()
        n = len(wb) // 2
        x = x.contiguous()
        ctx.slope = slope = float(slope)
        if n == 2 and CHAIN2_ENABLED and x.dtype == torch.bfloat16:
            h1, h2, bits1, bits2 = rows_chain2(x, wb[0], wb[1], True, wb[2], wb[3], True, want_bits=True, slope=slope)
            ctx.n, ctx.chain = n, True
            ctx.has_bias = [wb[1] is not None, wb[3] is not None]
            ctx.save_for_backward(x, h1, bits1, bits2, wb[0], wb[2])      # the output itself is not kept: only its sign bits
            return h2
        if (n == 2 and CHAIN2_F32_ENABLED and x.dtype == torch.float32 and x.shape[1] in (64, 128) and not f32_mode()
                and all(t is None or t.dtype == torch.float32 for t in wb)):
            # fp32 (the reference's precision) at H = 64 / 128: both Linears in one launch each way (dn_rows_chain2_f32); the saved
            # activations are the masks
            h1, h2 = rows_chain2_f32(x, wb[0], wb[1], True, wb[2], wb[3], True, slope=slope)
            ctx.n, ctx.chain = n, "f32"
            ctx.has_bias = [wb[1] is not None, wb[3] is not None]
            ctx.save_for_backward(x, h1, h2, wb[0], wb[2])
            return h2
        tiles, _ = _dense_table(x.shape[0], x.device)
        acts = [x]
        for i in range(n):
            w, b = wb[2 * i], wb[2 * i + 1]
            acts.append(rows_transform(acts[-1], w.contiguous().unsqueeze(0), tiles, x.shape[0],
                                       bias=None if b is None else b.contiguous().view(1, -1), relu=True, slope=slope))
        ctx.n, ctx.chain = n, False
        ctx.has_bias = [wb[2 * i + 1] is not None for i in range(n)]
        ctx.save_for_backward(*acts, *[wb[2 * i] for i in range(n)])
        return acts[-1]

    @staticmethod
    @_backward_in_forward_mode
    def backward(ctx, gout):
        n, slope = ctx.n, ctx.slope
        saved = ctx.saved_tensors
        g = gout.contiguous()
        grads = [None] * (2 + 2 * n)
        if ctx.chain == "f32":
            x0, h1, h2, w1, w2 = saved
            _, chunks = _dense_table(x0.shape[0], x0.device)
            gw2, cs2 = rows_wgrad(g, h1, chunks, 1, out_dtype=w2.dtype, colsum_of=1, mask_a=h2, slope=slope)
            g1, g0 = rows_chain2_f32(g, w2, None, False, w1, None, False, mask0=h2, mask1=h1, w_kn=(True, True), slope=slope)
            gw1, cs1 = rows_wgrad(g1, x0, chunks, 1, out_dtype=w1.dtype, colsum_of=1)
            grads[2], grads[4] = gw1[0], gw2[0]
            if ctx.has_bias[0]:
                grads[3] = cs1[0].to(g.dtype)
            if ctx.has_bias[1]:
                grads[5] = cs2[0].to(g.dtype)
            grads[0] = g0 if ctx.needs_input_grad[0] else None
            return tuple(grads)
        if ctx.chain:
            x0, h1, bits1, bits2, w1, w2 = saved
            _, chunks = _dense_table(x0.shape[0], x0.device)
            if (MLP_BWD_FUSED_ENABLED and x0.shape[0] >= MLP_BWD_FUSED_MIN_ROWS and mlp_bwd_fused_supported(g, h1, w2)
                    and mlp_bwd_fused_supported(g, x0, w1)):
                gw2, gb2, g1 = mlp_bwd_fused(g, h1, w2, chunks, mask_in_bits=bits2, mask_out_bits=bits1, slope=slope)
                if ctx.needs_input_grad[0]:
                    gw1, gb1, g0 = mlp_bwd_fused(g1, x0, w1, chunks, slope=slope)
                else:
                    gw1, cs1 = rows_wgrad(g1, x0, chunks, 1, out_dtype=w1.dtype, colsum_of=1, colsum_lp=True)
                    gw1, gb1, g0 = gw1[0], cs1[0], None
                grads[2], grads[4] = gw1, gw2
                if ctx.has_bias[0]:
                    grads[3] = gb1.to(g.dtype)
                if ctx.has_bias[1]:
                    grads[5] = gb2.to(g.dtype)
                grads[0] = g0
                return tuple(grads)
            gw2, cs2 = rows_wgrad(g, h1, chunks, 1, out_dtype=w2.dtype, colsum_of=1, mask_a_bits=bits2, colsum_lp=True, slope=slope)
            g1, g0 = rows_chain2(g, w2, None, False, w1, None, False, mask0_bits=bits2, mask1_bits=bits1, w_kn=(True, True),
                                 slope=slope)
            gw1, cs1 = rows_wgrad(g1, x0, chunks, 1, out_dtype=w1.dtype, colsum_of=1, colsum_lp=True)
            grads[2], grads[4] = gw1[0], gw2[0]
            if ctx.has_bias[0]:
                grads[3] = cs1[0].to(g.dtype)
            if ctx.has_bias[1]:
                grads[5] = cs2[0].to(g.dtype)
            grads[0] = g0 if ctx.needs_input_grad[0] else None
            return tuple(grads)
        acts, ws = saved[:n + 1], saved[n + 1:]
        tiles, chunks = _dense_table(acts[0].shape[0], acts[0].device)
        for i in range(n - 1, -1, -1):
            w = ws[i]
            if i == n - 1:
                # outermost activation: masked while the rows are staged for the weight gradient, masked rows saved for the
                # input-gradient launch -- no separate elementwise pass
                gm = torch.empty_like(g)
                gw, cs = rows_wgrad(g, acts[i], chunks, 1, out_dtype=w.dtype, colsum_of=1, mask_a=acts[n], a_out=gm, slope=slope)
                g = gm
            else:
                gw, cs = rows_wgrad(g, acts[i], chunks, 1, out_dtype=w.dtype, colsum_of=1)   # g^T a_{i} ; colsum(g)
            grads[2 + 2 * i] = gw[0]
            if ctx.has_bias[i]:
                grads[3 + 2 * i] = cs[0].to(g.dtype)
            if i > 0 or ctx.needs_input_grad[0]:
                kn = g.dtype == torch.float32                   # fp32 kernels read Linear.weight [out = k][in = n] as it is
                g = rows_transform(g, (w if kn else w.t()).contiguous().unsqueeze(0), tiles, g.shape[0],
                                   mask_pos=acts[i] if i > 0 else None, slope=slope, w_kn=kn)   # masked for the activation below
        grads[0] = g if ctx.needs_input_grad[0] else None
        return tuple(grads)


# DN_LAYER_GRAPHS=0: inside _RginLayerSmallFn the conv and the MLP chain stay separate launches (dn_conv_graphs_bf16 + dn_rows_chain2_bf16)
LAYER_GRAPHS_ENABLED = _os.environ.get("DN_LAYER_GRAPHS", "1") != "0"
# DN_LAYER_SMALL=0: an H = 64 bf16 RGIN layer on small graphs stays a chain of separate autograd functions (conv, MLP)
LAYER_SMALL_ENABLED = _os.environ.get("DN_LAYER_SMALL", "1") != "0"


def rgin_layer_small_ok(x, W, W_loop, bias, linears, index_set):
    """Can a whole RGIN layer (conv + bias + 2-layer MLP + activations) run as _RginLayerSmallFn?  bf16, H = 64, square, self loop,
    two square Linears, a batch dn_conv_graphs_bf16 takes."""
    if not (LAYER_SMALL_ENABLED and CHAIN2_ENABLED and W_loop is not None and len(linears) == 2):
        return False
    if not (x.is_cuda and x.dtype == torch.bfloat16 and x.dim() == 2 and x.shape[1] == 64 and W.dtype == x.dtype
            and all(l.weight.dtype == x.dtype and tuple(l.weight.shape) == (64, 64) for l in linears)):
        return False
    return conv_graphs_ok(x, PassWeights(W, W_loop, kn=True), index_set.index)


class _RginLayerSmallFn(torch.autograd.Function):
    """act(lin2(act(lin1(conv(x))))) of an RGIN layer at the reference's default width on a batch of small graphs (rgin.py:102-160 +
    50-57, BASELINE config 3) as SEVEN launches a step: forward = the conv (dn_conv_graphs_bf16) + the MLP chain
    (dn_rows_chain2_bf16); backward = the chain's input gradients, the conv's input gradient (the same launch on the transposed
    weights), ONE weight-gradient launch for the conv's R + 1 matrices and both Linears (dn_rows_wgrad_multi_bf16) + its reduce --
    where the separate autograd functions need 11 launches plus the casts between them."""

    @staticmethod
    def forward(ctx, x, slope, index_set, W, W_loop, bias, w1, b1, w2, b2):
        ctx.f32_mode = f32_mode()
        x = x.contiguous()
        ix = index_set.index
        if LAYER_GRAPHS_ENABLED:
            h, h1, h2, bits1, bits2, aux = layer_graphs_fwd(x, W.contiguous(), W_loop.contiguous(), bias, w1.contiguous(), b1,
                                                            w2.contiguous(), b2, float(slope), ix)
        else:
            h = torch.empty_like(x)
            aux = conv_graphs(x, PassWeights(W, W_loop, kn=True), bias, ix, "f", h)
            h1, h2, bits1, bits2 = rows_chain2(h, w1, b1, True, w2, b2, True, want_bits=True, slope=float(slope))
        ctx.ix, ctx.slope = ix, float(slope)
        ctx.has = (bias is not None, b1 is not None, b2 is not None, aux is not None)
        ctx.save_for_backward(x, h, h1, bits1, bits2, W, W_loop, w1, w2, aux if aux is not None else x.new_empty(0))
        return h2

    @staticmethod
    @_backward_in_forward_mode
    def backward(ctx, gout):
        ix, slope = ctx.ix, ctx.slope
        x, h, h1, bits1, bits2, W, W_loop, w1, w2, aux = ctx.saved_tensors
        g = gout.contiguous()
        if LAYER_GRAPHS_ENABLED:
            g1, g0, gx, aux_b = layer_graphs_bwd(g, W.contiguous(), W_loop.contiguous(), w1.contiguous(), w2.contiguous(), slope, bits1, bits2,
                                                 ix)
        else:
            g1, g0 = rows_chain2(g, w2, None, False, w1, None, False, mask0_bits=bits2, mask1_bits=bits1, w_kn=(True, True), slope=slope)
            gx = torch.empty_like(x)
            aux_b = conv_graphs(g0, PassWeights(W, W_loop, kn=False), None, ix, "b", gx)
        grads = layer_wgrad(ix, "small", 64, W.dtype, ctx.has, dict(A=x, A2=aux if ctx.has[3] else None, G=g0, G2=aux_b, colsum_of=2),
                            dict(A=g1, G=h), dict(A=g, G=h1, mask_a_bits=bits2, slope=slope))
        return (gx, None, None, *grads)


# DN_LAYER_WIDE=0: an H = 256 bf16 RGIN layer stays a chain of separate autograd functions (conv, MLP), three weight-gradient launches
LAYER_WIDE_ENABLED = _os.environ.get("DN_LAYER_WIDE", "1") != "0"
# ... as it does above this many rows (the conv's + the two Linears'): every weight gradient of the layer is HBM-bound, so ONE launch
# saves the fixed costs of two (partial tiles written and reduced, ring fill and drain: 40 us of a 0.53-ms step on an eighth of
# config 5 -- one rank's share at 8 GPUs) and nothing else; on the whole batch (6.2 M rows) the mixed launch measured 25-55 us SLOWER
# than the three -- the gathered rows' share of Infinity-Cache hits does not survive the Linears' streams (docs/LAB_NOTES.md)
WIDE_LAYER_MAX_ROWS = int(_os.environ.get("DN_WIDE_MAX_ROWS", str(2 << 20)))


WIDE_DENSE_WEIGHT = float(_os.environ.get("DN_WIDE_DENSE_WEIGHT", "2"))


def wide_layer_chunks(rel_ptr_host, n_nodes, device, workgroups=256, dense_weight=None):
    """Split-K chunk table of _RginLayerWideFn's ONE weight-gradient launch: the conv's relation-major rows (rel_ptr_host: R + 1
    relations, the self loop last), then the two Linears' n_nodes rows each, in one virtual row space.  A workgroup's time is its
    tile count x what a tile of its kind costs, and a tile of rows in row order -- streamed from HBM, no second reader -- costs about
    twice a tile of gathered rows (which the L2s and the Infinity Cache serve in part): the Linears' chunks hold 1 / dense_weight of
    the rows of a conv chunk, and the chunk size is the smallest for which everything fits ONE round of `workgroups`.
    -> (chunks [C, 4] int32, chunk_ptr [R + 4] int32, C), as make_row_chunks."""
    w = float(dense_weight if dense_weight is not None else WIDE_DENSE_WEIGHT)
    conv = [int(b) - int(a) for a, b in zip(rel_ptr_host[:-1], rel_ptr_host[1:])]
    P_all, n = int(rel_ptr_host[-1]), int(n_nodes)
    dense_step = lambda c: max(64, int(c / w) // 32 * 32)                   # noqa: E731
    count = lambda c: sum(-(-m // c) for m in conv if m > 0) + 2 * (-(-n // dense_step(c)))   # noqa: E731
    c = max(256, -(-int((sum(conv) + 2 * w * n) // workgroups) // 64) * 64)
    while c < WGRAD_CHUNK_CAP and count(c) > workgroups:
        c += 64
    c = min(c, WGRAD_CHUNK_CAP)
    steps = [c] * len(conv) + [dense_step(c)] * 2
    vptr = [int(v) for v in rel_ptr_host] + [P_all + n, P_all + 2 * n]
    chunks, cptr = [], [0]
    for r, step in enumerate(steps):
        a, b = vptr[r], vptr[r + 1]
        while a < b:
            e = min(a + step, b)
            chunks.append((r, a, e, 0))
            a = e
        cptr.append(len(chunks))
    ch = torch.tensor(chunks if chunks else [(0, 0, 0, 0)], dtype=I32).reshape(-1, 4)
    return ch.to(device), torch.tensor(cptr, dtype=I32).to(device), len(chunks)


def layer_wgrad(ix, cut, H, out_dtype, has, conv, lin1, lin2):
    """The ONE weight-gradient launch of a layer function (rows_wgrad_multi) over the virtual row space of an index with a self loop:
    the conv's rows (relation-major, the self loop as relation R), then the two Linears' N dense rows each.  conv / lin1 / lin2 = the
    operands of the three jobs, has = (conv bias?, bias 1?, bias 2?, ...).  -> the gradients of (W, W_loop, bias, w1, b1, w2, b2).
    The split-K chunk table is built on first use and cached on the index PER CUT ("wide": wide_layer_chunks, H = 256; "small": equal
    steps for two rounds of workgroups, H = 64 / 128): a graph keeps one index for layers of every width, and a layer must get the
    table it would build on a fresh index whichever layer touched the batch first."""
    R, N, P_all, dev = ix.num_rels, ix.num_nodes, ix.num_rows, ix.row_in.device
    if cut not in ix._layer_chunks and cut == "wide":
        ix._layer_chunks[cut] = wide_layer_chunks(list(ix.rel_ptr_host)[:R + 2], N, dev)
    elif cut not in ix._layer_chunks:
        vptr_host = list(ix.rel_ptr_host) + [P_all + N, P_all + 2 * N]
        vptr = torch.cat([ix.rel_ptr_dev[:R + 2], torch.tensor([P_all + N, P_all + 2 * N], dtype=I32, device=dev)])
        ix._layer_chunks[cut] = build_row_tables(vptr, R + 3, P_all + 2 * N, wgrad_chunk_rows(vptr_host, _SMALL_WG), want_ptr=True)
    jobs = [dict(idx_a=ix.row_in, idx_g=ix.row_out, first_rel=0, row0=0, **conv),
            dict(colsum_of=1, first_rel=R + 1, row0=P_all, **lin1),
            dict(colsum_of=1, first_rel=R + 2, row0=P_all + N, **lin2)]
    gw, cs = rows_wgrad_multi(jobs, ix._layer_chunks[cut], R + 3, H, out_dtype)
    return (gw[:R], gw[R], cs[R] if has[0] else None, gw[R + 1], cs[R + 1] if has[1] else None, gw[R + 2],
            cs[R + 2] if has[2] else None)


def rgin_layer_wide_ok(x, W, W_loop, bias, linears, index_set):
    """Can a whole RGIN layer run as _RginLayerWideFn?  bf16, H = 256, square, self loop, two square Linears, one index part on the
    closing-launch path (the benchmarked configuration: BASELINE config 5)."""
    if not (LAYER_WIDE_ENABLED and CHAIN2_ENABLED and W_loop is not None and len(linears) == 2):
        return False
    if not (x.is_cuda and x.dtype == torch.bfloat16 and x.dim() == 2 and x.shape[1] == 256 and W.dtype == x.dtype
            and tuple(W.shape[1:]) == (256, 256) and x.shape[0] > 0
            and all(l.weight.dtype == x.dtype and tuple(l.weight.shape) == (256, 256) for l in linears)):
        return False
    ix = index_set.index
    return _selfsum_ok(ix, x) and 0 < ix.num_rows and ix.num_rows + 2 * x.shape[0] <= WIDE_LAYER_MAX_ROWS


class _RginLayerWideFn(torch.autograd.Function):
    """act(lin2(act(lin1(conv(x))))) of an RGIN layer at H = 256 in bf16 (rgin.py:102-160 + 50-57, BASELINE config 5) with the
    launches of the separate functions (_RowTransformFn: transform + closing launch per direction; _ReluMlpFn: one chain launch per
    direction) and ONE weight-gradient launch for the conv's R + 1 matrices and both Linears (dn_rows_wgrad_multi_bf16 at H = 256)
    at the end of the backward pass: the Linears' rows, which no one reads twice, stream from HBM under the conv's matrix work on
    rows the L2s serve, and one round of partial tiles is written and reduced instead of three."""

    @staticmethod
    def forward(ctx, x, slope, index_set, W, W_loop, bias, w1, b1, w2, b2):
        ctx.f32_mode = f32_mode()
        x = x.contiguous()
        ix = index_set.index
        pw = PassWeights(W, W_loop, kn=True)
        if not _kn_ok(x):
            pw = pw.nk()
        h = torch.empty_like(x)
        aux = message_pass(x, pw, bias, ix, "f", index_set.ybuf(256, x.dtype, x.device), h)
        h1, h2, bits1, bits2 = rows_chain2(h, w1, b1, True, w2, b2, True, want_bits=True, slope=float(slope))
        ctx.index_set, ctx.slope = index_set, float(slope)
        ctx.has = (bias is not None, b1 is not None, b2 is not None, aux is not None)
        ctx.save_for_backward(x, h, h1, bits1, bits2, W, W_loop, w1, w2, aux if aux is not None else x.new_empty(0))
        return h2

    @staticmethod
    @_backward_in_forward_mode
    def backward(ctx, gout):
        iset, slope = ctx.index_set, ctx.slope
        ix = iset.index
        x, h, h1, bits1, bits2, W, W_loop, w1, w2, aux = ctx.saved_tensors
        g = gout.contiguous()
        H, R = 256, W.shape[0]
        g1, g0 = rows_chain2(g, w2, None, False, w1, None, False, mask0_bits=bits2, mask1_bits=bits1, w_kn=(True, True), slope=slope)
        gx = torch.empty_like(x)
        aux_b = message_pass(g0, PassWeights(W, W_loop, kn=False), None, ix, "b", iset.ybuf(H, g.dtype, g.device), gx)
        # (bias gradient = column sum of g0 over the self-loop rows: relation R of the conv's job)
        grads = layer_wgrad(ix, "wide", H, W.dtype, ctx.has,
                            dict(A=x, A2=aux if ctx.has[3] else None, G=g0, G2=aux_b, colsum_of=2 | ((R + 1) << 8)),
                            dict(A=g1, G=h), dict(A=g, G=h1, mask_a_bits=bits2, slope=slope))
        return (gx if ctx.needs_input_grad[0] else None, None, None, *grads)


def rgin_layer_wide(x, W, W_loop, bias, linears, slope, index_set):
    """The whole RGIN layer of rgin_layer_wide_ok's case as one autograd function (_RginLayerWideFn)."""
    return _RginLayerWideFn.apply(x, float(slope), index_set, W, W_loop, bias, linears[0].weight, linears[0].bias,
                                  linears[1].weight, linears[1].bias)


# DN_LAYER_CHAIN_WGRAD=0: an H = 256 bf16 RGIN layer on a large batch stays a chain of separate autograd functions (conv, MLP) whose
# backward takes Linear 1's weight gradient from its own pass over the rows of h (dn_mlp_bwd_fused_bf16's second launch) instead of
# deriving it from the conv's (_RginLayerChainFn: step 2.991 -> 2.892 ms on one box, docs/LAB_NOTES.md round 8) -- for A/B runs and the tests
LAYER_CHAIN_WGRAD_ENABLED = _os.environ.get("DN_LAYER_CHAIN_WGRAD", "1") != "0"


def _chain_seg_tiles(ix, fold):
    """Tile table of dn_layer_chain_dgrad_bf16 for the backward fold of an index whose every graph fits one tile: per graph
    {0, first node, end node, s0 | s1 << 8} with [s0, s1) = where the graph's aux_b list (a contiguous ascending run: the fold's
    verdict) lies inside the tile.  Built on first use (a few elementwise launches, no read-back), kept on the fold."""
    if fold.seg_tiles is None:
        n, v = fold.n, ix.dirs["b"]
        tp, ap = fold.graph_tiles[0][:n + 1], v.aux_ptr[:n + 1]
        beg, end = tp[:n], tp[1:]
        s0 = v.aux_idx[ap[:n].long()] - beg
        seg = s0 | ((s0 + (ap[1:] - ap[:n])) << 8)
        fold.seg_tiles = torch.stack([torch.zeros_like(beg), beg, end, seg], 1).to(I32).contiguous()
    return fold.seg_tiles


def layer_chain_dgrad(g1, w1, seg_tiles):
    """g0 = g1 @ w1 (w1: Linear.weight as stored, [out, in]) on the dense ring transform over seg_tiles (_chain_seg_tiles), and from
    the same pass the bf16 sums of g1 over every tile's segment in row order (dn_layer_chain_dgrad_bf16).  -> (g0, sums [T, H]).
    g0 is bit-identical to mlp_bwd_fused's unmasked g_next, the sums to gather_segsum over the same lists."""
    g1, w1 = g1.contiguous(), w1.contiguous()
    require_gpu(g1, w1, seg_tiles)
    N, H = g1.shape
    T = int(seg_tiles.shape[0])
    assert g1.dtype == torch.bfloat16 and w1.dtype == g1.dtype and H == 256 and tuple(w1.shape) == (H, H)
    assert seg_tiles.dtype == I32 and seg_tiles.dim() == 2 and seg_tiles.shape[1] == 4 and seg_tiles.is_contiguous()
    g0 = torch.empty_like(g1)
    sums = torch.empty((T, H), dtype=g1.dtype, device=g1.device)

    def _launch():
        check(lib().dn_layer_chain_dgrad_bf16(ptr(g1), ptr(w1), N, H, ptr(seg_tiles), T, ptr(g0), ptr(sums), stream_ptr()),
              "dn_layer_chain_dgrad_bf16")
    launch_tagged("chain_dgrad", _launch)
    return g0, sums


def layer_chain_wgrad_combine(M, c, w1, W, W_loop, bias):
    """The parameter gradients of the conv and of Linear 1 from M [R + 1, H, H] = A_r^T g1 (fp32, the self loop last) and c = colsum(g1)
    (fp32 [H]): dWc_r = M_r w1, db = c w1, dW1 = sum_r M_r^T Wc_r + c b^T, db1 = c  (dn_layer_chain_wgrad_combine; bf16 out of fp64
    sums of the exact products, one rounding each, fixed order).  -> (dWc [R + 1, H, H], db [H] or None, dW1 [H, H], db1 [H])."""
    M, c, w1, W, W_loop = M.contiguous(), c.contiguous(), w1.contiguous(), W.contiguous(), W_loop.contiguous()
    require_gpu(M, c, w1, W, W_loop, bias)
    R, H = W.shape[0], 256
    assert M.dtype == torch.float32 and tuple(M.shape) == (R + 1, H, H) and c.dtype == torch.float32 and c.numel() == H
    assert w1.dtype == torch.bfloat16 and tuple(w1.shape) == (H, H) and W.dtype == w1.dtype and tuple(W.shape[1:]) == (H, H)
    assert W_loop.dtype == w1.dtype and tuple(W_loop.shape) == (H, H)
    assert bias is None or (bias.dtype == w1.dtype and bias.numel() == H and bias.is_contiguous())
    dev = M.device
    dWc = torch.empty((R + 1, H, H), dtype=w1.dtype, device=dev)
    dW1 = torch.empty((H, H), dtype=w1.dtype, device=dev)
    db = torch.empty((H,), dtype=w1.dtype, device=dev) if bias is not None else None
    db1 = torch.empty((H,), dtype=w1.dtype, device=dev)
    ws = _ws(lib().dn_layer_chain_wgrad_combine_workspace_bytes(R, H), dev)

    def _launch():
        check(lib().dn_layer_chain_wgrad_combine(ptr(M), ptr(c), ptr(w1), ptr(W), ptr(W_loop), ptr(bias), R, H, ptr(dWc), ptr(db), ptr(dW1),
                                                 ptr(db1), ptr(ws), ws.numel(), stream_ptr()), "dn_layer_chain_wgrad_combine")
    launch_tagged("chain_combine", _launch)
    return dWc, db, dW1, db1


def rgin_layer_chain_ok(x, W, W_loop, bias, linears, index_set):
    """Can a whole RGIN layer run as _RginLayerChainFn?  bf16, H = 256, square, self loop, conv bias, two square Linears with biases,
    x wants a gradient, a batch of at least MLP_BWD_FUSED_MIN_ROWS rows above _RginLayerWideFn's range, one index part on the
    unit-stream closing path whose fold is absorbed by single-tile AGG units in both directions (every graph within 32 nodes)."""
    if not (LAYER_CHAIN_WGRAD_ENABLED and MLP_BWD_FUSED_ENABLED and CHAIN2_ENABLED and W_loop is not None and bias is not None
            and len(linears) == 2 and all(l.bias is not None for l in linears)):
        return False
    if not (x.is_cuda and x.dtype == torch.bfloat16 and x.dim() == 2 and x.shape[1] == 256 and W.dtype == x.dtype
            and tuple(W.shape[1:]) == (256, 256) and tuple(W_loop.shape) == (256, 256) and W_loop.dtype == x.dtype
            and bias.dtype == x.dtype and x.requires_grad and torch.is_grad_enabled()
            and all(l.weight.dtype == x.dtype and l.bias.dtype == x.dtype and tuple(l.weight.shape) == (256, 256) for l in linears)):
        return False
    ix = index_set.index
    N = x.shape[0]
    if not (_selfsum_ok(ix, x) and _kn_ok(x) and N >= max(MLP_BWD_FUSED_MIN_ROWS, 1) and ix.num_rows + 2 * N > WIDE_LAYER_MAX_ROWS
            and _close_kind(256, x.dtype) == "units" and not conv_graphs_ok(x, PassWeights(W, W_loop, kn=True), ix)):
        return False
    for d in ("f", "b"):
        fold = _row_index_fold(ix, d, "units")
        if fold is None or fold.graph_tiles is None or fold.multi is not None or not ix.close_units(d).agg:
            return False
    return ix.dirs["b"].n_aux == ix._fold["b"].n


class _RginLayerChainFn(torch.autograd.Function):
    """act(lin2(act(lin1(conv(x))))) of an RGIN layer at H = 256 in bf16 on a large batch (rgin.py:102-160 + 50-57, BASELINE config 5)
    with the forward launches of the separate functions (_RowTransformFn + _ReluMlpFn) and a backward that never reads the conv's
    output h: nothing lies between h and Linear 1, so with g1 = the gradient of Linear 1's output and M_r = A_r^T g1
        dWc_r = M_r W1,  db = colsum(g1) W1,  dW1 = sum_r M_r^T Wc_r + colsum(g1) b^T,  db1 = colsum(g1)
    -- backward = dn_mlp_bwd_fused_bf16 (layer 2, masked: dW2, db2, g1), dn_layer_chain_dgrad_bf16 (g0 = g1 W1 + the per-graph sums
    of g1), the conv's input-gradient launches on g0 as ever, the conv's weight-gradient launch on g1 (fp32 out) and
    dn_layer_chain_wgrad_combine: 35 products of 256^3 in place of the weight-gradient half of a pass over every row."""

    @staticmethod
    def forward(ctx, x, slope, index_set, W, W_loop, bias, w1, b1, w2, b2):
        ctx.f32_mode = f32_mode()
        x = x.contiguous()
        ix = index_set.index
        h = torch.empty_like(x)
        aux = message_pass(x, PassWeights(W, W_loop, kn=True), bias, ix, "f", index_set.ybuf(256, x.dtype, x.device), h)
        h1, h2, bits1, bits2 = rows_chain2(h, w1, b1, True, w2, b2, True, want_bits=True, slope=float(slope))
        ctx.index_set, ctx.slope = index_set, float(slope)
        ctx.save_for_backward(x, h1, bits1, bits2, W, W_loop, bias, w1, w2, aux if aux is not None else x.new_empty(0))
        return h2

    @staticmethod
    @_backward_in_forward_mode
    def backward(ctx, gout):
        iset, slope = ctx.index_set, ctx.slope
        ix = iset.index
        x, h1, bits1, bits2, W, W_loop, bias, w1, w2, aux = ctx.saved_tensors
        g = gout.contiguous()
        H, R = 256, W.shape[0]
        _, chunks = _dense_table(x.shape[0], x.device)
        gw2, gb2, g1 = mlp_bwd_fused(g, h1, w2, chunks, mask_in_bits=bits2, mask_out_bits=bits1, slope=slope)
        g0, g1_sums = layer_chain_dgrad(g1, w1, _chain_seg_tiles(ix, ix._fold["b"]))
        gx = torch.empty_like(x)
        message_pass(g0, PassWeights(W, W_loop, kn=False), None, ix, "b", iset.ybuf(H, g.dtype, g.device), gx)
        # the conv's weight-gradient launch as ever, on g1: M_r = A_r^T g1 in fp32, c = colsum(g1) over the self-loop rows
        M, cs = rows_wgrad(x, g1, ix.chunk_table, R + 1, idx_a=ix.row_in, idx_g=ix.row_out, A2=aux if ix.num_aux_f else None,
                           G2=g1_sums, out_dtype=torch.float32, colsum_of=2, colsum_rel=R)
        gAll, gb, gw1, gb1 = layer_chain_wgrad_combine(M, cs[R], w1, W, W_loop, bias)
        return (gx, None, None, gAll[:R], gAll[R], gb, gw1, gb1, gw2, gb2.to(g.dtype))


def rgin_layer_chain(x, W, W_loop, bias, linears, slope, index_set):
    """The whole RGIN layer of rgin_layer_chain_ok's case as one autograd function (_RginLayerChainFn)."""
    return _RginLayerChainFn.apply(x, float(slope), index_set, W, W_loop, bias, linears[0].weight, linears[0].bias,
                                   linears[1].weight, linears[1].bias)


LAYER_F32_ENABLED = _os.environ.get("DN_LAYER_F32", "1") != "0"
CHAIN2_F32_ENABLED = _os.environ.get("DN_CHAIN2_F32", "1") != "0"          # 0: the fp32 layer function keeps one launch per Linear


def rgin_layer_f32_ok(x, W, W_loop, bias, linears, index_set):
    """Can a whole fp32 RGIN layer run as _RginLayerF32Fn?  The reference's precision on the bf16 split (not the exact-f32 mode),
    H = 64 / 128, square, self loop, two square Linears, one part."""
    if not (LAYER_F32_ENABLED and W_loop is not None and len(linears) == 2 and not f32_mode()):
        return False
    H = x.shape[1] if x.dim() == 2 else 0
    ok = lambda t: t is None or (t.is_cuda and t.dtype == torch.float32)  # noqa: E731
    return (x.is_cuda and x.dtype == torch.float32 and H in (64, 128) and x.shape[0] > 0 and tuple(W.shape[1:]) == (H, H)
            and W.dtype == x.dtype and tuple(W_loop.shape) == (H, H) and ok(W_loop) and ok(bias)
            and all(ok(l.weight) and ok(l.bias) and tuple(l.weight.shape) == (H, H) for l in linears)
            and index_set.index.num_rows > 0 and _kn_ok(x))


class _RginLayerF32Fn(torch.autograd.Function):
    """act(lin2(act(lin1(conv(x))))) of an RGIN layer in the reference's own precision (fp32 on the 3-term bf16 split) at H = 64 / 128
    (rgin.py:102-160 + 50-57; BASELINE config 3 as the reference runs it) as ONE autograd function: the forward launches are those of
    _RowTransformFn + _ReluMlpFn; the backward masks the incoming gradient once (dn_relu_bwd_f32), runs the two input-gradient launches
    (the inner mask in the first one's epilogue), the conv's input-gradient pass, and then ONE weight-gradient launch + ONE reduce for
    the conv's R + 1 matrices and both Linears (dn_rows_wgrad_multi_f32) where the separate functions take three of each."""

    @staticmethod
    def forward(ctx, x, slope, index_set, W, W_loop, bias, w1, b1, w2, b2, residual=False):
        ctx.f32_mode = f32_mode()
        x = x.contiguous()
        ix = index_set.index
        N, H = x.shape
        slope = float(slope)
        h = torch.empty_like(x)
        aux = message_pass(x, PassWeights(W, W_loop, kn=True), bias, ix, "f", index_set.ybuf(H, x.dtype, x.device), h)
        ctx.residual = bool(residual)
        out = None
        if CHAIN2_F32_ENABLED and residual:             # x + layer(x): the sum leaves the MLP launch next to the activation
            h1, h2, out = rows_chain2_f32(h, w1, b1, True, w2, b2, True, slope=slope, residual=x)
        elif CHAIN2_F32_ENABLED:
            h1, h2 = rows_chain2_f32(h, w1, b1, True, w2, b2, True, slope=slope)
        else:
            tiles, _ = _dense_table(N, x.device)
            h1 = rows_transform(h, w1.contiguous().unsqueeze(0), tiles, N, bias=None if b1 is None else b1.contiguous().view(1, -1), relu=True,
                                slope=slope)
            h2 = rows_transform(h1, w2.contiguous().unsqueeze(0), tiles, N, bias=None if b2 is None else b2.contiguous().view(1, -1), relu=True,
                                slope=slope)
        ctx.index_set, ctx.slope = index_set, slope
        ctx.has = (bias is not None, b1 is not None, b2 is not None, aux is not None)
        ctx.save_for_backward(x, h, h1, h2, W, W_loop, w1, w2, aux if aux is not None else x.new_empty(0))
        if residual:
            if out is None:
                out = h2 + x
            return out
        return h2

    @staticmethod
    @_backward_in_forward_mode
    def backward(ctx, gout):
        iset, slope = ctx.index_set, ctx.slope
        ix = iset.index
        x, h, h1, h2, W, W_loop, w1, w2, aux = ctx.saved_tensors
        N, H = x.shape
        g = gout.contiguous()
        if CHAIN2_F32_ENABLED:
            # outer mask, dgrad 2, inner mask, dgrad 1 in ONE launch; the weight gradient of Linear 2 masks g itself (mask = the saved output)
            gm1, g0 = rows_chain2_f32(g, w2, None, False, w1, None, False, mask0=h2, mask1=h1, w_kn=(True, True), slope=slope)
            job2 = dict(A=g, G=h1, mask_a_bits=h2, slope=slope)
        else:
            tiles, _ = _dense_table(N, x.device)
            gm2 = relu_bwd(g, h2, slope)                                    # the outer activation's mask
            gm1 = rows_transform(gm2, w2.contiguous().unsqueeze(0), tiles, N, mask_pos=h1, slope=slope, w_kn=True)   # masked for the inner one
            g0 = rows_transform(gm1, w1.contiguous().unsqueeze(0), tiles, N, w_kn=True)
            job2 = dict(A=gm2, G=h1)
        gx = torch.empty_like(x)
        # (residual: the gradient of x + layer(x) is g + the layer's input gradient -- g rides in the conv's closing gather)
        aux_b = message_pass(g0, PassWeights(W, W_loop, kn=False), None, ix, "b", iset.ybuf(H, x.dtype, x.device), gx,
                             add_in=g if ctx.residual else None)
        grads = layer_wgrad(ix, "small", H, torch.float32, ctx.has, dict(A=x, A2=aux if ctx.has[3] else None, G=g0, G2=aux_b, colsum_of=2),
                            dict(A=gm1, G=h), job2)
        return (gx, None, None, *grads, None)


def rgin_layer_f32(x, W, W_loop, bias, linears, slope, index_set, residual=False):
    """residual: return x + layer(x) (the representation nets' residual connection) from the same launches."""
    return _RginLayerF32Fn.apply(x, float(slope), index_set, W, W_loop, bias, linears[0].weight, linears[0].bias, linears[1].weight,
                                 linears[1].bias, bool(residual))


def rgin_layer_small(x, W, W_loop, bias, linears, slope, index_set):
    return _RginLayerSmallFn.apply(x, float(slope), index_set, W, W_loop, bias, linears[0].weight, linears[0].bias, linears[1].weight,
                                   linears[1].bias)


def relu_mlp_supported(x, linears):
    return (x.is_cuda and x.dtype in MFMA_DTYPES and x.dim() == 2 and x.shape[0] > 0 and len(linears) > 0
            and all(l.weight.dtype == x.dtype and l.weight.shape[0] == l.weight.shape[1] == x.shape[1]
                    and x.shape[1] in (64, 128, 256) for l in linears))


def relu_mlp(x, linears, slope=0.0):
    """act(lin_L(... act(lin_1(x)))) through _ReluMlpFn; slope 0 = ReLU, > 0 = leaky ReLU."""
    wb = []
    for l in linears:
        wb += [l.weight, l.bias]
    return _ReluMlpFn.apply(x, float(slope), *wb)


def linear_act(x, weight, bias=None, relu=False, exact=None):
    """nn.Linear (+ ReLU) on the MFMA kernels when supported (bf16 / fp32, square 64/128/256), else torch.  exact: force the
    exact-f32 MFMA (True) or the bf16 split (False) for fp32 operands; None = the module default (ops.F32_EXACT)."""
    if (x.is_cuda and x.dtype == weight.dtype and x.dtype in MFMA_DTYPES and x.dim() == 2
            and weight.shape[0] == weight.shape[1] and weight.shape[0] in (64, 128, 256) and x.shape[1] == weight.shape[1]
            and x.shape[0] > 0):
        return _LinearActFn.apply(x, weight, bias, relu, exact)
    y = torch.nn.functional.linear(x, weight, bias)
    return torch.relu(y) if relu else y


# ----------------------------------------------------------------------------------------------
# dense side of the GC models: BatchNorm over the nodes of the batch, Linear of any width
# ----------------------------------------------------------------------------------------------
class _BatchNormRowsFn(torch.autograd.Function):
    """Training-mode BatchNorm over the rows of [N, C] (dn_batchnorm_rows_*): returns (y, mean, biased var)."""

    @staticmethod
    def forward(ctx, x, weight, bias, eps, running_mean=None, running_var=None, momentum=0.0, relu=False, batches_tracked=None):
        x = x.contiguous()
        N, C = x.shape
        if batches_tracked is not None:
            require_gpu(batches_tracked)
            assert batches_tracked.dtype == torch.int64 and batches_tracked.numel() == 1
        if running_mean is not None:
            assert running_mean.dtype == torch.float32 and running_var.dtype == torch.float32
            assert running_mean.is_contiguous() and running_var.is_contiguous() and running_mean.numel() == C
        w32 = weight.detach().float().contiguous() if weight is not None else None
        b32 = bias.detach().float().contiguous() if bias is not None else None
        y = torch.empty_like(x)
        mean, var, rstd = (torch.empty(C, dtype=torch.float32, device=x.device) for _ in range(3))
        ws = _ws(lib().dn_batchnorm_rows_workspace_bytes(N, C), x.device)
        check(getattr(lib(), "dn_batchnorm_rows_" + _suffix(x))(ptr(x), N, C, ptr(w32), ptr(b32), float(eps), ptr(y), ptr(mean), ptr(var),
                                                               ptr(rstd), ptr(running_mean), ptr(running_var), float(momentum),
                                                               1 if relu else 0, ptr(batches_tracked), ptr(ws), ws.numel(),
                                                               stream_ptr()),
              "dn_batchnorm_rows")
        ctx.relu = bool(relu)
        ctx.save_for_backward(x, mean, rstd, w32 if w32 is not None else x.new_empty(0),
                              b32 if (relu and b32 is not None) else x.new_empty(0))
        ctx.has_w, ctx.has_b = weight is not None, bias is not None
        ctx.wdtype = weight.dtype if weight is not None else None
        ctx.mark_non_differentiable(mean, var)
        ctx.set_materialize_grads(False)                      # (no zero tensors for the statistics outputs' "gradients": 2 fills a call)
        return y, mean, var

    @staticmethod
    def backward(ctx, dy, _dm, _dv):
        x, mean, rstd, w32, b32 = ctx.saved_tensors
        if dy is None:
            return (None,) * 9
        dy = dy.contiguous()
        N, C = x.shape
        dx = torch.empty_like(x)
        s1, s2 = (torch.empty(C, dtype=torch.float32, device=x.device) for _ in range(2))
        ws = _ws(lib().dn_batchnorm_rows_workspace_bytes(N, C), x.device)
        check(getattr(lib(), "dn_batchnorm_rows_bwd_" + _suffix(x))(ptr(dy), ptr(x), N, C, ptr(mean), ptr(rstd),
                                                                   ptr(w32) if ctx.has_w else None,
                                                                   ptr(b32) if (ctx.relu and ctx.has_b) else None,
                                                                   1 if ctx.relu else 0, ptr(dx), ptr(s1), ptr(s2), ptr(ws),
                                                                   ws.numel(), stream_ptr()), "dn_batchnorm_rows_bwd")
        gw = s2.to(ctx.wdtype) if ctx.has_w else None
        gb = s1.to(ctx.wdtype if ctx.has_w else dy.dtype) if ctx.has_b else None
        return dx, gw, gb, None, None, None, None, None, None


def batch_norm_rows_supported(x):
    return (x.is_cuda and x.dim() == 2 and x.dtype in (torch.float32, torch.bfloat16) and x.shape[0] >= 1
            and x.shape[1] % 4 == 0 and 4 <= x.shape[1] <= 1024)


def batch_norm_rows(x, weight, bias, eps=1e-5, running_mean=None, running_var=None, momentum=0.0, relu=False, batches_tracked=None):
    """(y, batch mean, biased batch variance) of training-mode BatchNorm over the rows of x; relu: y = ReLU(BatchNorm(x)) in the
    same launches, forward and backward.  running_mean / running_var (fp32 buffers, optional) are updated in place by the
    statistics launch: r = (1 - momentum) r + momentum * new, unbiased variance; batches_tracked (int64 [1], optional): + 1."""
    return _BatchNormRowsFn.apply(x, weight, bias, eps, running_mean, running_var, momentum, relu, batches_tracked)


_single_rel_tables = {}


def _single_rel_table(n_rows, dev):
    """Device tile / chunk tables of ONE relation of n_rows rows for the any-width products (cached per size and device)."""
    key = (int(n_rows), str(dev))
    t = _single_rel_tables.get(key)
    if t is None:
        rp = torch.tensor([0, int(n_rows)], dtype=I32).to(dev)
        # (at least 64 rows a chunk: the any-width weight gradient walks a chunk in dependent 16-row steps -- load, barrier, multiply --
        #  so a 128-row chunk was eight round trips of latency: GIN steps under replay 0.355 -> 0.334 ms / 0.647 -> 0.636 / 0.838 -> 0.816)
        chunk = max(64, min(2048, -(-int(n_rows) // 256 // 64) * 64))
        t = (build_row_tables(rp, 1, n_rows, 64), build_row_tables(rp, 1, n_rows, chunk, want_ptr=True))
        if len(_single_rel_tables) > 8:
            _single_rel_tables.clear()
        _single_rel_tables[key] = t
    return t


class _LinearAnyFn(torch.autograd.Function):
    """y = x @ weight^T (+ bias) for any in / out widths on dn_rows_gemm_* / dn_rows_wgrad_any_* (weight [out, in], nn.Linear
    layout).  The library GEMMs torch picks for a [20 k x 5] x [5 x 128] product and its [128 x 20 k] x [20 k x 5] weight
    gradient take 20-80 us each; these are single small launches."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        ctx.f32_mode = f32_mode()
        x = x.contiguous()
        tiles, _ = _single_rel_table(x.shape[0], x.device)
        y = rows_gemm(x, weight.contiguous().unsqueeze(0), tiles, transpose_w=True,          # W[0] is [N, K] = [out, in]
                      bias=None if bias is None else bias.contiguous().view(1, -1))
        ctx.has_bias = bias is not None
        ctx.save_for_backward(x, weight)
        return y

    @staticmethod
    @_backward_in_forward_mode
    def backward(ctx, g):
        x, weight = ctx.saved_tensors
        g = g.contiguous()
        tiles, chunks = _single_rel_table(x.shape[0], x.device)
        gx = gw = gb = None
        if ctx.needs_input_grad[0]:
            gx = rows_gemm(g, weight.contiguous().unsqueeze(0), tiles)                       # g [P, out] @ W [out, in]
        need_b = ctx.has_bias and ctx.needs_input_grad[2]
        if ctx.needs_input_grad[1] or need_b:                                                # g^T x -> [out, in]; colsum(g) -> bias
            gw, cs = rows_wgrad_any(g, x, chunks, 1, want_colsum=True)
            gw = gw[0]
            if need_b:
                gb = cs[0].to(g.dtype)
        return gx, gw, gb


def linear_any(x, weight, bias=None, exact=None):
    """nn.Linear on the HIP path whatever its widths: matrix cores when square 64 / 128 / 256, the any-width kernels otherwise.
    exact: fp32 arithmetic of the matrix-core path (None = module default, True = exact f32, False = bf16 split)."""
    if (x.is_cuda and x.dim() == 2 and x.shape[0] > 0 and x.dtype == weight.dtype and x.dtype in MFMA_DTYPES):
        if weight.shape[0] == weight.shape[1] and weight.shape[0] in (64, 128, 256) and x.shape[1] == weight.shape[1]:
            return _LinearActFn.apply(x, weight, bias, False, exact)
        return _LinearAnyFn.apply(x, weight, bias)
    return torch.nn.functional.linear(x, weight, bias)


# ----------------------------------------------------------------------------------------------
# SI count models: the glue of GraphAdjModel.forward around the rep nets (dn_simodel.hip)
# ----------------------------------------------------------------------------------------------
SI_FLAGS = ((1, "a node label outside the label table"), (2, "a node id outside the id table"),
            (4, "a pattern with no nodes"), (8, "a graph with no nodes"), (16, "inconsistent node_ptr"))


def _u8_or_none(t):
    """The is_dummy node flag as uint8 [N] (bool is viewed, not copied)."""
    if t is None:
        return None
    t = t.reshape(-1)
    if t.dtype == torch.bool:
        return t.view(torch.uint8)
    if t.dtype != torch.uint8:
        raise _lib.DnHipError("dummy flags must be bool or uint8 on the device (got %s)" % t.dtype)
    return t


def si_filter_meta(p_ptr, p_label, p_id, g_ptr, g_label, g_id, p_sizes, g_sizes, gate_dtype=None):
    """(meta int32 [4] on the device = {Lp, Lg, flags, 0}, gate [Ng, 1] in gate_dtype or None) -- dn_si_filter_meta_*.  The
    table sizes are (labels, ids) per side; ids / labels outside them, zero-node graphs and broken ptrs set flag bits."""
    require_gpu(p_ptr, p_label, p_id, g_ptr, g_label, g_id)
    for t, n in ((p_ptr, "p_ptr"), (p_label, "p_label"), (p_id, "p_id"), (g_ptr, "g_ptr"), (g_label, "g_label"), (g_id, "g_id")):
        _i32(t, n)
    B = p_ptr.numel() - 1
    if B < 1 or g_ptr.numel() != B + 1:
        raise _lib.DnHipError("si_filter_meta: pattern and graph batches need the same B >= 1 graphs")
    meta = torch.empty(4, dtype=I32, device=p_ptr.device)
    gate = None
    dt = gate_dtype if gate_dtype is not None else torch.float32
    if gate_dtype is not None:
        gate = torch.empty((g_label.numel(), 1), dtype=gate_dtype, device=g_label.device)
    fn = getattr(lib(), "dn_si_filter_meta_" + ("bf16" if dt == torch.bfloat16 else "f32"))

    def _launch():
        check(fn(B, ptr(p_ptr), ptr(p_label), ptr(p_id), p_label.numel(), ptr(g_ptr), ptr(g_label), ptr(g_id), g_label.numel(),
                 int(p_sizes[0]), int(p_sizes[1]), int(g_sizes[0]), int(g_sizes[1]), ptr(gate), ptr(meta), stream_ptr()),
              "dn_si_filter_meta")
    launch_tagged("si_filter" if gate is not None else "si_meta", _launch)
    return meta, gate


def si_read_meta(meta):
    """THE device-to-host read of an SI model forward: (Lp, Lg); raises on the flags the kernels set (ValueError for zero-node
    graphs, whose padded mask the reference gets wrong; DnHipError for ids / labels / ptrs out of range)."""
    lp, lg, flags, _ = meta.tolist()
    if flags:
        what = "; ".join(m for bit, m in SI_FLAGS if flags & bit)
        if flags & (4 | 8):
            raise ValueError("SI model batch: %s" % what)
        raise _lib.DnHipError("SI model batch: %s" % what)
    return int(lp), int(lg)


def _embed_tables(parts):
    """parts: [(key int32 [N], enc [rows, K], W [K, H])] -> flat launch arguments of one or two tables."""
    args = []
    for i in range(2):
        if i < len(parts):
            key, enc, W = parts[i]
            args += [ptr(key), ptr(enc), int(enc.shape[0]), int(enc.shape[1]), ptr(W)]
        else:
            args += [None, None, 0, 0, None]
    return args


class _SiEmbedFn(torch.autograd.Function):
    """emb[v] = enc_vl[label_v] @ W_vl (+ enc_v[id_v] @ W_v): dn_si_embed_fwd_* / dn_si_embed_wgrad_*.  The enc tables are frozen
    (basemodel.py:669-670): no gradient to them or to the keys."""

    @staticmethod
    def forward(ctx, key1, enc1, W1, key2, enc2, W2):
        parts = [(key1, enc1.contiguous(), W1.contiguous())]
        if key2 is not None:
            parts.append((key2, enc2.contiguous(), W2.contiguous()))
        require_gpu(*[t for p in parts for t in p])
        for key, enc, W in parts:
            _i32(key, "key")
            if enc.dtype != W.dtype or W.shape[0] != enc.shape[1] or key.numel() != key1.numel():
                raise _lib.DnHipError("si_embed: enc [rows, K], W [K, H] of one dtype and one key per row expected")
        N, H = key1.numel(), int(W1.shape[1])
        if key2 is not None and W2.shape[1] != H:
            raise _lib.DnHipError("si_embed: both tables must embed into the same width")
        out = torch.empty((N, H), dtype=W1.dtype, device=W1.device)
        fn = getattr(lib(), "dn_si_embed_fwd_" + _suffix(W1))
        launch_tagged("si_embed", lambda: check(fn(N, H, *_embed_tables(parts), ptr(out), stream_ptr()), "dn_si_embed_fwd"))
        ctx.parts = len(parts)
        ctx.save_for_backward(*[t for p in parts for t in p])
        return out

    @staticmethod
    def backward(ctx, g):
        saved = ctx.saved_tensors
        g = g.contiguous()
        grads = [None] * 6
        for i in range(ctx.parts):
            key, enc, W = saved[3 * i:3 * i + 3]
            if not ctx.needs_input_grad[3 * i + 2]:
                continue
            grads[3 * i + 2] = si_embed_wgrad(key, enc, g)
        return tuple(grads)


def si_embed(key1, enc1, W1, key2=None, enc2=None, W2=None):
    return _SiEmbedFn.apply(key1, enc1, W1, key2, enc2, W2)


def si_embed_wgrad(key, enc, g):
    """dW [K, H] = enc[key]^T @ g, deterministic (dn_si_embed_wgrad_*)."""
    require_gpu(key, enc, g)
    N, H, K = g.shape[0], g.shape[1], enc.shape[1]
    dW = torch.empty((K, H), dtype=g.dtype, device=g.device)
    ws = _ws(lib().dn_si_embed_wgrad_workspace_bytes(N, K, H), g.device)
    fn = getattr(lib(), "dn_si_embed_wgrad_" + _suffix(g))
    launch_tagged("si_embed_wgrad", lambda: check(fn(N, H, ptr(_i32(key, "key")), ptr(enc.contiguous()), int(enc.shape[0]), K, ptr(g), ptr(dW),
                                              ptr(ws), ws.numel(), stream_ptr()), "dn_si_embed_wgrad"))
    return dW


class _SiPoolSumFn(torch.autograd.Function):
    """pooled [B, D] fp32 = per-graph sum of the non-dummy virtual rows [enc_v(id) | enc_vl(label) | out_deg | in_deg | rep]
    (dn_si_pool_sum_*); the gradient reaches rep only (encoders frozen, degrees integer)."""

    @staticmethod
    def forward(ctx, rep, node_ptr, dummy, id_, enc_v, label, enc_vl, out_deg, in_deg):
        rep = rep.contiguous()
        require_gpu(rep, node_ptr, dummy, id_, enc_v, label, enc_vl, out_deg, in_deg)
        B, H = node_ptr.numel() - 1, rep.shape[1]
        Kv = int(enc_v.shape[1]) if id_ is not None else 0
        Kvl = int(enc_vl.shape[1]) if label is not None else 0
        D = Kv + Kvl + (2 if out_deg is not None else 0) + H
        for t in (enc_v if id_ is not None else None, enc_vl if label is not None else None):
            if t is not None and t.dtype != rep.dtype:
                raise _lib.DnHipError("si_pool_sum: encoder tables must have the dtype of rep")
        pooled = torch.empty((B, D), dtype=torch.float32, device=rep.device)
        count = torch.empty(B, dtype=I32, device=rep.device)
        fn = getattr(lib(), "dn_si_pool_sum_" + _suffix(rep))
        launch_tagged("si_pool_sum", lambda: check(fn(B, ptr(_i32(node_ptr, "node_ptr")), ptr(dummy), ptr(id_), ptr(enc_v), int(enc_v.shape[0]) if id_ is not None else 0,
                                               Kv, ptr(label), ptr(enc_vl), int(enc_vl.shape[0]) if label is not None else 0, Kvl,
                                               ptr(out_deg), ptr(in_deg), ptr(rep), H, ptr(pooled), ptr(count), stream_ptr()),
                                            "dn_si_pool_sum"))
        ctx.save_for_backward(node_ptr, dummy if dummy is not None else node_ptr.new_empty(0))
        ctx.has_dummy, ctx.shape, ctx.dtype, ctx.col0 = dummy is not None, rep.shape, rep.dtype, D - H
        ctx.mark_non_differentiable(count)
        return pooled, count

    @staticmethod
    def backward(ctx, dpooled, _dc):
        node_ptr, dummy = ctx.saved_tensors
        if dpooled is None:
            return (None,) * 9
        dpooled = dpooled.contiguous().float()
        B = node_ptr.numel() - 1
        drep = torch.empty(ctx.shape, dtype=ctx.dtype, device=dpooled.device)
        fn = getattr(lib(), "dn_si_pool_sum_bwd_" + _suffix(drep))
        launch_tagged("si_pool_sum_bwd", lambda: check(fn(B, ptr(node_ptr), ptr(dummy) if ctx.has_dummy else None, ptr(dpooled),
                                                   int(dpooled.shape[1]), ctx.col0, int(ctx.shape[1]), ptr(drep), stream_ptr()),
                                                "dn_si_pool_sum_bwd"))
        return (drep,) + (None,) * 8


def si_pool_sum(rep, node_ptr, dummy=None, id_=None, enc_v=None, label=None, enc_vl=None, out_deg=None, in_deg=None):
    return _SiPoolSumFn.apply(rep, node_ptr, _u8_or_none(dummy), id_, enc_v, label, enc_vl, out_deg, in_deg)


class _SiPoolMaxFn(torch.autograd.Function):
    """out [B, C] = per-graph max of Y [N, C] over the non-dummy rows, bias as a candidate when the graph has fewer than L of them
    (dn_si_pool_max_*); the gradient goes to the argmax row, or to the bias where it won."""

    @staticmethod
    def forward(ctx, Y, bias, node_ptr, dummy, L):
        Y, bias = Y.contiguous(), bias.contiguous()
        require_gpu(Y, bias, node_ptr, dummy)
        if bias.dtype != Y.dtype or bias.numel() != Y.shape[1]:
            raise _lib.DnHipError("si_pool_max: bias [C] of the dtype of Y expected")
        B, C = node_ptr.numel() - 1, Y.shape[1]
        out = torch.empty((B, C), dtype=Y.dtype, device=Y.device)
        arg = torch.empty((B, C), dtype=I32, device=Y.device)
        fn = getattr(lib(), "dn_si_pool_max_" + _suffix(Y))
        launch_tagged("si_pool_max", lambda: check(fn(B, ptr(_i32(node_ptr, "node_ptr")), ptr(dummy), ptr(Y), C, ptr(bias), int(L), ptr(out),
                                               ptr(arg), stream_ptr()), "dn_si_pool_max"))
        ctx.save_for_backward(arg)
        ctx.shape = Y.shape
        return out

    @staticmethod
    def backward(ctx, dout):
        (arg,) = ctx.saved_tensors
        dout = dout.contiguous()
        B, C = arg.shape
        dY = torch.zeros(ctx.shape, dtype=dout.dtype, device=dout.device)
        fn = getattr(lib(), "dn_si_pool_max_bwd_" + _suffix(dout))
        launch_tagged("si_pool_max_bwd", lambda: check(fn(B, C, ptr(arg), ptr(dout), ptr(dY), stream_ptr()), "dn_si_pool_max_bwd"))
        dbias = (dout.float() * (arg < 0)).sum(0).to(dout.dtype)
        return dY, dbias, None, None, None


def si_pool_max(Y, bias, node_ptr, L, dummy=None):
    return _SiPoolMaxFn.apply(Y, bias, node_ptr, _u8_or_none(dummy), L)


def si_len_mask(node_ptr, L, dummy=None):
    """[B, L] bool: batch_convert_len_to_mask(pre_pad=True) with the dummy positions cleared (dn_si_len_mask_u8)."""
    dummy = _u8_or_none(dummy)
    require_gpu(node_ptr, dummy)
    B = node_ptr.numel() - 1
    mask = torch.empty((B, int(L)), dtype=torch.bool, device=node_ptr.device)
    launch_tagged("si_len_mask", lambda: check(lib().dn_si_len_mask_u8(B, int(L), ptr(_i32(node_ptr, "node_ptr")), ptr(dummy),
                                                                ptr(mask.view(torch.uint8)), stream_ptr()), "dn_si_len_mask"))
    return mask


def si_read_meta_pair(meta_v, meta_e, need_edges=True):
    """si_read_meta for a model with node AND edge sides: both metas in ONE device-to-host read.  Returns ((Lp, Lg), (Lpe, Lge)).
    The edge meta comes from dn_si_filter_meta run on edge_ptr / edge labels (its "id" slot re-checks the label); a graph without
    edges only raises when need_edges (the edge head would divide by its zero length)."""
    lp, lg, flags, _, lpe, lge, eflags, _ = torch.cat([meta_v, meta_e]).tolist()
    if flags:
        what = "; ".join(m for bit, m in SI_FLAGS if flags & bit)
        if flags & (4 | 8):
            raise ValueError("SI model batch: %s" % what)
        raise _lib.DnHipError("SI model batch: %s" % what)
    if eflags & (1 | 2):
        raise _lib.DnHipError("SI model batch: an edge label outside the edge label table")
    if eflags & 16:
        raise _lib.DnHipError("SI model batch: inconsistent edge_ptr")
    if eflags & (4 | 8) and need_edges:
        raise ValueError("SI model batch: a %s with no edges" % ("pattern" if eflags & 4 else "graph"))
    return (int(lp), int(lg)), (max(int(lpe), 1), max(int(lge), 1))


# ----------------------------------------------------------------------------------------------
# dual (node + edge) message passing of CompGCN / DMPNN and the ragged edge head (dn_dual.hip)
# ----------------------------------------------------------------------------------------------
DUAL_EDGE, DUAL_SUB, DUAL_MULT = 0, 1, 2
DUAL_MAX_H = 256


# The layers' default.  Measured on the scale batch (docs/LAB_NOTES.md "SI count models: CompGCN / DMPNN"): the fused DMPLayer and
# CompGCNLayer (sub, mult) steps are 7-14 % faster in median than the composed ones, but inside the run-to-run spread of the box, so
# the composed path stays the default and the fused kernels are an opt-in (`with ops.dual_fused():`).
DUAL_FUSED_DEFAULT = False


def dual_fused_enabled():
    """Do CompGCNLayer / DMPLayer forwards started NOW on this thread take dn_dual.hip?  The thread's dual_fused / dual_composed
    override, else ops.DUAL_FUSED_DEFAULT."""
    return dual_fused.override(DUAL_FUSED_DEFAULT)


class dual_fused(_ThreadSwitch):
    """Context manager: CompGCNLayer (sub, mult) / DMPLayer forwards started inside it (on this thread) run on the fused dual
    kernels (dn_dual.hip) where the predicate of dual.py allows it.  Their backward passes use the same kernels whenever they run."""
    _slot = "dual_fused"


class dual_composed(dual_fused):
    """Context manager: force the composed path (generic segment kernels + torch glue) for the layers inside it, whatever the
    default -- for tests and A/B runs.  dual_composed(False) = dual_fused()."""
    _inverse = True


def dual_supported(*tensors):
    """The predicate of the fused dual path: fp32 / bf16 rows of one dtype and width H <= 256, contiguous, on the GPU."""
    t0 = tensors[0]
    return all(t.is_cuda and t.dim() == 2 and t.dtype == t0.dtype and t.dtype in MFMA_DTYPES and t.is_contiguous()
               and t.shape[1] == t0.shape[1] for t in tensors) and 1 <= t0.shape[1] <= DUAL_MAX_H


class _DualUnits:
    """Unit table of dn_dual_agg_* over one grouped list of an EdgeIndex ("in": CSR by destination, "out": CSC by source): one
    unit per segment of at most HUB_SPLIT entries, HUB_SPLIT-entry chunks (with a partial slot each) for the longer ones."""

    def __init__(self, ptr_, num_segments):
        N, dev = int(num_segments), ptr_.device
        lo, hi = ptr_[:-1].long(), ptr_[1:].long()
        nchunk = ((hi - lo + HUB_SPLIT - 1) // HUB_SPLIT).clamp(min=1)
        first = torch.cat([nchunk.new_zeros(1), torch.cumsum(nchunk, 0)])
        U = int(first[-1]) if N else 0
        self.num_units, self.num_slots, self.hub_ids, self.fold_ptr = U, 0, None, None
        if U == N:
            seg = torch.arange(N, device=dev)
            self.units = torch.stack([seg, lo, hi, torch.full_like(seg, -1)], 1).to(I32).contiguous()
            return
        seg = torch.repeat_interleave(torch.arange(N, device=dev), nchunk, output_size=U)
        beg = lo[seg] + (torch.arange(U, device=dev) - first[:-1][seg]) * HUB_SPLIT
        end = torch.minimum(beg + HUB_SPLIT, hi[seg])
        hub = (nchunk > 1)[seg]
        slot = torch.where(hub, torch.cumsum(hub.long(), 0) - 1, torch.full_like(seg, -1))
        self.units = torch.stack([seg, beg, end, slot], 1).to(I32).contiguous()
        self.hub_ids = torch.nonzero(nchunk > 1).reshape(-1)
        hub_chunks = nchunk[self.hub_ids]
        self.fold_ptr = torch.cat([hub_chunks.new_zeros(1), torch.cumsum(hub_chunks, 0)]).to(I32)
        self.num_slots = int(self.fold_ptr[-1])

    def part(self, width, device):
        return torch.empty((self.num_slots, width), dtype=torch.float32, device=device) if self.num_slots else None

    def fold(self, out, part):
        """out [R, N, H] <- the chunk partials of every long segment summed in chunk order (part [P, R * H] fp32)."""
        if part is None:
            return
        R, _, H = out.shape
        hub = gather_segsum(part, None, self.fold_ptr)
        out.index_copy_(1, self.hub_ids, hub.view(-1, R, H).transpose(0, 1).to(out.dtype))


def dual_units(index, side):
    tabs = getattr(index, "_dual_units", None)
    if tabs is None:
        tabs = index._dual_units = {}
    if side not in tabs:
        tabs[side] = _DualUnits(index.in_ptr if side == "in" else index.out_ptr, index.num_nodes)
    return tabs[side]


def _rev_u8(rev):
    if rev is None:
        return None
    rev = rev.reshape(-1)
    if rev.dtype == torch.bool:
        return rev.contiguous().view(torch.uint8)
    if rev.dtype != torch.uint8:
        raise _lib.DnHipError("reversed-edge flags must be bool or uint8 on the device (got %s)" % rev.dtype)
    return rev.contiguous()


def dual_agg_raw(mode, ef, x, index, side, rev, scale, out_f32=False):
    """out [2, N, H] of dn_dual_agg_* over the CSR by destination (side "in": perm = in_perm) or the CSC by source ("out");
    out_f32: the fp32 sums instead of rows in the dtype of ef."""
    require_gpu(ef, x, rev, scale)
    N, E, H = index.num_nodes, index.num_edges, int(ef.shape[1])
    if ef.shape[0] != E or (x is not None and (x.shape != (N, H) or x.dtype != ef.dtype)) or H > DUAL_MAX_H:
        raise _lib.DnHipError("dual_agg: ef [E, H], x [N, H] of one dtype and H <= %d expected" % DUAL_MAX_H)
    if (rev is not None and rev.numel() != E) or (scale is not None and (scale.numel() != E or scale.dtype != torch.float32)):
        raise _lib.DnHipError("dual_agg: rev uint8 [E] and scale fp32 [E] expected")
    tab = dual_units(index, side)
    perm = index.in_perm if side == "in" else index.out_perm
    out = torch.empty((2, N, H), dtype=torch.float32 if out_f32 else ef.dtype, device=ef.device)
    part = tab.part(2 * H, ef.device)
    fn = getattr(lib(), "dn_dual_agg_" + _suffix(ef))
    launch_tagged("dual_agg", lambda: check(fn(int(mode), N, E, H, tab.num_units, ptr(tab.units), ptr(perm), ptr(index.src), ptr(rev),
                                               ptr(scale), ptr(ef), ptr(x), ptr(out), 1 if out_f32 else 0, ptr(part), tab.num_slots, stream_ptr()),
                                            "dn_dual_agg"))
    tab.fold(out, part)
    return out


class _DualAggFn(torch.autograd.Function):
    """(out_fwd, out_rev) [N, H] each = sums over the in-edges of v, by direction, of scale_e * m_e (dn_dual_agg_*);
    backward: d ef on dn_dual_agg_bwd_edge_*, d x (sub / mult) on dn_dual_agg_bwd_node_* over the CSC.  No gradient to scale."""

    @staticmethod
    def forward(ctx, ef, x, index, rev, scale, mode):
        ef = ef.contiguous()
        x = None if mode == DUAL_EDGE else x.contiguous()
        out = dual_agg_raw(mode, ef, x, index, "in", rev, scale)
        ctx.index, ctx.mode, ctx.rev, ctx.scale = index, int(mode), rev, scale
        ctx.save_for_backward(ef if mode == DUAL_MULT else ef.new_empty(0), x if mode == DUAL_MULT else ef.new_empty(0))
        ctx.shape = (tuple(ef.shape), None if x is None else tuple(x.shape))
        return out[0], out[1]

    @staticmethod
    def backward(ctx, g0, g1):
        ef, x = ctx.saved_tensors
        ix, mode, rev, scale = ctx.index, ctx.mode, ctx.rev, ctx.scale
        N, E = ix.num_nodes, ix.num_edges
        H = ctx.shape[0][1]
        ref = g0 if g0 is not None else g1
        g = torch.stack([t if t is not None else torch.zeros_like(ref) for t in (g0, g1)], 0).contiguous()
        sfx = _suffix(g)
        d_ef = d_x = None
        if ctx.needs_input_grad[0]:
            d_ef = torch.empty(ctx.shape[0], dtype=g.dtype, device=g.device)
            fn = getattr(lib(), "dn_dual_agg_bwd_edge_" + sfx)
            launch_tagged("dual_agg_bwd_edge", lambda: check(fn(mode, N, E, H, ptr(ix.src), ptr(ix.dst), ptr(rev), ptr(scale), ptr(g),
                                                                ptr(x) if mode == DUAL_MULT else None, ptr(d_ef), stream_ptr()),
                                                             "dn_dual_agg_bwd_edge"))
        if mode != DUAL_EDGE and ctx.needs_input_grad[1]:
            tab = dual_units(ix, "out")
            dx = torch.empty((1, N, H), dtype=g.dtype, device=g.device)
            part = tab.part(H, g.device)
            fn = getattr(lib(), "dn_dual_agg_bwd_node_" + sfx)
            launch_tagged("dual_agg_bwd_node", lambda: check(fn(mode, N, E, H, tab.num_units, ptr(tab.units), ptr(ix.out_perm), ptr(ix.dst),
                                                                ptr(rev), ptr(scale), ptr(g), ptr(ef) if mode == DUAL_MULT else None,
                                                                ptr(dx), ptr(part), tab.num_slots, stream_ptr()),
                                                             "dn_dual_agg_bwd_node"))
            tab.fold(dx, part)
            d_x = dx[0]
        return d_ef, d_x, None, None, None, None


def dual_agg(ef, x, index, rev=None, scale=None, mode=DUAL_EDGE):
    """(sum over the forward in-edges, sum over the reversed in-edges) of scale_e * m_e per destination node, one pass.
    mode DUAL_EDGE: m_e = ef_e (x ignored); DUAL_SUB: x[src_e] - ef_e; DUAL_MULT: x[src_e] * ef_e.  rev: bool / uint8 [E] or
    None (every edge is a forward edge); scale: fp32 [E] in edge order or None."""
    return _DualAggFn.apply(ef, x, index, _rev_u8(rev), scale, mode)


def dmp_coef(index):
    """2 (1 + log2(1 + out_deg[v])) as fp32 [N] (dmpnn.py:150-157), kept on the index."""
    c = getattr(index, "_dmp_coef", None)
    if c is None:
        out_deg = (index.out_ptr[1:] - index.out_ptr[:-1]).float()
        c = index._dmp_coef = (2.0 * (1.0 + torch.log2(1.0 + out_deg))).contiguous()
    return c


class _DmpEdgeUpdateFn(torch.autograd.Function):
    """out[e] = (p_loop[e] + coef[dst_e] p_diff[e]) + (xd[a_e] - xs[b_e]) + ebias  (dn_dual_edge_update_*).  Backward: d p_loop = g,
    d p_diff = coef[dst] g (dn_dual_edge_update_bwd_*), d xd / d xs = row sums of g from the index's CSR and CSC with the direction
    flag (two dn_dual_agg_* passes, in-list first, then out-list), d ebias = the column sum."""

    @staticmethod
    def forward(ctx, p_loop, p_diff, xd, xs, ebias, index, rev):
        p_loop, p_diff, xd, xs = (t.contiguous() for t in (p_loop, p_diff, xd, xs))
        require_gpu(p_loop, p_diff, xd, xs, ebias, rev)
        N, E, H = index.num_nodes, index.num_edges, int(p_loop.shape[1])
        if p_loop.shape != (E, H) or p_diff.shape != (E, H) or xd.shape != (N, H) or xs.shape != (N, H) or H > DUAL_MAX_H:
            raise _lib.DnHipError("dmp_edge_update: p_loop / p_diff [E, H], xd / xs [N, H], H <= %d expected" % DUAL_MAX_H)
        coef = dmp_coef(index)
        out = torch.empty_like(p_loop)
        fn = getattr(lib(), "dn_dual_edge_update_" + _suffix(p_loop))
        launch_tagged("dual_edge_update", lambda: check(fn(N, E, H, ptr(index.src), ptr(index.dst), ptr(rev), ptr(coef), ptr(p_loop),
                                                           ptr(p_diff), ptr(xd), ptr(xs), ptr(ebias), ptr(out), stream_ptr()),
                                                        "dn_dual_edge_update"))
        ctx.index, ctx.rev, ctx.has_bias = index, rev, ebias is not None
        return out

    @staticmethod
    def backward(ctx, g):
        g = g.contiguous()
        ix, rev = ctx.index, ctx.rev
        N, E, H = ix.num_nodes, ix.num_edges, int(g.shape[1])
        d_loop = g if ctx.needs_input_grad[0] else None
        d_diff = d_xd = d_xs = d_bias = None
        if ctx.needs_input_grad[1]:
            d_diff = torch.empty_like(g)
            fn = getattr(lib(), "dn_dual_edge_update_bwd_" + _suffix(g))
            launch_tagged("dual_edge_update_bwd", lambda: check(fn(N, E, H, ptr(ix.dst), ptr(dmp_coef(ix)), ptr(g), ptr(d_diff),
                                                                   stream_ptr()), "dn_dual_edge_update_bwd"))
        if ctx.needs_input_grad[2] or ctx.needs_input_grad[3]:
            by_dst = dual_agg_raw(DUAL_EDGE, g, None, ix, "in", rev, None, out_f32=True)     # [fwd | rev] sums over the in-lists
            by_src = dual_agg_raw(DUAL_EDGE, g, None, ix, "out", rev, None, out_f32=True)    # ... over the out-lists
            # (fp32 sums, rounded ONCE after the two lists are added)
            d_xd = (by_dst[0] + by_src[1]).to(g.dtype)                            # a_e = dst (forward) | src (reversed)
            d_xs = (-(by_dst[1] + by_src[0])).to(g.dtype)                         # b_e = src (forward) | dst (reversed)
        if ctx.has_bias and ctx.needs_input_grad[4]:
            d_bias = g.float().sum(0).to(g.dtype)
        return d_loop, d_diff, d_xd, d_xs, d_bias, None, None


def dmp_edge_update(p_loop, p_diff, xd, xs, ebias, index, rev=None):
    return _DmpEdgeUpdateFn.apply(p_loop, p_diff, xd, xs, ebias, index, _rev_u8(rev))


class _SiePoolSumFn(torch.autograd.Function):
    """pooled [B, D] fp32 = per-graph sum of the kept edge head rows (dn_sie_pool_sum_*); the gradient reaches rep only
    (dn_si_pool_sum_bwd_* on edge_ptr / skip)."""

    @staticmethod
    def forward(ctx, rep, edge_ptr, skip, src, dst, id_, enc_v, vlabel, enc_vl, elabel, enc_el, out_deg, in_deg):
        rep = rep.contiguous()
        require_gpu(rep, edge_ptr, skip, src, dst, id_, enc_v, vlabel, enc_vl, elabel, enc_el, out_deg, in_deg)
        for t, n in ((edge_ptr, "edge_ptr"), (src, "src"), (dst, "dst"), (id_, "id"), (vlabel, "vlabel"), (elabel, "elabel"),
                     (out_deg, "out_deg"), (in_deg, "in_deg")):
            _i32(t, n)
        B, H = edge_ptr.numel() - 1, rep.shape[1]
        has_enc = id_ is not None
        if has_enc and (vlabel is None or elabel is None or any(t.dtype != rep.dtype for t in (enc_v, enc_vl, enc_el))):
            raise _lib.DnHipError("sie_pool_sum: all three encoder tables, of the dtype of rep, or none")
        if (has_enc or out_deg is not None) and (src is None or dst is None):
            raise _lib.DnHipError("sie_pool_sum: the encoder / degree columns need src and dst")
        if any(t is not None and t.numel() != rep.shape[0] for t in (src, dst, skip, elabel)):
            raise _lib.DnHipError("sie_pool_sum: one rep row, flag and label per edge expected")
        N = int(id_.numel()) if has_enc else (int(out_deg.numel()) if out_deg is not None else 0)
        if has_enc and out_deg is not None and out_deg.numel() != N:
            raise _lib.DnHipError("sie_pool_sum: id and degrees must cover the same nodes")
        Kv, Kvl, Kel = (int(enc_v.shape[1]), int(enc_vl.shape[1]), int(enc_el.shape[1])) if has_enc else (0, 0, 0)
        rows = (int(enc_v.shape[0]), int(enc_vl.shape[0]), int(enc_el.shape[0])) if has_enc else (0, 0, 0)
        D = 2 * Kv + 2 * Kvl + Kel + (2 if out_deg is not None else 0) + H
        pooled = torch.empty((B, D), dtype=torch.float32, device=rep.device)
        count = torch.empty(B, dtype=I32, device=rep.device)
        fn = getattr(lib(), "dn_sie_pool_sum_" + _suffix(rep))
        launch_tagged("sie_pool_sum", lambda: check(fn(B, ptr(edge_ptr), ptr(skip), ptr(src), ptr(dst), N, ptr(id_), ptr(enc_v), rows[0], Kv,
                                                       ptr(vlabel), ptr(enc_vl), rows[1], Kvl, ptr(elabel), ptr(enc_el), rows[2], Kel,
                                                       ptr(out_deg), ptr(in_deg), ptr(rep), H, ptr(pooled), ptr(count), stream_ptr()),
                                                    "dn_sie_pool_sum"))
        ctx.save_for_backward(edge_ptr, skip if skip is not None else edge_ptr.new_empty(0))
        ctx.has_skip, ctx.shape, ctx.dtype, ctx.col0 = skip is not None, rep.shape, rep.dtype, D - H
        ctx.mark_non_differentiable(count)
        return pooled, count

    @staticmethod
    def backward(ctx, dpooled, _dc):
        edge_ptr, skip = ctx.saved_tensors
        if dpooled is None:
            return (None,) * 13
        dpooled = dpooled.contiguous().float()
        B = edge_ptr.numel() - 1
        drep = torch.empty(ctx.shape, dtype=ctx.dtype, device=dpooled.device)
        fn = getattr(lib(), "dn_si_pool_sum_bwd_" + _suffix(drep))
        launch_tagged("sie_pool_sum_bwd", lambda: check(fn(B, ptr(edge_ptr), ptr(skip) if ctx.has_skip else None, ptr(dpooled),
                                                           int(dpooled.shape[1]), ctx.col0, int(ctx.shape[1]), ptr(drep), stream_ptr()),
                                                        "dn_si_pool_sum_bwd"))
        return (drep,) + (None,) * 12


def sie_pool_sum(rep, edge_ptr, skip=None, src=None, dst=None, id_=None, enc_v=None, vlabel=None, enc_vl=None, elabel=None,
                 enc_el=None, out_deg=None, in_deg=None):
    """(pooled [B, D] fp32, count [B]) over the edges with skip == 0 of every graph; see dn_sie_pool_sum_* (include/dn_hip.h)."""
    return _SiePoolSumFn.apply(rep, edge_ptr, _u8_or_none(skip), src, dst, id_, enc_v.contiguous() if enc_v is not None else None,
                               vlabel, enc_vl.contiguous() if enc_vl is not None else None, elabel,
                               enc_el.contiguous() if enc_el is not None else None, out_deg, in_deg)


# ----------------------------------------------------------------------------------------------
# LRP (local relational pooling) of the SI count model LRP: ego-net index and pooling (dn_lrp.hip)
# ----------------------------------------------------------------------------------------------
LRP_SEQ_LENS = (2, 3, 4)
LRP_MAX_H = 256
LRP_LEAKY_SLOPE = 1.0 / 5.5              # the reference's leaky_relu (subgraph_isomorphism/utils/act.py)
# LDS budget of dn_lrp_pool_*: an ego of d + 1 nodes keeps its T_node rows in LDS while (d + 1) * L * H * 4 <= LRP_STAGE_BYTES and
# its pair -> edge table while d + 1 <= LRP_PAIR_NODES (checked against the library when the first index is built)
LRP_STAGE_BYTES = 56 * 1024
LRP_PAIR_NODES = 64
# The default path of ops.lrp_pool.  Measured on the config-3 scale batch (docs/LAB_NOTES.md "LRP"): with one workgroup per node the
# fused kernels lose to the composed path when every ego is small (LRPLayer step 4.5 ms against 2.9 ms at L = 4), so the composed
# path is the default and the fused kernels are an opt-in (`with ops.lrp_fused():`) -- and the path of a batch whose sequence
# list does not fit the materialised index (hub egos), where the composed path cannot run at all.
LRP_FUSED_DEFAULT = False
_INT32_MAX = 2 ** 31 - 1


def lrp_stage_nodes(H, seq_len):
    """Largest ego (the node and its neighbours) whose table rows dn_lrp_pool_* stages in LDS at width H."""
    return LRP_STAGE_BYTES // (int(seq_len) * int(H) * 4)


def lrp_fused_enabled():
    return lrp_fused.override(LRP_FUSED_DEFAULT)


class lrp_fused(_ThreadSwitch):
    """Context manager: ops.lrp_pool calls started inside it (on this thread) run on dn_lrp_pool_* where the width allows it."""
    _slot = "lrp_fused"


class lrp_composed(lrp_fused):
    """Context manager: force the composed path (gather_segsum over the materialised index + dn_segment_mean / _sum), whatever
    the default -- the A/B partner of the fused kernels and the path of widths they do not take."""
    _inverse = True


# The default path of ops.lrp_pool_linear (the pooling of a DMPLRP layer): the collapsed index (LrpIndex.collapsed) or
# lrp_pool(act="none", factor=None).  Measured in docs/LAB_NOTES.md "DMPLRP" (L = 4, H = 64): level with the composed path on the
# config-3 scale batch (op 2.32 against 2.41 ms, the layer step inside the spread), 2.3 against 15.9 ms per layer step on 64-node
# graphs with a forward-connected dummy node -- so the collapsed path is the default.
LRP_COLLAPSED_DEFAULT = True


def lrp_collapsed_enabled():
    return lrp_collapsed.override(LRP_COLLAPSED_DEFAULT)


class lrp_collapsed(_ThreadSwitch):
    """Context manager: ops.lrp_pool_linear calls started inside it (on this thread) pool over the collapsed index (on=True) or
    through ops.lrp_pool(act="none", factor=None) (on=False: the composed or fused path, as ops.lrp_fused / lrp_composed say)."""
    _slot = "lrp_collapsed"


def lrp_fused_supported(H):
    return 16 <= int(H) <= LRP_MAX_H and int(H) % 16 == 0


class LrpPermIndex(NamedTuple):
    perm_ptr: torch.Tensor       # [N + 1] int32
    perm_nodes: torch.Tensor     # [P, L] int32, -1 = empty
    perm_edges: torch.Tensor     # [P, L * L] int32, -1 = empty


class LrpCollapsed(NamedTuple):
    col_ptr: torch.Tensor        # [N + 1] int32
    col_rows: torch.Tensor       # [Q] int32: per node the distinct table rows of its sequences, ascending
    col_cnt: torch.Tensor        # [Q] int64: the occurrences of the row in the node's sequences
    col_node: torch.Tensor       # [Q] int32: the node of every entry
    tptr: torch.Tensor           # [rows + 1] int32: the same entries grouped by table row (the backward's lists) ...
    tperm: torch.Tensor          # [Q] int32: ... as positions into col_rows / col_cnt / col_node


class LrpIndex:
    """Ego-net index of a batch for sequence length L (dn_lrp.hip): the sorted duplicate-free out-neighbour lists over the edges
    with is_reversed == 0 (uptr / unbr, with ueid = the last edge id of every pair), per node its kind, its dummy neighbours, the
    neighbour positions split into non-dummy / dummy (upos) and its sequence count (int64).  Nothing here is sized by the number
    of sequences; the one device-to-host read is the error word (a self-loop among the counted edges raises DnHipError)."""

    def __init__(self, src, dst, num_nodes, seq_len, rev=None, dummy=None, node_ptr=None):
        if int(seq_len) not in LRP_SEQ_LENS:
            raise ValueError("lrp_seq_len must be one of %s (got %s)" % (LRP_SEQ_LENS, seq_len))
        require_gpu(src, dst, rev, dummy)
        if lib().dn_lrp_stage_bytes() != LRP_STAGE_BYTES or lib().dn_lrp_pair_nodes() != LRP_PAIR_NODES:
            raise _lib.DnHipError("ops.LRP_STAGE_BYTES / LRP_PAIR_NODES differ from the library's")
        N, E, dev = int(num_nodes), int(src.numel()), src.device
        self.num_nodes, self.num_edges, self.seq_len = N, E, int(seq_len)
        big = N * N
        key = src.long() * N + dst.long()
        if rev is not None:
            key = torch.where(rev.reshape(-1).bool(), torch.full_like(key, big), key)
        ks, order = torch.sort(key, stable=True)
        # the last entry of every run of equal keys: the pair's largest edge id (stable sort); everything else lands in slot E
        last = (ks < big) & (ks != torch.cat([ks[1:], ks.new_full((1,), -1)]))
        tgt = torch.where(last, torch.cumsum(last, 0) - 1, torch.full_like(ks, E))
        self.unbr = torch.zeros(E + 1, dtype=I32, device=dev).scatter_(0, tgt, (ks % N).to(I32))
        self.ueid = torch.zeros(E + 1, dtype=I32, device=dev).scatter_(0, tgt, order.to(I32))
        deg = torch.zeros(N + 1, dtype=torch.long, device=dev).scatter_add_(
            0, torch.where(last, ks // max(N, 1), torch.full_like(ks, N)), torch.ones_like(ks))
        self.uptr = torch.cat([deg.new_zeros(1), torch.cumsum(deg[:N], 0)]).to(I32)
        self.upos = torch.zeros(E + 1, dtype=I32, device=dev)
        self.ego = torch.zeros((N, 2), dtype=I32, device=dev)
        self.count = torch.ones(N, dtype=torch.long, device=dev)
        self.dummy = _u8_or_none(dummy)
        err = torch.tensor([_INT32_MAX, 0], dtype=I32, device=dev)
        check(lib().dn_lrp_ego_index_i32(N, self.seq_len, ptr(self.uptr), ptr(self.unbr), ptr(self.dummy), ptr(self.upos),
                                         ptr(self.ego), ptr(self.count), ptr(err), stream_ptr()), "dn_lrp_ego_index_i32")
        loop, flags = err.tolist()
        if loop != _INT32_MAX:
            where = ""
            if node_ptr is not None:
                g = int(torch.searchsorted(node_ptr.long(), torch.tensor([loop], device=node_ptr.device), right=True)) - 1
                where = " (node %d of graph %d)" % (loop - int(node_ptr[g]), g)
            raise _lib.DnHipError("LRP index: a self-loop on batch node %d%s; the ego-net sequences are undefined for it" % (loop, where))
        if flags & 1:
            raise _lib.DnHipError("LRP index: a node's sequence count does not fit 64 bits")
        self._perm = None
        self._composed = None
        self._total = None
        self._collapsed = None
        self._collapsed_scale = {}

    def _args(self):
        return (ptr(self.uptr), ptr(self.unbr), ptr(self.ueid), ptr(self.upos), ptr(self.ego), ptr(self.count))

    def num_sequences(self):
        """P, the batch's sequence total (one device-to-host read, kept)."""
        if self._total is None:
            self._total = int(self.count.sum())
        return self._total

    def materialisable(self):
        return self.num_sequences() * self.seq_len * self.seq_len <= _INT32_MAX

    def perm_index(self):
        """The materialised index (LrpPermIndex), built by count -> scan -> fill and kept; reads the sequence total back once."""
        if self._perm is None:
            N, L = self.num_nodes, self.seq_len
            P = self.num_sequences()
            ptr64 = torch.cat([self.count.new_zeros(1), torch.cumsum(self.count, 0)])
            if not self.materialisable():
                raise _lib.DnHipError("LRP index: %d sequences do not fit an int32 index; use the fused path" % P)
            perm_ptr = ptr64.to(I32)
            nodes = torch.empty((P, L), dtype=I32, device=perm_ptr.device)
            edges = torch.empty((P, L * L), dtype=I32, device=perm_ptr.device)
            check(lib().dn_lrp_perm_fill_i32(N, L, *self._args(), ptr(perm_ptr), P, ptr(nodes), ptr(edges), stream_ptr()),
                  "dn_lrp_perm_fill_i32")
            self._perm = LrpPermIndex(perm_ptr, nodes, edges)
        return self._perm

    def composed_tables(self):
        """(idx, ptr, csr of idx, segment of every entry) of the composed path over the stacked table [N L + E L (L - 1), H]:
        sequence p gathers row node * L + k for its k-th node and row N L + eid * L (L - 1) + slot for every edge it holds."""
        if self._composed is None:
            pi = self.perm_index()
            N, E, L = self.num_nodes, self.num_edges, self.seq_len
            P, dev = pi.perm_nodes.shape[0], pi.perm_nodes.device
            k = torch.arange(L, device=dev)
            slot = torch.arange(L * L, device=dev)
            a, b = slot // L, slot % L
            off = a * (L - 1) + torch.where(b > a, b - 1, b)
            rows = torch.full((P, L + L * L), -1, dtype=torch.long, device=dev)
            rows[:, :L] = torch.where(pi.perm_nodes >= 0, pi.perm_nodes.long() * L + k, rows[:, :L])
            rows[:, L:] = torch.where(pi.perm_edges >= 0, N * L + pi.perm_edges.long() * (L * (L - 1)) + off, rows[:, L:])
            keep = rows >= 0
            idx = rows[keep].to(I32).contiguous()
            ptr_ = torch.cat([keep.new_zeros(1, dtype=torch.long), torch.cumsum(keep.sum(1), 0)]).to(I32)
            seg = torch.repeat_interleave(torch.arange(P, device=dev, dtype=I32), keep.sum(1), output_size=idx.numel())
            tptr, tperm = csr_build(idx, N * L + E * L * (L - 1))
            self._composed = (idx, ptr_, tptr, seg.index_select(0, tperm.long()).contiguous())
        return self._composed


    def table_rows(self):
        """Rows of the stacked table [T_node; T_edge] of composed_tables / collapsed."""
        return self.num_nodes * self.seq_len + self.num_edges * self.seq_len * (self.seq_len - 1)

    def collapsed(self):
        """The collapsed index (LrpCollapsed) of dmplrp.py:180-185, kept: per node the distinct rows of the stacked table that its
        sequences touch (numbered as composed_tables numbers them) with their occurrence counts, from the closed forms of
        dn_lrp_collapse_*_i32 by count -> scan -> fill, then one device sort that makes the rows of a node ascend.  Nothing is sized
        by the sequence count; reads the entry total Q back once."""
        if self._collapsed is None:
            N, E, L, dev = self.num_nodes, self.num_edges, self.seq_len, self.uptr.device
            R = self.table_rows()
            if R > _INT32_MAX:
                raise _lib.DnHipError("LRP index: %d table rows do not fit an int32 index" % R)
            per_node = torch.zeros(N, dtype=torch.long, device=dev)
            check(lib().dn_lrp_collapse_count_i32(N, E, L, *self._args(), ptr(self.dummy), ptr(per_node), stream_ptr()),
                  "dn_lrp_collapse_count_i32")
            ptr64 = torch.cat([per_node.new_zeros(1), torch.cumsum(per_node, 0)])
            Q = int(ptr64[-1])
            if Q > _INT32_MAX:
                raise _lib.DnHipError("LRP index: %d collapsed rows do not fit an int32 index" % Q)
            col_ptr = ptr64.to(I32)
            rows = torch.empty(Q, dtype=I32, device=dev)
            cnt = torch.empty(Q, dtype=torch.long, device=dev)
            check(lib().dn_lrp_collapse_fill_i32(N, E, L, *self._args(), ptr(self.dummy), ptr(col_ptr), Q, ptr(rows), ptr(cnt),
                                                 stream_ptr()), "dn_lrp_collapse_fill_i32")
            node = torch.repeat_interleave(torch.arange(N, device=dev, dtype=I32), per_node, output_size=Q)
            order = torch.sort(node.long() * max(R, 1) + rows.long())[1]          # distinct keys: the order is unique
            rows, cnt = rows.index_select(0, order).contiguous(), cnt.index_select(0, order).contiguous()
            tptr, tperm = csr_build(rows, R)
            self._collapsed = LrpCollapsed(col_ptr, rows, cnt, node, tptr, tperm)
        return self._collapsed

    def collapsed_scale(self, pool):
        """(scale [Q], its transposed order, the transposed node list) of ops.lrp_pool_linear: occurrences / P_v, divided in
        double and rounded to fp32, for pool = "mean"; the occurrences for "sum"."""
        if pool not in self._collapsed_scale:
            c = self.collapsed()
            if pool == "mean":
                scale = (c.col_cnt.double() / self.count.index_select(0, c.col_node.long()).double()).float()
            else:
                scale = c.col_cnt.float()
            t = c.tperm.long()
            self._collapsed_scale[pool] = (scale.contiguous(), scale.index_select(0, t).contiguous(),
                                           c.col_node.index_select(0, t).contiguous())
        return self._collapsed_scale[pool]


def _lrp_index_of(graph, seq_len):
    if isinstance(graph, LrpIndex):
        if graph.seq_len != int(seq_len):
            raise ValueError("the LRP index was built for sequence length %d, not %d" % (graph.seq_len, seq_len))
        return graph
    return graph.lrp_index(seq_len)


def lrp_perm_index(graph, seq_len=4):
    """The materialised ego-net permutation index of a BatchedGraph (or an LrpIndex): LrpPermIndex(perm_ptr [N + 1],
    perm_nodes [P, L], perm_edges [P, L * L]), int32 with -1 for empty; as row / column lists it is the reference's
    node_to_perm / edge_to_perm matrices (dataset.py:1843-1886), order included."""
    return _lrp_index_of(graph, seq_len).perm_index()


class _GatherSegsumFn(torch.autograd.Function):
    """out[s] = sum of x[idx[i]] over segment s (gather_segsum); backward: the same kernel over the transposed lists."""

    @staticmethod
    def forward(ctx, x, idx, ptr_, tptr, tseg):
        ctx.tables, ctx.rows = (tptr, tseg), x.shape[0]
        return gather_segsum(x.contiguous(), idx, ptr_)

    @staticmethod
    def backward(ctx, g):
        tptr, tseg = ctx.tables
        return gather_segsum(g.contiguous(), tseg, tptr, ctx.rows), None, None, None, None


class _LrpPoolFn(torch.autograd.Function):
    """The fused pooling (dn_lrp_pool_fwd_f32 / _bwd_f32) over the row-factorised tables t_node [N, L H], t_edge [E, L (L-1) H].
    The backward adds into zeroed tables with fp32 atomics: exact sums, not bit-repeatable on general inputs."""

    @staticmethod
    def forward(ctx, t_node, t_edge, bias, factor, ix, H, pool_mean, act_on, slope):
        t_node, t_edge = t_node.contiguous(), t_edge.contiguous()
        bias = None if bias is None else bias.contiguous()
        factor = None if factor is None else factor.contiguous()
        require_gpu(t_node, t_edge, bias, factor)
        N, E, L = ix.num_nodes, ix.num_edges, ix.seq_len
        if t_node.shape != (N, L * H) or t_edge.shape != (E, L * (L - 1) * H) or t_node.dtype != torch.float32 or \
                t_edge.dtype != torch.float32 or (factor is not None and (factor.shape != (N, H) or factor.dtype != torch.float32)) or \
                (bias is not None and (bias.numel() != H or bias.dtype != torch.float32)):
            raise _lib.DnHipError("lrp_pool: fp32 t_node [N, L H], t_edge [E, L (L - 1) H], bias [H], factor [N, H] expected")
        out = torch.empty((N, H), dtype=torch.float32, device=t_node.device)
        pooled = torch.empty_like(out) if factor is not None else None
        launch_tagged("lrp_pool_fwd", lambda: check(lib().dn_lrp_pool_fwd_f32(
            N, E, H, L, *ix._args(), ptr(t_node), ptr(t_edge), ptr(bias), ptr(factor), int(pool_mean), int(act_on), float(slope),
            ptr(pooled), ptr(out), stream_ptr()), "dn_lrp_pool_fwd_f32"))
        ctx.ix, ctx.H, ctx.mode = ix, H, (int(pool_mean), int(act_on), float(slope))
        ctx.has = (bias is not None, factor is not None)
        empty = t_node.new_empty(0)
        ctx.save_for_backward(t_node, t_edge, bias if bias is not None else empty, factor if factor is not None else empty,
                              pooled if pooled is not None else empty)
        return out

    @staticmethod
    def backward(ctx, g):
        t_node, t_edge, bias, factor, pooled = ctx.saved_tensors
        ix, H = ctx.ix, ctx.H
        has_bias, has_factor = ctx.has
        g = g.contiguous().float()
        d_tnode, d_tedge = torch.zeros_like(t_node), torch.zeros_like(t_edge)
        d_bias = torch.zeros(H, dtype=torch.float32, device=g.device) if has_bias else None
        d_factor = torch.empty_like(g) if has_factor else None
        launch_tagged("lrp_pool_bwd", lambda: check(lib().dn_lrp_pool_bwd_f32(
            ix.num_nodes, ix.num_edges, H, ix.seq_len, *ix._args(), ptr(t_node), ptr(t_edge), ptr(bias) if has_bias else None,
            ptr(factor) if has_factor else None, *ctx.mode, ptr(pooled) if has_factor else None, ptr(g), ptr(d_tnode), ptr(d_tedge),
            ptr(d_bias), ptr(d_factor), stream_ptr()), "dn_lrp_pool_bwd_f32"))
        return d_tnode, d_tedge, d_bias, d_factor, None, None, None, None, None


def _lrp_act(t, act):
    if act == "relu":
        return torch.relu(t)
    if act == "leaky_relu":
        return torch.nn.functional.leaky_relu(t, LRP_LEAKY_SLOPE)
    return t


def _lrp_tables(x, edge_feat, weight, L):
    """(T_node [N, L H], T_edge [E, L (L - 1) H], H): the weight [in, H, L^2] row-factorised on the Linear kernels."""
    require_gpu(x.contiguous(), edge_feat.contiguous())
    H = int(weight.shape[1])
    wt = weight.permute(2, 1, 0)                                          # [L * L, H, in]
    diag = [k * (L + 1) for k in range(L)]
    off = [s for s in range(L * L) if s % (L + 1) != 0]
    t_node = linear_any(x, wt[diag].reshape(L * H, -1))                   # [N, L * H]
    t_edge = linear_any(edge_feat, wt[off].reshape(L * (L - 1) * H, -1))  # [E, L * (L - 1) * H]
    return t_node, t_edge, H


def lrp_pool(x, edge_feat, weight, bias, factor, graph, seq_len=4, act="relu", pool="mean"):
    """[N, H] = act(pool_p(act(sum_slots W_slot^T row_slot + bias)) * factor) of lrp.py:65-75 without its [P L^2, in] tensor.
    x [N, in], edge_feat [E, in], weight [in, H, L^2] (the reference's parameter), bias [H] or None, factor [N, H] or None (then no
    scale and no second activation), graph a BatchedGraph (its cached LrpIndex) or an LrpIndex; act "relu" | "leaky_relu"
    (slope 1 / 5.5) | "none"; pool "mean" | "sum".  fp32.  The weight is row-factorised: T_node = x @ [W_0 | W_(L+1) | ...] and
    T_edge = edge_feat @ [off-diagonal slots] on the Linear kernels (linear_any), then dn_lrp_pool_* (one workgroup per node
    enumerates the node's sequences; `with ops.lrp_fused():`, and by itself when the sequence list does not fit the materialised
    index) -- or, by default and for widths the kernel does not take, gather_segsum over the materialised index and
    dn_segment_mean / _sum (ops.LRP_FUSED_DEFAULT)."""
    if act not in ("relu", "leaky_relu", "none") or pool not in ("mean", "sum"):
        raise ValueError("lrp_pool: act in relu | leaky_relu | none and pool in mean | sum (got %s, %s)" % (act, pool))
    ix = _lrp_index_of(graph, seq_len)
    L = ix.seq_len
    if weight.dim() != 3 or weight.shape[2] != L * L or x.shape[1] != weight.shape[0] or edge_feat.shape[1] != weight.shape[0]:
        raise _lib.DnHipError("lrp_pool: weight [in, H, L * L] with in = the width of x and edge_feat expected")
    if x.shape[0] != ix.num_nodes or edge_feat.shape[0] != ix.num_edges:
        raise _lib.DnHipError("lrp_pool: one x row per node and one edge_feat row per edge of the indexed batch expected")
    t_node, t_edge, H = _lrp_tables(x, edge_feat, weight, L)
    forced = lrp_fused.override()
    fused = (LRP_FUSED_DEFAULT or not ix.materialisable()) if forced is None else forced
    if fused and lrp_fused_supported(H) and x.dtype == torch.float32:
        slope = LRP_LEAKY_SLOPE if act == "leaky_relu" else 0.0
        return _LrpPoolFn.apply(t_node, t_edge, bias, factor, ix, H, pool == "mean", act != "none", slope)
    idx, ptr_, tptr, tseg = ix.composed_tables()
    table = torch.cat([t_node.reshape(-1, H), t_edge.reshape(-1, H)], 0)
    z = _GatherSegsumFn.apply(table, idx, ptr_, tptr, tseg)
    if bias is not None:
        z = z + bias
    out = segment_reduce(_lrp_act(z, act), ix.perm_index().perm_ptr, pool)
    return out if factor is None else _lrp_act(out * factor, act)


class _WeightedSegsumFn(torch.autograd.Function):
    """out[s] = sum of scale[i] x[idx[i]] over segment s (gather_segsum); backward: the same kernel over the transposed lists,
    every sum in a fixed order."""

    @staticmethod
    def forward(ctx, x, idx, ptr_, scale, tptr, tseg, tscale):
        ctx.tables, ctx.rows = (tptr, tseg, tscale), x.shape[0]
        return gather_segsum(x.contiguous(), idx, ptr_, scale=scale, tag="lrp_collapsed")

    @staticmethod
    def backward(ctx, g):
        tptr, tseg, tscale = ctx.tables
        return (gather_segsum(g.contiguous(), tseg, tptr, ctx.rows, scale=tscale, tag="lrp_collapsed_bwd"),) + (None,) * 6


def lrp_pool_linear(x, edge_feat, weight, bias, graph, seq_len=4, pool="mean"):
    """[N, H] = pool_p(sum_slots W_slot^T row_slot + bias) of dmplrp.py:180-185: lrp_pool without activation and factor, where the
    pooling commutes with the sum over the slots.  The same row-factorised tables as lrp_pool, then ONE weighted gather_segsum over
    the collapsed index (LrpIndex.collapsed: per node the distinct table rows of its sequences, scale = occurrences / P_v for
    "mean", occurrences for "sum"), + bias (mean) or + P_v bias (sum); the backward runs the same kernel over the transposed lists,
    so both directions are deterministic.  Any width gather_segsum takes.  `with ops.lrp_collapsed(False):` runs
    lrp_pool(act="none", factor=None) instead (ops.LRP_COLLAPSED_DEFAULT)."""
    if pool not in ("mean", "sum"):
        raise ValueError("lrp_pool_linear: pool in mean | sum (got %s)" % pool)
    if not lrp_collapsed_enabled():
        return lrp_pool(x, edge_feat, weight, bias, None, graph, seq_len, act="none", pool=pool)
    ix = _lrp_index_of(graph, seq_len)
    L = ix.seq_len
    if weight.dim() != 3 or weight.shape[2] != L * L or x.shape[1] != weight.shape[0] or edge_feat.shape[1] != weight.shape[0]:
        raise _lib.DnHipError("lrp_pool_linear: weight [in, H, L * L] with in = the width of x and edge_feat expected")
    if x.shape[0] != ix.num_nodes or edge_feat.shape[0] != ix.num_edges:
        raise _lib.DnHipError("lrp_pool_linear: one x row per node and one edge_feat row per edge of the indexed batch expected")
    t_node, t_edge, H = _lrp_tables(x, edge_feat, weight, L)
    col = ix.collapsed()
    scale, tscale, tnode = ix.collapsed_scale(pool)
    table = torch.cat([t_node.reshape(-1, H), t_edge.reshape(-1, H)], 0)
    out = _WeightedSegsumFn.apply(table, col.col_rows, col.col_ptr, scale, col.tptr, tnode, tscale)
    if bias is None:
        return out
    return out + bias if pool == "mean" else out + ix.count.to(out.dtype).unsqueeze(1) * bias


# ----------------------------------------------------------------------------------------------
# HGT: rows times the weight of their node type, and the edge-softmax attention (dn_hgt.hip)
# ----------------------------------------------------------------------------------------------
HGT_MAX_H = 256
HGT_HEADS = (1, 2, 4, 8)

# The layers' default.  Measured on the scale batch (docs/LAB_NOTES.md "SI count models: HGT"; H = 64, 4 heads, 14 relations, 25.6 k
# nodes, 155 k edges, fused and composed alternated in one process): the layer step 1.72 against 2.54 ms, the model step 10.4 against
# 12.5 ms, every fused round faster than every composed round -- outside the spread, so the fused kernels are the default (unlike
# LRP_FUSED_DEFAULT / DUAL_FUSED_DEFAULT, whose gains stayed inside it).
HGT_FUSED_DEFAULT = True


def hgt_fused_enabled():
    return hgt_fused.override(HGT_FUSED_DEFAULT)


class hgt_fused(_ThreadSwitch):
    """Context manager: HeteroGraphTransLayer forwards started inside it (on this thread) run their attention on dn_hgt.hip (on=True)
    where hgt_fused_supported allows it, or on the composed path (on=False: torch scatter ops over the same factorisation)."""
    _slot = "hgt_fused"


def hgt_fused_supported(x, heads):
    """The predicate of the fused attention: fp32 rows on the GPU, heads in {1, 2, 4, 8}, H <= 256, H / heads a multiple of 4."""
    H, heads = int(x.shape[-1]), int(heads)
    return (x.is_cuda and x.dtype == torch.float32 and heads in HGT_HEADS and H <= HGT_MAX_H and H % heads == 0
            and (H // heads) % 4 == 0)


class TypeIndex:
    """The rows of a batch grouped by an integer type (the node label): perm / inv between the given and the grouped order and
    the tile / chunk tables of the any-width grouped products (dn_rows_gemm_* / dn_rows_wgrad_any_*).  Built once per batch."""

    def __init__(self, types, num_types):
        require_gpu(types)
        T, n = int(num_types), int(types.numel())
        t = types.reshape(-1).long()
        if n:
            lo, hi = (int(v) for v in torch.aminmax(t))
            if lo < 0 or hi >= T:
                raise _lib.DnHipError("node type out of [0, %d): min %d, max %d" % (T, lo, hi))
        self.num_types, self.num_rows = T, n
        self.perm = torch.argsort(t, stable=True)
        self.inv = torch.empty_like(self.perm)
        self.inv[self.perm] = torch.arange(n, device=t.device)
        cnt = torch.bincount(t, minlength=T)
        tptr = torch.cat([cnt.new_zeros(1), torch.cumsum(cnt, 0)]).to(I32)
        self.type_ptr = tptr
        self.tiles = build_row_tables(tptr, T, n, 64)
        self.chunks = build_row_tables(tptr, T, n, 1024, want_ptr=True)


class _TypedLinearFn(torch.autograd.Function):
    """y[i] = x[i] @ W[type_i] for any widths: the rows grouped by type, one dn_rows_gemm_* launch; backward one launch for d x and
    the deterministic split-K weight gradient (dn_rows_wgrad_any_*)."""

    @staticmethod
    def forward(ctx, x, W, tix):
        xs = x.index_select(0, tix.perm)
        y = rows_gemm(xs, W, tix.tiles).index_select(0, tix.inv)
        ctx.tix = tix
        ctx.save_for_backward(xs, W)
        return y

    @staticmethod
    def backward(ctx, g):
        xs, W = ctx.saved_tensors
        tix = ctx.tix
        gs = g.index_select(0, tix.perm)
        gx = gW = None
        if ctx.needs_input_grad[0]:
            gx = rows_gemm(gs, W, tix.tiles, transpose_w=True).index_select(0, tix.inv)
        if ctx.needs_input_grad[1]:
            gW = rows_wgrad_any(xs, gs, tix.chunks, W.shape[0])
        return gx, gW, None


def typed_linear(x, W, types, tix=None):
    """x [N, K] times W[type of the row] ([T, K, M]) -> [N, M].  fp32 / bf16 on the GPU: the grouped product kernels over a
    TypeIndex (tix, or built here from `types`); anything else: the gathered torch product."""
    if x.is_cuda and x.dim() == 2 and x.dtype == W.dtype and x.dtype in MFMA_DTYPES and x.shape[0] > 0:
        return _TypedLinearFn.apply(x, W, tix if tix is not None else TypeIndex(types, W.shape[0]))
    return torch.bmm(x.unsqueeze(1), W.index_select(0, types.reshape(-1).long())).squeeze(1)


class HgtIndex:
    """The edges of a batch sorted by (destination, edge type), the non-empty (destination, edge type) PAIRS numbered in that order,
    and the reverse CSR by source over the sorted order (int32, device).  pair_ptr [P + 1] bounds the edges of a pair, dst_ptr
    [N + 1] the pairs of a destination (consecutive), pair_rel [P] is the pair's type.  The per-pair tensors of the layer (Qp, U and
    their gradients) live in ROWS grouped by edge type -- the order of the relation-grouped products, so nothing is permuted between
    the products and the attention: pair_row [P] is a pair's row, row_dst / row_rel [P] name the pair of a row, row_s [E] is the row
    of an edge's pair.  Built once per batch with torch sorts and scans."""

    def __init__(self, src, dst, etype, num_nodes, num_rels):
        require_gpu(src, dst, etype)
        N, R, E = int(num_nodes), int(num_rels), int(src.numel())
        _check_edge_types(etype, R)
        self.num_nodes, self.num_rels, self.num_edges = N, R, E
        src, dst, etype = src.reshape(-1).long(), dst.reshape(-1).long(), etype.reshape(-1).long()
        if dst.numel() != E or etype.numel() != E:
            raise _lib.DnHipError("HgtIndex: src, dst and etype must have one entry per edge")
        if E:                                                                  # (the kernels index rows by these: checked once per batch)
            lo, hi = (int(v) for v in torch.aminmax(torch.stack([src, dst])))
            if lo < 0 or hi >= N:
                raise _lib.DnHipError("HgtIndex: node id out of [0, %d): min %d, max %d" % (N, lo, hi))
        dev = src.device
        key = dst * R + etype
        self.perm = torch.argsort(key, stable=True)
        key_s = key.index_select(0, self.perm)
        self.src_l, self.dst_l = src.index_select(0, self.perm), dst.index_select(0, self.perm)
        self.et_l = etype.index_select(0, self.perm)
        pair_key, pair_l, cnt = torch.unique_consecutive(key_s, return_inverse=True, return_counts=True)
        P = int(pair_key.numel())
        self.num_pairs = P
        zero = torch.zeros(1, dtype=torch.long, device=dev)
        self.pair_ptr = torch.cat([zero, torch.cumsum(cnt, 0)]).to(I32)
        pair_dst = torch.div(pair_key, R, rounding_mode="floor")
        pair_rel = pair_key - pair_dst * R
        self.pair_rel = pair_rel.to(I32)
        self.dst_ptr = torch.cat([zero, torch.cumsum(torch.bincount(pair_dst, minlength=N), 0)]).to(I32)
        self.src_s, self.et_s = self.src_l.to(I32), self.et_l.to(I32)
        if P:
            t = self.pair_types = TypeIndex(self.pair_rel, R)                  # rows: the pairs grouped by edge type
            pair_row = t.inv
            self.row_dst_l, self.row_rel_l = pair_dst.index_select(0, t.perm), pair_rel.index_select(0, t.perm)
        else:
            self.pair_types = None
            pair_row = self.row_dst_l = self.row_rel_l = pair_dst
        self.pair_row = pair_row.to(I32)
        self.row_l = pair_row.index_select(0, pair_l)
        self.row_s = self.row_l.to(I32)
        operm = torch.argsort(self.src_l, stable=True)
        self.out_ptr = torch.cat([zero, torch.cumsum(torch.bincount(src, minlength=N), 0)]).to(I32)
        self.out_pos = operm.to(I32)
        self.out_row = self.row_s.index_select(0, operm).contiguous()
        self._pri_csr = None

    def pri_csr(self):
        """The rows of every edge type (contiguous) as a _SplitCSR: the fixed-order sum of the per-pair partials of d relation_pri."""
        if self._pri_csr is None:
            rows = torch.arange(self.num_pairs, dtype=I32, device=self.pair_rel.device)
            self._pri_csr = _SplitCSR(self.pair_types.type_ptr, rows, self.num_rels)
        return self._pri_csr


class _HgtPairExpandFn(torch.autograd.Function):
    """Qp [P, H] (rows grouped by edge type): Qp[row] = q[row_dst[row]] @ W[row_rel[row]] -- one row gather, ONE relation-grouped product
    (dn_rows_gemm_*).  Backward: the transposed product, the sum over the pairs of every destination (a gather over pair_row), and
    the deterministic split-K weight gradient."""

    @staticmethod
    def forward(ctx, q, W, ix):
        xs = q.index_select(0, ix.row_dst_l)
        ctx.ix = ix
        ctx.save_for_backward(xs, W)
        return rows_gemm(xs, W, ix.pair_types.tiles)

    @staticmethod
    def backward(ctx, g):
        xs, W = ctx.saved_tensors
        ix = ctx.ix
        t = ix.pair_types
        g = g.contiguous()
        gq = gW = None
        if ctx.needs_input_grad[0]:
            gq = gather_segsum(rows_gemm(g, W, t.tiles, transpose_w=True), ix.pair_row, ix.dst_ptr, ix.num_nodes)
        if ctx.needs_input_grad[1]:
            gW = rows_wgrad_any(xs, g, t.chunks, W.shape[0])
        return gq, gW, None


class _HgtPairReduceFn(torch.autograd.Function):
    """agg [N, H]: agg[d] = sum over the pairs p of d of U[pair_row[p]] @ W[pair_rel[p]] (one relation-grouped product over the rows,
    one segment sum)."""

    @staticmethod
    def forward(ctx, U, W, ix):
        ctx.ix = ix
        ctx.save_for_backward(U, W)
        return gather_segsum(rows_gemm(U, W, ix.pair_types.tiles), ix.pair_row, ix.dst_ptr, ix.num_nodes)

    @staticmethod
    def backward(ctx, g):
        U, W = ctx.saved_tensors
        ix = ctx.ix
        t = ix.pair_types
        gs = g.index_select(0, ix.row_dst_l)                                                # d Y, row by row
        gU = gW = None
        if ctx.needs_input_grad[0]:
            gU = rows_gemm(gs, W, t.tiles, transpose_w=True)
        if ctx.needs_input_grad[1]:
            gW = rows_wgrad_any(U, gs, t.chunks, W.shape[0])
        return gU, gW, None


def _hgt_products_on_kernels(x, W, ix):
    return x.is_cuda and x.dtype == W.dtype and x.dtype in MFMA_DTYPES and ix.num_pairs > 0


def hgt_pair_expand(q, W, ix):
    """Qp [P, H] = q[row_dst] @ W[row_rel] (W [R, H, H]; rows grouped by edge type, see HgtIndex)."""
    if _hgt_products_on_kernels(q, W, ix):
        return _HgtPairExpandFn.apply(q.contiguous(), W.contiguous(), ix)
    return torch.bmm(q.index_select(0, ix.row_dst_l).unsqueeze(1), W.index_select(0, ix.row_rel_l)).squeeze(1)


def hgt_pair_reduce(U, W, ix):
    """agg [N, H] = sum over the pairs of every destination of U[row] @ W[row_rel[row]] (W [R, H, H])."""
    if _hgt_products_on_kernels(U, W, ix):
        return _HgtPairReduceFn.apply(U.contiguous(), W.contiguous(), ix)
    Y = torch.bmm(U.unsqueeze(1), W.index_select(0, ix.row_rel_l)).squeeze(1)
    return torch.zeros((ix.num_nodes, W.shape[2]), dtype=Y.dtype, device=Y.device).index_add(0, ix.row_dst_l, Y)


class _HgtAttnFn(torch.autograd.Function):
    """U [P, H] of dn_hgt_attn_fwd_f32 from Qp [P, H] (both in HgtIndex rows), k, v [N, H] and pri [R, heads]; backward: dn_hgt_attn_bwd_dst_f32 (d Qp, the
    per-pair partials of d pri, summed here per edge type in a fixed order) and dn_hgt_attn_bwd_src_f32 (d k, d v).  Deterministic."""

    @staticmethod
    def forward(ctx, Qp, k, v, pri, ix, heads, scale):
        Qp, k, v, pri = Qp.contiguous(), k.contiguous(), v.contiguous(), pri.contiguous()
        require_gpu(Qp, k, v, pri)
        N, R, E, P, H = ix.num_nodes, ix.num_rels, ix.num_edges, ix.num_pairs, int(k.shape[1])
        if Qp.shape != (P, H) or k.shape != (N, H) or v.shape != (N, H) or pri.shape != (R, heads):
            raise _lib.DnHipError("hgt_attention: Qp [P, H], k / v [N, H] and pri [R, heads] expected")
        U = torch.empty((P, H), dtype=torch.float32, device=k.device)
        att = torch.empty((E, heads), dtype=torch.float32, device=k.device)
        launch_tagged("hgt_attn_fwd", lambda: check(lib().dn_hgt_attn_fwd_f32(
            N, E, P, H, heads, ptr(ix.dst_ptr), ptr(ix.pair_ptr), ptr(ix.pair_row), ptr(ix.src_s), ptr(ix.et_s), ptr(ix.row_s), ptr(Qp), ptr(k),
            ptr(v), ptr(pri), float(scale), ptr(att), ptr(U), stream_ptr()), "dn_hgt_attn_fwd_f32"))
        ctx.ix, ctx.heads, ctx.scale = ix, int(heads), float(scale)
        ctx.save_for_backward(Qp, k, v, pri, att)
        return U

    @staticmethod
    def backward(ctx, dU):
        Qp, k, v, pri, att = ctx.saved_tensors
        ix, heads, scale = ctx.ix, ctx.heads, ctx.scale
        N, R, E, P, H = ix.num_nodes, ix.num_rels, ix.num_edges, ix.num_pairs, int(k.shape[1])
        dU = dU.contiguous()
        dev = k.device
        dl = torch.empty((E, heads), dtype=torch.float32, device=dev)
        dQp = torch.empty_like(Qp)
        part = torch.empty((P, heads), dtype=torch.float32, device=dev)
        launch_tagged("hgt_attn_bwd_dst", lambda: check(lib().dn_hgt_attn_bwd_dst_f32(
            N, E, P, H, heads, ptr(ix.dst_ptr), ptr(ix.pair_ptr), ptr(ix.pair_rel), ptr(ix.pair_row), ptr(ix.src_s), ptr(ix.row_s), ptr(Qp), ptr(k),
            ptr(v), ptr(pri), scale, ptr(att), ptr(dU), ptr(dl), ptr(dQp), ptr(part), stream_ptr()), "dn_hgt_attn_bwd_dst_f32"))
        dk, dv = torch.empty_like(k), torch.empty_like(v)
        launch_tagged("hgt_attn_bwd_src", lambda: check(lib().dn_hgt_attn_bwd_src_f32(
            N, E, P, H, heads, ptr(ix.out_ptr), ptr(ix.out_pos), ptr(ix.out_row), ptr(Qp), ptr(dU), ptr(att), ptr(dl), ptr(dk), ptr(dv),
            stream_ptr()), "dn_hgt_attn_bwd_src_f32"))
        dpri = ix.pri_csr().segsum(part) if P else torch.zeros_like(pri)
        return dQp, dk, dv, dpri, None, None, None


def hgt_attention_composed(Qp, k, v, pri, ix, heads, scale):
    """The same U [P, H] from torch gathers and scatter ops over the sorted edge list (any dtype; its sums are atomic adds)."""
    N, E, P, H = ix.num_nodes, ix.num_edges, ix.num_pairs, int(k.shape[1])
    dk = H // heads
    q_e = Qp.reshape(P, heads, dk).index_select(0, ix.row_l)
    k_e = k.reshape(N, heads, dk).index_select(0, ix.src_l)
    logit = (q_e * k_e).sum(-1) * pri.index_select(0, ix.et_l) * scale                                   # [E, heads]
    didx = ix.dst_l.view(-1, 1).expand(E, heads)
    mx = torch.full((N, heads), float("-inf"), dtype=logit.dtype, device=logit.device)
    mx = mx.scatter_reduce(0, didx, logit.detach(), "amax", include_self=True)
    p = torch.exp(logit - mx.index_select(0, ix.dst_l))
    sm = torch.zeros((N, heads), dtype=p.dtype, device=p.device).index_add(0, ix.dst_l, p)
    a = p / sm.index_select(0, ix.dst_l)
    msg = (a.unsqueeze(-1) * v.reshape(N, heads, dk).index_select(0, ix.src_l)).reshape(E, H)
    return torch.zeros((P, H), dtype=msg.dtype, device=msg.device).index_add(0, ix.row_l, msg)


def hgt_attention(Qp, k, v, pri, ix, heads, scale):
    """U [P, H]: per (destination, edge type) pair the softmax-weighted sum of the value rows over the pair's edges, the softmax
    running over ALL in-edges of the destination per head with logits <Qp[pair], k[src]> pri[et] scale.  The fused kernels
    (dn_hgt.hip) where hgt_fused_enabled() and hgt_fused_supported, else the composed path."""
    if hgt_fused_enabled() and hgt_fused_supported(k, heads) and Qp.dtype == v.dtype == pri.dtype == torch.float32:
        return _HgtAttnFn.apply(Qp, k, v, pri, ix, int(heads), float(scale))
    return hgt_attention_composed(Qp, k, v, pri, ix, int(heads), float(scale))


def block_diag_dense(blocks):
    """[..., B, si, so] -> [..., B si, B so] with the blocks on the diagonal, zeros elsewhere (torch, differentiable)."""
    B, si, so = blocks.shape[-3:]
    eye = torch.eye(B, dtype=blocks.dtype, device=blocks.device).view(B, 1, B, 1)
    return (blocks.unsqueeze(-2) * eye).reshape(blocks.shape[:-3] + (B * si, B * so))


def hgt_message_pass(q, k, v, att, msg, pri, ix, scale):
    """agg [N, H] of an HGT layer (hgt.py:252-264, 324-333): per destination and head the softmax over its in-edges of
    <q_dst, k_src @ att[et]> pri[et] scale, then the sum of a_e (v_src @ msg[et]).  q, k, v [N, H]; att, msg [R, heads, d_k, d_k];
    pri [R, heads]; ix an HgtIndex.  The relation matrices are applied on the destination side, once per (destination, edge type)
    pair that has an edge: Qp[p] = q_dst @ blockdiag(att[r])^T (hgt_pair_expand), the attention (hgt_attention) yields the weighted
    value sums U[p] per pair, and agg[d] = sum over the pairs of d of U[p] @ blockdiag(msg[r]) (hgt_pair_reduce)."""
    heads = int(att.shape[1])
    w_att = block_diag_dense(att.transpose(-1, -2))                  # Qp[p, (h, j)] = sum_i q[(h, i)] att[r, h, j, i]
    w_msg = block_diag_dense(msg)                                    # agg[(h, i)] += sum_j U[p, (h, j)] msg[r, h, j, i]
    Qp = hgt_pair_expand(q, w_att, ix)
    U = hgt_attention(Qp, k.contiguous(), v.contiguous(), pri, ix, heads, scale)
    return hgt_pair_reduce(U, w_msg, ix)


# ------------------------------------------------------------------------------------------------ WL / WLOA graph kernels
# (dn_wl.hip; the dataset side -- reader, node classes, features, command line -- is graph_kernels.py)
# The default of graph_kernels.wl_colors.  Measured by tools/graph_kernel_bench.py (docs/LAB_NOTES.md "Graph kernels: WL / WLOA"; 4096
# NCI1-shaped graphs with dummy nodes, H = 5, fused and composed alternated in one process): 0.13 against 1.99 ms for the five
# refinement steps, 0.27 against 2.95 ms with edge labels, spreads below 4 % -- far outside the spread, so the fused kernels are the default.
WL_FUSED_DEFAULT = True


def wl_fused_enabled():
    return wl_fused.override(WL_FUSED_DEFAULT)


class wl_fused(_ThreadSwitch):
    """Context manager: WL colour refinements started inside it (on this thread) sort in registers and LDS (on=True: dn_wl_refine_u64,
    lists of up to wl_max_entries() entries; longer ones take the composed path either way) or on the composed path (on=False: a
    device-wide segmented sort with torch ops, then dn_wl_fold_u64)."""
    _slot = "wl_fused"


def wl_max_entries():
    """The longest entry list (deg, or 2 deg with edge labels) the fused refinement sorts."""
    return int(lib().dn_wl_max_entries())


def wl_max_steps():
    return int(lib().dn_wl_max_steps())


def wl_gram_tile():
    return int(lib().dn_wl_gram_tile())


_WL_SIGN = -(1 << 63)          # xor with it: signed order of the int64 carriers == unsigned order of the colours


def wl_pairing(a, b):
    """Szudzik's pairing on int64 carriers of unsigned 64-bit values (wrapping; the comparison is unsigned)."""
    return torch.where((a ^ _WL_SIGN) >= (b ^ _WL_SIGN), a * a + a + b, a + b * b)


def wl_refine_fused(num_nodes, nodes, group, lds_entries, csr_ptr, nbr, edge_label, colors_in, colors_out):
    """One launch of dn_wl_refine_u64 for the node list `nodes` (int32; None: every node)."""
    require_gpu(nodes, csr_ptr, nbr, edge_label, colors_in, colors_out)
    n_list = int(num_nodes) if nodes is None else int(nodes.numel())
    check(lib().dn_wl_refine_u64(int(num_nodes), n_list, ptr(nodes), int(group), int(lds_entries), ptr(csr_ptr), ptr(nbr), ptr(edge_label),
                                 ptr(colors_in), ptr(colors_out), stream_ptr()), "dn_wl_refine_u64")


def wl_refine_composed(num_nodes, nodes, slots, seg, seg_ptr, nbr_long, edge_label, colors_in, colors_out):
    """The same step without the in-kernel sort: the entries of the listed nodes (slots: their CSR slots, seg: the list position of
    each slot's node, seg_ptr [len + 1] int64: where each node's entries start) are gathered, sorted device-wide by (node, value)
    with two stable torch sorts, and folded by dn_wl_fold_u64.  slots / seg None: every slot in CSR order (seg must then be given as
    the slot's node).  No read-back."""
    require_gpu(nodes, seg, seg_ptr, nbr_long, edge_label, colors_in, colors_out)
    n_list = int(num_nodes) if nodes is None else int(nodes.numel())
    a = colors_in[nbr_long if slots is None else nbr_long[slots]]
    if edge_label is not None:
        el = edge_label if slots is None else edge_label[slots]
        ent = torch.stack([a, wl_pairing(a, el)], 1).reshape(-1)
        seg = seg.repeat_interleave(2)
    else:
        ent = a
    key, order = torch.sort(ent ^ _WL_SIGN, stable=True)
    by_seg = torch.sort(seg[order], stable=True)[1]
    sorted_entries = (key[by_seg] ^ _WL_SIGN).contiguous()
    check(lib().dn_wl_fold_u64(int(num_nodes), n_list, ptr(nodes), ptr(seg_ptr), ptr(sorted_entries) if sorted_entries.numel() else None,
                               ptr(colors_in), ptr(colors_out), stream_ptr()), "dn_wl_fold_u64")


def wl_gram(feat_ptr, feat_color, feat_count, feat_step, num_graphs, num_steps, use_min):
    """[num_steps, B, B] int64: dn_wl_gram_i64 over a feature CSR (graph_kernels.wl_features)."""
    require_gpu(feat_ptr, feat_color, feat_count, feat_step)
    out = torch.empty((int(num_steps), int(num_graphs), int(num_graphs)), dtype=torch.int64, device=feat_ptr.device)
    check(lib().dn_wl_gram_i64(int(num_graphs), int(num_steps), int(bool(use_min)), ptr(feat_ptr), ptr(feat_color), ptr(feat_count),
                               ptr(feat_step), ptr(out), stream_ptr()), "dn_wl_gram_i64")
    return out


# ------------------------------------------------------------------------------------------------ SP / GR graph kernels
# (dn_gk.hip; the dataset side -- graph and centre classes, label ranks, composed paths, command line -- is graph_kernels_spgr.py)
# The defaults of graph_kernels_spgr.sp_features / gr_features, one per kernel.  Measured by tools/graph_kernel_spgr_bench.py
# (docs/LAB_NOTES.md "Graph kernels: SP / GR"), fused and composed alternated in one process: 4096 NCI1-shaped graphs with dummy nodes,
# SP 1.54 against 5.24 ms and GR 1.51 against 3.75 ms; 300 DD-shaped graphs, SP 105.1 against 110.7 ms and GR 103.1 against 161.7 ms;
# spreads of the per-round medians below 2 % -- outside the spread everywhere, so both default to the kernels.
GK_FUSED_DEFAULT = {"SP": True, "GR": True}


def gk_fused_enabled(kernel=None):
    """Whether `kernel` ("SP" or "GR") takes the dn_gk_* kernels; without a kernel: whether both do."""
    m = gk_fused.override()
    if m is not None:
        return m
    return all(GK_FUSED_DEFAULT.values()) if kernel is None else GK_FUSED_DEFAULT[kernel]


class gk_fused(_ThreadSwitch):
    """Context manager: SP / GR feature builds started inside it (on this thread) run the dn_gk_* kernels (on=True; SP graphs above
    gk_sp_lds_max_nodes() nodes take the composed path either way) or the composed torch-op path (on=False)."""
    _slot = "gk_fused"


def gk_sp_lds_max_nodes():
    """The largest graph whose adjacency bit matrix the fused SP kernel holds in LDS."""
    return int(lib().dn_gk_sp_lds_max_nodes())


def gk_sp(num_graphs, graphs, group, lds_nodes, node_ptr, csr_ptr, nbr, src_base, local_class, class_ptr, class_rank, counts=None,
          offsets=None, out_key=None, out_count=None):
    """One launch of dn_gk_sp_u64 for the graph list `graphs` (int32): the counting pass (counts) or the fill (offsets, out_*)."""
    require_gpu(graphs, node_ptr, csr_ptr, nbr, src_base, local_class, class_ptr, class_rank, counts, offsets, out_key, out_count)
    check(lib().dn_gk_sp_u64(int(num_graphs), int(graphs.numel()), ptr(graphs), int(group), int(lds_nodes), ptr(node_ptr), ptr(csr_ptr),
                             ptr(nbr), ptr(src_base), ptr(local_class), ptr(class_ptr), ptr(class_rank), ptr(counts), ptr(offsets),
                             0 if out_key is None else int(out_key.numel()), ptr(out_key), ptr(out_count), stream_ptr()), "dn_gk_sp_u64")


def gk_gr_keys(num_nodes, group, item_node, item_row0, item_row1, item_offset, csr_ptr, nbr, node_label, edge_label, node_graph, ws_key,
               ws_graph):
    """One launch of dn_gk_gr_keys_u64 for one class of work items of a chunk."""
    require_gpu(item_node, item_row0, item_row1, item_offset, csr_ptr, nbr, node_label, edge_label, node_graph, ws_key, ws_graph)
    check(lib().dn_gk_gr_keys_u64(int(num_nodes), int(item_node.numel()), int(group), ptr(item_node), ptr(item_row0), ptr(item_row1),
                                  ptr(item_offset), ptr(csr_ptr), ptr(nbr), ptr(node_label), ptr(edge_label), ptr(node_graph),
                                  int(min(ws_key.numel(), ws_graph.numel())), ptr(ws_key), ptr(ws_graph), stream_ptr()), "dn_gk_gr_keys_u64")


# ------------------------------------------------------------------------------------------------ 2-WL graph kernels
# (dn_kwl.hip; the dataset side -- tuples, classes, composed path, features, command line -- is graph_kernels_kwl.py)
# The default of graph_kernels_kwl.kwl_colors.  Measured by tools/graph_kernel_kwl_bench.py (docs/LAB_NOTES.md "Graph kernels: 2-WL"),
# fused and composed alternated in one process, initial colours + 3 steps: 512 NCI1-shaped graphs with dummy nodes, WL 0.93 against
# 94.5 ms, DWL 2.29 / 99.0, LWL 0.44 / 11.9, LWLC 0.23 / 5.7; 128 PROTEINS-shaped graphs (one above 128 nodes, composed either way), WL
# 19.0 / 79.4, DWL 25.8 / 83.2, LWL 0.44 / 8.4, LWLC 0.28 / 4.2; spreads of the per-round medians below 4 % -- far outside the spread on
# both shapes, so the fused kernels are the default.
KWL_FUSED_DEFAULT = True


def kwl_fused_enabled():
    return kwl_fused.override(KWL_FUSED_DEFAULT)


class kwl_fused(_ThreadSwitch):
    """Context manager: 2-WL refinements started inside it (on this thread) run the dn_kwl_* kernels (on=True; graphs above
    kwl_max_nodes() nodes (WL / DWL) or with a degree above kwl_max_entries() (LWL / LWLC) take the composed path either way) or the
    composed path (on=False: torch device ops, a device-wide segmented sort and dn_wl_fold_u64)."""
    _slot = "kwl_fused"


def kwl_max_nodes():
    """The largest graph whose colour matrix the fused WL / DWL step holds in LDS."""
    return int(lib().dn_kwl_max_nodes())


def kwl_max_entries():
    """The longest list (a node degree) the fused LWL / LWLC step sorts."""
    return int(lib().dn_kwl_max_entries())


def kwl_init(num_nodes, tup_v, tup_w, csr_ptr, nbr, node_label, edge_label, colors_out):
    """One launch of dn_kwl_init_u64: the initial colours of every tuple."""
    require_gpu(tup_v, tup_w, csr_ptr, nbr, node_label, edge_label, colors_out)
    check(lib().dn_kwl_init_u64(int(num_nodes), int(tup_v.numel()), ptr(tup_v), ptr(tup_w), ptr(csr_ptr), ptr(nbr), ptr(node_label),
                                ptr(edge_label), ptr(colors_out), stream_ptr()), "dn_kwl_init_u64")


def kwl_local(num_nodes, tuples, group, lds_entries, connected, tup_v, tup_w, row_ptr, node_first, csr_ptr, nbr, colors_in, colors_out):
    """One launch of dn_kwl_local_u64 (LWL / LWLC) for the tuple list `tuples` (int32; None: every tuple)."""
    require_gpu(tuples, tup_v, tup_w, row_ptr, node_first, csr_ptr, nbr, colors_in, colors_out)
    T = int(tup_v.numel())
    check(lib().dn_kwl_local_u64(int(num_nodes), T, T if tuples is None else int(tuples.numel()), ptr(tuples), int(group), int(lds_entries),
                                 int(bool(connected)), ptr(tup_v), ptr(tup_w), ptr(row_ptr), ptr(node_first), ptr(csr_ptr), ptr(nbr),
                                 ptr(colors_in), ptr(colors_out), stream_ptr()), "dn_kwl_local_u64")


def kwl_global(num_graphs, graphs, lds_nodes, malkin, node_ptr, tuple_ptr, csr_ptr, nbr, colors_in, colors_out, work):
    """One launch of dn_kwl_global_u64 (WL / DWL) for the graph list `graphs` (int32)."""
    require_gpu(graphs, node_ptr, tuple_ptr, csr_ptr, nbr, colors_in, colors_out, work)
    check(lib().dn_kwl_global_u64(int(num_graphs), int(colors_in.numel()), int(graphs.numel()), ptr(graphs), int(lds_nodes), int(bool(malkin)),
                                  ptr(node_ptr), ptr(tuple_ptr), ptr(csr_ptr), ptr(nbr), ptr(colors_in), ptr(colors_out), ptr(work),
                                  stream_ptr()), "dn_kwl_global_u64")


def kwl_fold_from_max(seg, key, num_segments):
    """The folds of the multisets (seg [E] int64 in 0 .. num_segments, key [E] int64 colour carriers; segment num_segments collects
    what is dropped): every segment sorted ascending (unsigned), started from its maximum and folded over the rest by dn_wl_fold_u64.
    Returns (fold [num_segments], size [num_segments]); the fold of an empty segment means nothing.  No read-back: the maxima are
    taken out of the sorted array by a scatter to compacted positions."""
    require_gpu(seg, key)
    S, E, dev = int(num_segments), int(key.numel()), key.device
    k1, order = torch.sort(key ^ _WL_SIGN, stable=True)
    seg2, by_seg = torch.sort(seg[order], stable=True)
    sorted_key = k1[by_seg] ^ _WL_SIGN
    end = torch.searchsorted(seg2, torch.arange(1, S + 1, device=dev))     # (bincount would read its maximum back)
    size = end - torch.cat([end.new_zeros(1), end[:-1]])
    some = size > 0
    top = sorted_key[(end - 1).clamp_(min=0)].contiguous()                  # the maximum of every non-empty segment
    keep = torch.ones(E + 1, dtype=torch.bool, device=dev)
    keep.scatter_(0, torch.where(some, end - 1, torch.full_like(end, E)), False)      # (slot E: nobody's; a scalar index_put would sync)
    keep = keep[:E]
    dest = torch.where(keep, torch.cumsum(keep, 0) - 1, torch.full((E,), E, dtype=torch.int64, device=dev))
    rest = torch.empty(E + 1, dtype=torch.int64, device=dev)
    rest[dest] = sorted_key
    seg_ptr = torch.cat([end.new_zeros(1), end - torch.cumsum(some, 0)]).contiguous()
    fold = torch.empty(S, dtype=torch.int64, device=dev)
    check(lib().dn_wl_fold_u64(S, S, None, ptr(seg_ptr), ptr(rest), ptr(top), ptr(fold), stream_ptr()), "dn_wl_fold_u64")
    return fold, size


# ------------------------------------------------------------------------------------------------ 3-WL graph kernels
# (dn_k3wl.hip; the dataset side -- items, classes, composed path, features, command line -- is graph_kernels_k3wl.py)
# The default of graph_kernels_k3wl.k3wl_colors, one per kernel.  Measured by tools/graph_kernel_k3wl_bench.py (docs/LAB_NOTES.md
# "Graph kernels: 3-WL"), fused and composed alternated in one process, initial colours + 2 steps: 188 MUTAG-shaped graphs with dummy
# nodes, WL 0.84 against 222.7 ms, DWL 0.85 / 234.4, LWL 1.60 / 40.8, LWLC 1.05 / 12.1; 16 graphs of about 40 nodes, WL 0.94 / 230.8,
# DWL 0.95 / 241.8, LWL 0.88 / 25.8, LWLC 0.45 / 7.9; spreads of the per-round medians below 6 % -- far outside the spread for every
# kernel on both shapes, so all four default to the kernels.
K3WL_FUSED_DEFAULT = {"WL": True, "DWL": True, "LWL": True, "LWLC": True}


def k3wl_fused_enabled(kernel=None):
    """Whether `kernel` ("WL", "DWL", "LWL" or "LWLC") takes the dn_k3wl_* kernels; without a kernel: whether all four do."""
    m = k3wl_fused.override()
    if m is not None:
        return m
    return all(K3WL_FUSED_DEFAULT.values()) if kernel is None else K3WL_FUSED_DEFAULT[kernel]


class k3wl_fused(_ThreadSwitch):
    """Context manager: 3-WL refinements started inside it (on this thread) run the dn_k3wl_* kernels (on=True; graphs above
    k3wl_max_nodes() nodes (WL / DWL) or with a degree above k3wl_max_entries() (LWL / LWLC) take the composed path either way) or the
    composed path (on=False: torch device ops, a device-wide segmented sort and dn_wl_fold_u64)."""
    _slot = "k3wl_fused"


def k3wl_max_nodes():
    """The largest graph whose fibres the fused WL / DWL step sorts in one wavefront."""
    return int(lib().dn_k3wl_max_nodes())


def k3wl_max_entries():
    """The largest degree of a graph the fused LWL / LWLC step takes (LWLC's merged list holds up to twice as many entries)."""
    return int(lib().dn_k3wl_max_entries())


def k3wl_init(num_nodes, connected, tup_v, tup_w, tup_u, csr_ptr, nbr, node_label, colors_out):
    """One launch of dn_k3wl_init_u64: the initial colours of every item."""
    require_gpu(tup_v, tup_w, tup_u, csr_ptr, nbr, node_label, colors_out)
    check(lib().dn_k3wl_init_u64(int(num_nodes), int(tup_v.numel()), int(bool(connected)), ptr(tup_v), ptr(tup_w), ptr(tup_u), ptr(csr_ptr),
                                 ptr(nbr), ptr(node_label), ptr(colors_out), stream_ptr()), "dn_k3wl_init_u64")


def k3wl_local(num_nodes, items, group, lds_entries, connected, tup_v, tup_w, tup_u, node_graph, node_ptr, tuple_ptr, csr_ptr, nbr, item_key,
               item_slot, colors_in, colors_out):
    """One launch of dn_k3wl_local_u64 (LWL / LWLC) for the item list `items` (int32; None: every item)."""
    require_gpu(items, tup_v, tup_w, tup_u, node_graph, node_ptr, tuple_ptr, csr_ptr, nbr, item_key, item_slot, colors_in, colors_out)
    T = int(tup_v.numel())
    check(lib().dn_k3wl_local_u64(int(num_nodes), T, T if items is None else int(items.numel()), ptr(items), int(group), int(lds_entries),
                                  int(bool(connected)), ptr(tup_v), ptr(tup_w), ptr(tup_u), ptr(node_graph), ptr(node_ptr), ptr(tuple_ptr),
                                  ptr(csr_ptr), ptr(nbr), ptr(item_key), ptr(item_slot), ptr(colors_in), ptr(colors_out), stream_ptr()),
          "dn_k3wl_local_u64")


def k3wl_global(num_graphs, graphs, fib_ptr, num_fibres, group, malkin, node_ptr, tuple_ptr, adj_bits, colors_in, work):
    """One launch of dn_k3wl_global_u64 (the fibre pass of WL / DWL) for the graph list `graphs` (int32)."""
    require_gpu(graphs, fib_ptr, node_ptr, tuple_ptr, adj_bits, colors_in, work)
    check(lib().dn_k3wl_global_u64(int(num_graphs), int(colors_in.numel()), int(graphs.numel()), ptr(graphs), ptr(fib_ptr), int(num_fibres),
                                   int(group), int(bool(malkin)), ptr(node_ptr), ptr(tuple_ptr), ptr(adj_bits), ptr(colors_in), ptr(work),
                                   stream_ptr()), "dn_k3wl_global_u64")


def k3wl_close(num_nodes, malkin, tup_v, tup_w, tup_u, node_graph, node_ptr, csr_ptr, colors_in, work, colors_out):
    """One launch of dn_k3wl_close_u64 (the closing pass of WL / DWL) over every item."""
    require_gpu(tup_v, tup_w, tup_u, node_graph, node_ptr, csr_ptr, colors_in, work, colors_out)
    check(lib().dn_k3wl_close_u64(int(num_nodes), int(tup_v.numel()), int(bool(malkin)), ptr(tup_v), ptr(tup_w), ptr(tup_u), ptr(node_graph),
                                  ptr(node_ptr), ptr(csr_ptr), ptr(colors_in), ptr(work), ptr(colors_out), stream_ptr()), "dn_k3wl_close_u64")


# ----------------------------------------------------------------------------------------------
# SI count heads: ragged sparsemax / softmax attention and DIAMNet's window pooling (dn_seg_attn.hip)
# ----------------------------------------------------------------------------------------------
SEG_ATTN_MAX_H = 256
SEG_ATTN_HEADS = (1, 2, 4, 8)
SEG_ATTN_WAVE_KEYS = 64            # dn_seg_attn_wave_keys(): up to here a wavefront per (row, head)
SEG_ATTN_MAX_KEYS = 1024           # dn_seg_attn_max_keys(): above, the composed path
SEG_POOL_MAX_MEM = 64
SEG_SCORES = {"sparsemax": 0, "softmax": 1}
SEG_POOL_MODES = {"mean": 0, "sum": 1, "max": 2}

# The heads' default.  Measured on the scale batch (docs/LAB_NOTES.md "SI count heads: attention / DIAMNet"; 512 pairs, hidden 64, 4
# heads, fused and composed alternated in one process): the MeanAttnPredictNet head 2.99 against 6.01 ms on the node rows and 15.6
# against 35.2 ms on the edge rows, the DIAMNet heads 2.3 against 5.6 / 6.1 ms, the DMPNN step 15.9 against 25.2 ms (DIAMNet) and 29.0
# against 53.9 ms (MeanAttnPredictNet), every fused round faster than every composed round -- outside the spread, so the fused
# kernels are the default (as HGT_FUSED_DEFAULT).
ATTN_FUSED_DEFAULT = True


def attn_fused_enabled():
    return attn_fused.override(ATTN_FUSED_DEFAULT)


class attn_fused(_ThreadSwitch):
    """Context manager: seg_attention / seg_window_pool calls made inside it (on this thread) run on dn_seg_attn.hip (on=True) where
    attn_fused_supported allows it, or on the composed path (on=False: the padded torch computation of attn_pred.py on the ragged rows)."""
    _slot = "attn_fused"


def attn_fused_supported(x, heads, max_k=1):
    """The predicate of the fused attention: fp32 rows on the GPU, heads in {1, 2, 4, 8}, hidden <= 256, hidden / heads a power of two,
    at most 1024 keys per pair."""
    H, heads = int(x.shape[-1]), int(heads)
    if not (x.is_cuda and x.dtype == torch.float32 and heads in SEG_ATTN_HEADS and 1 <= H <= SEG_ATTN_MAX_H and H % heads == 0):
        return False
    dk = H // heads
    return dk & (dk - 1) == 0 and 1 <= int(max_k) <= SEG_ATTN_MAX_KEYS


def _max_len(ptr_):
    return int((ptr_[1:] - ptr_[:-1]).max()) if ptr_.numel() > 1 else 0


def _pad_index(ptr_, L, n):
    """(idx [B, L] long: the row of every left-aligned padded slot, clamped into the rows; valid [B, L] bool)."""
    p = ptr_.long()
    pos = torch.arange(int(L), device=ptr_.device).view(1, -1)
    valid = pos < (p[1:] - p[:-1]).view(-1, 1)
    idx = (p[:-1].view(-1, 1) + pos).clamp(max=max(int(n) - 1, 0))
    return idx, valid


class _SegAttnFn(torch.autograd.Function):
    """out [Nq, H] of dn_seg_attn_fwd_f32; backward: dn_seg_attn_bwd_q_f32 (dq and the row terms) and dn_seg_attn_bwd_kv_f32 (dk, dv).
    Saved: the inputs and stat [Nq, heads, 2].  Deterministic."""

    @staticmethod
    def forward(ctx, q, k, v, q_ptr, k_ptr, heads, scale, score, q_skip, k_skip, max_q, max_k):
        q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
        require_gpu(q, k, v, q_ptr, k_ptr, q_skip, k_skip)
        _i32(q_ptr, "q_ptr"), _i32(k_ptr, "k_ptr")
        Nq, H = q.shape
        Nk = k.shape[0]
        B = q_ptr.numel() - 1
        if k.shape != (Nk, H) or v.shape != (Nk, H) or k_ptr.numel() != B + 1 or B < 1:
            raise _lib.DnHipError("seg_attention: q [Nq, H], k / v [Nk, H] and two pointer arrays over the same B >= 1 pairs expected")
        if (q_skip is not None and q_skip.numel() != Nq) or (k_skip is not None and k_skip.numel() != Nk):
            raise _lib.DnHipError("seg_attention: one skip flag per row expected")
        out = torch.empty_like(q)
        stat = torch.empty((Nq, heads, 2), dtype=torch.float32, device=q.device)
        args = (B, Nq, Nk, H, heads, max_q, max_k, score, ptr(q_ptr), ptr(k_ptr), ptr(q_skip), ptr(k_skip), ptr(q), ptr(k), ptr(v), scale)
        if Nq and Nk:
            launch_tagged("seg_attn_fwd", lambda: check(lib().dn_seg_attn_fwd_f32(*args, ptr(out), ptr(stat), stream_ptr()),
                                                       "dn_seg_attn_fwd_f32"))
        else:
            out.zero_()
        ctx.args = (B, H, heads, max_q, max_k, score, scale, q_skip, k_skip)
        ctx.save_for_backward(q, k, v, q_ptr, k_ptr, stat)
        return out

    @staticmethod
    def backward(ctx, dout):
        q, k, v, q_ptr, k_ptr, stat = ctx.saved_tensors
        B, H, heads, max_q, max_k, score, scale, q_skip, k_skip = ctx.args
        dout = dout.contiguous()
        Nq, Nk = q.shape[0], k.shape[0]
        dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        if not (Nq and Nk):
            return (dq.zero_(), dk.zero_(), dv.zero_()) + (None,) * 9
        rterm = torch.empty((Nq, heads), dtype=torch.float64, device=q.device)
        args = (B, Nq, Nk, H, heads, max_q, max_k, score, ptr(q_ptr), ptr(k_ptr), ptr(q_skip), ptr(k_skip), ptr(q), ptr(k), ptr(v), scale,
                ptr(stat))
        launch_tagged("seg_attn_bwd_q", lambda: check(lib().dn_seg_attn_bwd_q_f32(*args, ptr(dout), ptr(dq), ptr(rterm), stream_ptr()),
                                                     "dn_seg_attn_bwd_q_f32"))
        launch_tagged("seg_attn_bwd_kv", lambda: check(lib().dn_seg_attn_bwd_kv_f32(*args, ptr(rterm), ptr(dout), ptr(dk), ptr(dv),
                                                                                   stream_ptr()), "dn_seg_attn_bwd_kv_f32"))
        return (dq, dk, dv) + (None,) * 9


def seg_attention_composed(q, k, v, q_ptr, k_ptr, heads, scale, score="sparsemax", q_skip=None, k_skip=None, max_q=None, max_k=None):
    """The same rows from the reference's algorithm: the rows padded to [B, L, H], the masked keys filled with -1e30, sparsemax or
    softmax along the key axis, the masked query rows cleared (any dtype, any device)."""
    from .subgraph_isomorphism.act import Sparsemax
    Nq, H = q.shape
    B, dk = q_ptr.numel() - 1, H // heads
    Lq = int(max_q) if max_q is not None else _max_len(q_ptr)
    Lk = int(max_k) if max_k is not None else _max_len(k_ptr)
    if Nq == 0 or k.shape[0] == 0 or Lk == 0:
        return q * 0
    qi, qv = _pad_index(q_ptr, Lq, Nq)
    ki, kv = _pad_index(k_ptr, Lk, k.shape[0])
    if q_skip is not None:
        qv = qv & ~q_skip.reshape(-1).bool()[qi]
    if k_skip is not None:
        kv = kv & ~k_skip.reshape(-1).bool()[ki]
    qp, kp, vp = q[qi].view(B, Lq, heads, dk), k[ki].view(B, Lk, heads, dk), v[ki].view(B, Lk, heads, dk)
    s = torch.einsum("bind,bjnd->bijn", qp, kp) * scale
    s = s.masked_fill(~kv.view(B, 1, Lk, 1), -1e30)
    s = Sparsemax(2)(s) if score == "sparsemax" else torch.softmax(s, dim=2)
    s = s * kv.view(B, 1, Lk, 1).to(s.dtype)                           # (a pair without a live key: zero rows)
    o = torch.einsum("bijn,bjnd->bind", s, vp).reshape(B, Lq, H).masked_fill(~qv.unsqueeze(-1), 0)
    _, inside = _pad_index(q_ptr, Lq, Nq)
    return o[inside]


def seg_attention(q, k, v, q_ptr, k_ptr, heads, scale, score="sparsemax", q_skip=None, k_skip=None, max_q=None, max_k=None):
    """out [Nq, hidden]: multi-head attention of the query rows of every pair over the pair's key rows with sparsemax or softmax
    weights (module comment of dn_seg_attn.hip).  q [Nq, hidden], k / v [Nk, hidden] are the projected rows, ragged by q_ptr / k_ptr
    [B + 1] int32; *_skip: uint8 / bool flags per row (a skipped key takes no weight, a skipped query row yields a zero row).
    max_q / max_k: the largest row counts per pair when the caller knows them (the SI models do, from si_read_meta); otherwise they
    are read back from the pointers.  The fused kernels where attn_fused_enabled() and attn_fused_supported (fp32, at most 1024
    keys per pair), else the composed path."""
    if score not in SEG_SCORES:
        raise ValueError("seg_attention: score must be 'sparsemax' or 'softmax' (got %r)" % (score,))
    heads = int(heads)
    if q.dim() != 2 or q.shape[1] % heads != 0:
        raise _lib.DnHipError("seg_attention: q [Nq, hidden] with hidden %% heads == 0 expected")
    if max_q is None:
        max_q = _max_len(q_ptr)
    if max_k is None:
        max_k = _max_len(k_ptr)
    if (attn_fused_enabled() and q.dtype == k.dtype == v.dtype and k.is_cuda and v.is_cuda
            and attn_fused_supported(q, heads, max(int(max_k), 1)) and q.shape[0] and k.shape[0] and max_q >= 1 and max_k >= 1):
        return _SegAttnFn.apply(q, k, v, q_ptr, k_ptr, heads, float(scale), SEG_SCORES[score], _u8_or_none(q_skip), _u8_or_none(k_skip),
                                int(max_q), int(max_k))
    return seg_attention_composed(q, k, v, q_ptr, k_ptr, heads, float(scale), score, q_skip, k_skip, max_q, max_k)


class _SegWindowPoolFn(torch.autograd.Function):
    """(mem [B mem_len, D], mem_mask [B, mem_len]) of dn_seg_window_pool_fwd_f32; the backward gathers per row (dn_seg_window_pool_bwd_f32)."""

    @staticmethod
    def forward(ctx, rows, ptr_, skip, mem_len, mode):
        rows = rows.contiguous()
        require_gpu(rows, ptr_, skip)
        _i32(ptr_, "ptr")
        N, D = rows.shape
        B = ptr_.numel() - 1
        dev = rows.device
        mem = torch.empty((B * mem_len, D), dtype=torch.float32, device=dev)
        mask = torch.empty((B, mem_len), dtype=torch.bool, device=dev)
        arg = torch.empty((B * mem_len, D), dtype=I32, device=dev) if mode == SEG_POOL_MODES["max"] else None
        span = torch.empty((B, 2), dtype=I32, device=dev)
        launch_tagged("seg_window_pool", lambda: check(lib().dn_seg_window_pool_fwd_f32(
            B, N, D, mem_len, mode, ptr(ptr_), ptr(skip), ptr(rows), ptr(mem), ptr(mask.view(torch.uint8)), ptr(arg), ptr(span),
            stream_ptr()), "dn_seg_window_pool_fwd_f32"))
        ctx.args = (B, N, D, mem_len, mode, skip, arg)
        ctx.save_for_backward(ptr_, span)
        ctx.mark_non_differentiable(mask)
        return mem, mask

    @staticmethod
    def backward(ctx, dmem, _dmask):
        ptr_, span = ctx.saved_tensors
        B, N, D, mem_len, mode, skip, arg = ctx.args
        dmem = dmem.contiguous()
        drows = torch.empty((N, D), dtype=torch.float32, device=dmem.device)
        launch_tagged("seg_window_pool_bwd", lambda: check(lib().dn_seg_window_pool_bwd_f32(
            B, N, D, mem_len, mode, ptr(ptr_), ptr(skip), ptr(span), ptr(arg), ptr(dmem), ptr(drows), stream_ptr()),
            "dn_seg_window_pool_bwd_f32"))
        return drows, None, None, None, None


def seg_window_pool_composed(rows, ptr_, skip, mem_len, mode, max_len=None):
    """The same memory from attn_pred.init_mem on the padded rows, one group per distinct span (any dtype, any device)."""
    from .subgraph_isomorphism.attn_pred import init_mem
    from .subgraph_isomorphism.dl import batch_convert_mask_to_start_and_end
    N, D = rows.shape
    B = ptr_.numel() - 1
    L = int(max_len) if max_len is not None else _max_len(ptr_)
    idx, valid = _pad_index(ptr_, max(L, 1), N)
    if skip is not None:
        valid = valid & ~skip.reshape(-1).bool()[idx]
    x = rows[idx].masked_fill(~valid.unsqueeze(-1), 0)
    start, end = batch_convert_mask_to_start_and_end(valid)
    uniq, inv = torch.unique(torch.stack([start, end + 1], dim=1), dim=0, return_inverse=True)
    mem = rows.new_zeros((B, mem_len, D))
    mask = torch.zeros((B, mem_len), dtype=torch.bool, device=rows.device)
    for i, (s, e) in enumerate(uniq.tolist()):
        sel = torch.nonzero(inv == i).view(-1)
        m, mk = init_mem(x[sel, s:e], valid[sel, s:e], mem_len, mode)
        mem = mem.index_copy(0, sel, m)
        mask = mask.index_copy(0, sel, mk.bool())
    return mem.reshape(B * mem_len, D), mask


def seg_window_pool(rows, ptr_, skip, mem_len, mode, max_len=None):
    """DIAMNet's initial memory of every segment of rows [N, D] (ptr_ [B + 1] int32): (mem [B mem_len, D], mem_mask [B, mem_len] bool).
    Per segment the rows from the first to the last with skip == 0 (L rows; skipped rows inside count as zero rows): L <= mem_len gives
    those rows behind mem_len - L zero rows, else the mean | sum | max of the mem_len windows of L - (mem_len - 1) stride rows every
    stride = L // mem_len rows.  mem_mask: the window holds an unskipped row."""
    if mode not in SEG_POOL_MODES:
        raise NotImplementedError("seg_window_pool: mode=%s (mean, sum and max are built)" % (mode,))
    mem_len = int(mem_len)
    if rows.dim() != 2 or mem_len < 1:
        raise _lib.DnHipError("seg_window_pool: rows [N, D] and mem_len >= 1 expected")
    if (attn_fused_enabled() and rows.is_cuda and rows.dtype == torch.float32 and rows.shape[0] and rows.shape[1]
            and mem_len <= SEG_POOL_MAX_MEM and ptr_.numel() > 1):
        return _SegWindowPoolFn.apply(rows, ptr_, _u8_or_none(skip), mem_len, SEG_POOL_MODES[mode])
    return seg_window_pool_composed(rows, ptr_, skip, mem_len, mode, max_len)


# ----------------------------------------------------------------------------------------------
# DiffPool on ragged rows: per-graph products and the fused assignment (dn_diffpool.hip)
# ----------------------------------------------------------------------------------------------
DIFFPOOL_MAX_C = 256
DIFFPOOL_MAX_F = 512

# The default of diffpool_assign.  Measured on the config-2 and config-4 batches (docs/LAB_NOTES.md "GC: DiffPool"; 512 dummy-augmented
# graphs, the reference's default dimensions, fused and composed alternated in one process): the assignment forward + backward 0.91
# against 4.95 ms (config 2: 55 clusters) and 0.34 against 1.17 ms (config 4: 17 clusters), the model's training step 6.90 against
# 10.57 ms and 6.54 against 7.03 ms, every fused round faster than every composed round -- the rule of the attention heads
# (ATTN_FUSED_DEFAULT), so the fused kernels are the default.
DIFFPOOL_FUSED_DEFAULT = True


def diffpool_fused_enabled():
    return diffpool_fused.override(DIFFPOOL_FUSED_DEFAULT)


class diffpool_fused(_ThreadSwitch):
    """Context manager: diffpool_assign calls made inside it (on this thread) run on dn_diffpool.hip (on=True) where
    diffpool_fused_supported allows it, or on the composed path (on=False: the same ragged mathematics in torch ops)."""
    _slot = "diffpool_fused"


def diffpool_fused_supported(logits, z):
    """The predicate of the fused assignment: fp32 rows on the GPU, 1 <= C <= 256 cluster columns, 1 <= F <= 512 feature columns."""
    return (logits.is_cuda and z.is_cuda and logits.dtype == torch.float32 and z.dtype == torch.float32 and logits.dim() == 2
            and z.dim() == 2 and 1 <= int(logits.shape[1]) <= DIFFPOOL_MAX_C and 1 <= int(z.shape[1]) <= DIFFPOOL_MAX_F)


def diffpool_graph_rows(C):
    """The most rows of a graph that one workgroup of dn_diffpool_assign_graphs_f32 takes whole at C cluster columns."""
    return int(lib().dn_diffpool_graph_rows(int(C)))


class DiffPoolIndex:
    """What the DiffPool level on ragged rows needs of a batch, built once per batch (graph.diffpool_index_of caches it there):
    the graph boundaries (int32 on the device AND as host integers -- ONE read-back of its own, which also verifies that every edge
    names rows of the batch and stays inside its graph), the graph of every row, the edges, 1 / max(out-degree, 1), on the GPU the
    batch's EdgeIndex and its transpose (the SAME six tensors and the same two hub splits with the roles of source and destination
    exchanged, nothing rebuilt or read back: DenseSAGEConv aggregates over OUT-edges), the 64-row tile
    table of the per-graph products' backward, and per cluster count the graphs one workgroup takes whole."""

    def __init__(self, src, dst, graph_ptr, num_nodes, edge_index=None):
        dev = graph_ptr.device
        self.num_nodes, self.num_graphs = int(num_nodes), int(graph_ptr.numel() - 1)
        self.src, self.dst = src.long(), dst.long()
        p = graph_ptr.long()
        sizes = p[1:] - p[:-1]
        self.batch = torch.repeat_interleave(torch.arange(self.num_graphs, device=dev), sizes, output_size=self.num_nodes)
        inside = in_range = torch.ones((), dtype=torch.bool, device=dev)
        if self.src.numel() and self.num_nodes:
            hi = self.num_nodes - 1                                               # (checked before anything is indexed by an edge id)
            in_range = ((self.src >= 0) & (self.src <= hi) & (self.dst >= 0) & (self.dst <= hi)).all()
            inside = (self.batch[self.src.clamp(0, hi)] == self.batch[self.dst.clamp(0, hi)]).all()
        elif self.src.numel():
            in_range = ~in_range
        host = torch.cat([p, in_range.view(1).long(), inside.view(1).long()]).tolist()      # the one read-back
        if not host[-2]:
            raise _lib.DnHipError("DiffPool: an edge names a node outside the batch's %d rows" % self.num_nodes)
        if not host[-1]:
            raise _lib.DnHipError("DiffPool: an edge joins two graphs of the batch")
        host = host[:-2]
        if host[0] != 0 or host[-1] != self.num_nodes or any(b < a for a, b in zip(host[:-1], host[1:])):
            raise _lib.DnHipError("DiffPool: the graph boundaries must rise from 0 to the number of rows")
        self.ptr_host = host
        self.sizes = [b - a for a, b in zip(self.ptr_host[:-1], self.ptr_host[1:])]
        self.max_nodes = max(self.sizes) if self.sizes else 0
        self.graph_ptr = graph_ptr.to(I32).contiguous()
        self.out_deg = torch.bincount(self.src, minlength=self.num_nodes).clamp(min=1).view(-1, 1)
        self._inv_out_deg = {}
        self.edge = edge_index
        self._edge_t = self._tiles = self._adj_sq = None
        self._whole = {}

    def inv_out_deg(self, dtype):
        """1 / max(out-degree, 1) as an [N, 1] column of dtype."""
        hit = self._inv_out_deg.get(dtype)
        if hit is None:
            hit = self._inv_out_deg[dtype] = 1.0 / self.out_deg.to(dtype)
        return hit

    @property
    def padded_rows(self):
        """B Nmax: the rows of the reference's padded batch."""
        return self.num_graphs * self.max_nodes

    @property
    def edge_t(self):
        """The batch's EdgeIndex read the other way round: its CSR by destination IS this batch's CSR by source."""
        if self._edge_t is None:
            e = self.edge
            self._edge_t = EdgeIndex.from_parts(e.dst, e.src, e.num_nodes, None, e.out_ptr, e.out_perm, e.dst_by_src, e.in_ptr, e.in_perm,
                                                e.src_by_dst, splits=(e.bwd, e.fwd))
        return self._edge_t

    @property
    def tiles(self):
        if self._tiles is None:
            self._tiles = build_row_tables(self.graph_ptr, self.num_graphs, self.num_nodes, 64)
        return self._tiles

    def whole_graphs(self, C):
        """(graphs taken whole [n] int32 or None, their largest row count, the other graphs [m] int32 or None) at C clusters."""
        hit = self._whole.get(C)
        if hit is None:
            cap = diffpool_graph_rows(C)
            small = [g for g, n in enumerate(self.sizes) if n <= cap]
            big = [g for g, n in enumerate(self.sizes) if n > cap]
            dev = self.graph_ptr.device
            hit = (torch.tensor(small, dtype=I32, device=dev) if small else None, max([self.sizes[g] for g in small], default=0),
                   torch.tensor(big, dtype=I32, device=dev) if big else None)
            self._whole[C] = hit
        return hit

    def adj_sq_norm(self):
        """||A||_F^2 of the dense adjacency: the squares of the multiplicities of the distinct (source, destination) pairs."""
        if self._adj_sq is None:
            _, cnt = torch.unique(self.src * self.num_nodes + self.dst, return_counts=True)
            self._adj_sq = (cnt.double() ** 2).sum()
        return self._adj_sq


def _segment_gram_launch(L, R, graph_ptr, out, graphs=None):
    B, (N, CL), CR = graph_ptr.numel() - 1, L.shape, R.shape[1]
    launch_tagged("segment_gram", lambda: check(lib().dn_segment_gram_f32(
        B, N, CL, CR, ptr(graphs), 0 if graphs is None else graphs.numel(), ptr(graph_ptr), ptr(L), ptr(R), ptr(out), stream_ptr()),
        "dn_segment_gram_f32"))
    return out


class _SegmentGramFn(torch.autograd.Function):
    """out [B, CL, CR] of dn_segment_gram_f32; backward: every row times its own graph's matrix, two dn_rows_gemm_f32 launches over the
    64-row tiles of the graphs (as _TypedLinearFn with the graph as the type; the rows are already grouped)."""

    @staticmethod
    def forward(ctx, L, R, graph_ptr, tiles):
        L, R = L.contiguous(), R.contiguous()
        require_gpu(L, R, graph_ptr)
        _i32(graph_ptr, "graph_ptr")
        B = graph_ptr.numel() - 1
        out = torch.empty((B, L.shape[1], R.shape[1]), dtype=torch.float32, device=L.device)
        if L.shape[0]:
            _segment_gram_launch(L, R, graph_ptr, out)
        else:
            out.zero_()
        ctx.tiles = tiles
        ctx.save_for_backward(L, R, graph_ptr)
        return out

    @staticmethod
    def backward(ctx, dout):
        L, R, graph_ptr = ctx.saved_tensors
        dout = dout.contiguous()
        tiles = ctx.tiles if ctx.tiles is not None else build_row_tables(graph_ptr, graph_ptr.numel() - 1, L.shape[0], 64)
        dL = rows_gemm(R, dout, tiles, transpose_w=True) if ctx.needs_input_grad[0] else None        # R[p] dout[g]^T
        dR = rows_gemm(L, dout, tiles) if ctx.needs_input_grad[1] else None                          # L[p] dout[g]
        return dL, dR, None, None


def _graph_of_rows(graph_ptr, num_rows):
    p = graph_ptr.long()
    return torch.repeat_interleave(torch.arange(p.numel() - 1, device=p.device), p[1:] - p[:-1], output_size=int(num_rows))


def segment_gram_composed(L, R, graph_ptr, batch=None):
    """The same per-graph products from torch ops on the ragged rows (any dtype, any device): the rows' outer products added into
    their graph's matrix, a slab of rows at a time so that no temporary passes 2^24 elements."""
    N, CL = L.shape
    CR, B = R.shape[1], graph_ptr.numel() - 1
    if batch is None:
        batch = _graph_of_rows(graph_ptr, N)
    out = L.new_zeros((B, CL, CR))
    step = max(1, (1 << 24) // max(CL * CR, 1))
    for a in range(0, N, step):
        out.index_add_(0, batch[a:a + step], L[a:a + step].unsqueeze(2) * R[a:a + step].unsqueeze(1))
    return out


def segment_gram(L, R, graph_ptr, tiles=None):
    """out [B, CL, CR]: out[g] = L[rows of graph g]^T R[rows of graph g], the rows of graph g = graph_ptr[g] .. graph_ptr[g + 1]
    (graph_ptr [B + 1] int32).  fp32 on the GPU with CL <= 256 and CR <= 512: dn_segment_gram_f32 (exact-f32 MFMA, the same bits on
    every run; autograd to L and R); anything else: segment_gram_composed.  tiles: the graphs' 64-row tile table when the caller has it."""
    if L.dim() != 2 or R.dim() != 2 or L.shape[0] != R.shape[0] or graph_ptr.numel() < 2:
        raise _lib.DnHipError("segment_gram: L [N, CL], R [N, CR] and graph_ptr [B + 1] with B >= 1 expected")
    if (L.is_cuda and R.is_cuda and L.dtype == R.dtype == torch.float32 and 1 <= L.shape[1] <= DIFFPOOL_MAX_C
            and 1 <= R.shape[1] <= DIFFPOOL_MAX_F):
        return _SegmentGramFn.apply(L, R, graph_ptr, tiles)
    return segment_gram_composed(L, R, graph_ptr)


class _DiffPoolAssignFn(torch.autograd.Function):
    """(X' [B, C, F], A' [B, C, C]) of the fused assignment.  Forward: the graphs whose S fits in LDS in ONE launch
    (dn_diffpool_assign_graphs_f32); the others through a softmax launch, the gather over the CSR by source and dn_segment_gram_f32
    restricted to them.  Saved: logits' softmax S and A S ([N, C] each).  Backward on the ragged rows:
    dS = z dX'^T + (A S) dA'^T + A^T (S dA'), dz = S dX', dlogits = S (dS - rowsum(dS S)) -- four dn_rows_gemm_f32 launches over the graphs'
    tiles, the gather over the CSR by destination and dn_diffpool_softmax_bwd_f32, which adds the three terms as it reads them."""

    @staticmethod
    def forward(ctx, logits, z, index):
        logits, z = logits.contiguous(), z.contiguous()
        require_gpu(logits, z, index.graph_ptr)
        (N, C), F_ = logits.shape, z.shape[1]
        B, e = index.num_graphs, index.edge
        if z.shape[0] != N or index.num_nodes != N:
            raise _lib.DnHipError("diffpool_assign: logits [N, C], z [N, F] and the batch's N rows expected")
        dev = logits.device
        S = torch.empty_like(logits)
        X = torch.empty((B, C, F_), dtype=torch.float32, device=dev)
        A = torch.empty((B, C, C), dtype=torch.float32, device=dev)
        small, max_rows, big = index.whole_graphs(C)
        if N == 0:
            X.zero_(), A.zero_()
        AS = torch.empty_like(logits) if big is None or not N else None
        if big is not None and N:
            # The softmax and the gather run over ALL rows although only the listed graphs' rows are used (the whole-graph launch below
            # writes the others again, the same S bit for bit).  Restricting them needs a second CSR per (batch, C) over the listed
            # graphs' rows -- exactly the graphs with a hub row, so with its own hub split -- to save two passes over [N, C] (config 2:
            # 4.4 MB each, a few microseconds of the 0.9 ms); the products, which dominate, ARE restricted to the list.
            launch_tagged("diffpool_softmax", lambda: check(lib().dn_diffpool_softmax_fwd_f32(N, C, ptr(logits), ptr(S), stream_ptr()),
                                                           "dn_diffpool_softmax_fwd_f32"))
            AS = e.bwd.segsum(S)                                                  # row i: the S rows of its out-edges' destinations
            _segment_gram_launch(S, z, index.graph_ptr, X, big)
            _segment_gram_launch(S, AS, index.graph_ptr, A, big)
        if small is not None and N:
            launch_tagged("diffpool_assign_graphs", lambda: check(lib().dn_diffpool_assign_graphs_f32(
                B, N, e.num_edges, small.numel(), max_rows, C, F_, ptr(small), ptr(index.graph_ptr), ptr(e.out_ptr), ptr(e.dst_by_src),
                ptr(logits), ptr(z), ptr(S), ptr(AS), ptr(X), ptr(A), stream_ptr()), "dn_diffpool_assign_graphs_f32"))
        ctx.index = index
        ctx.save_for_backward(z, S, AS)
        return X, A

    @staticmethod
    def backward(ctx, dX, dA):
        z, S, AS = ctx.saved_tensors
        index = ctx.index
        N, C = S.shape
        dX, dA = dX.contiguous(), dA.contiguous()
        if N == 0:
            return torch.zeros_like(S), torch.zeros_like(z), None
        tiles = index.tiles
        dz = rows_gemm(S, dX, tiles) if ctx.needs_input_grad[1] else None
        dlogits = None
        if ctx.needs_input_grad[0]:
            d0 = rows_gemm(z, dX, tiles, transpose_w=True)                         # z dX'^T
            d1 = rows_gemm(AS, dA, tiles, transpose_w=True)                        # (A S) dA'^T
            d2 = index.edge.fwd.segsum(rows_gemm(S, dA, tiles))                    # A^T (S dA'): row j gathers over its in-edges' sources
            dlogits = torch.empty_like(S)
            launch_tagged("diffpool_softmax_bwd", lambda: check(lib().dn_diffpool_softmax_bwd_f32(
                N, C, ptr(S), ptr(d0), ptr(d1), ptr(d2), ptr(dlogits), stream_ptr()), "dn_diffpool_softmax_bwd_f32"))
        return dlogits, dz, None


def diffpool_assign_composed(logits, z, index):
    """The same two products from torch ops on the ragged rows (any dtype, any device): softmax, index_add over the edges,
    segment_gram_composed."""
    S = torch.softmax(logits, dim=-1)
    AS = torch.zeros_like(S).index_add(0, index.src, S.index_select(0, index.dst))
    return segment_gram_composed(S, z, index.graph_ptr, index.batch), segment_gram_composed(S, AS, index.graph_ptr, index.batch)


def diffpool_assign(logits, z, index):
    """(X' [B, C, F], A' [B, C, C]) of dense_diff_pool on ragged rows: S = softmax(logits [N, C]) over the clusters, per graph
    X' = S^T z (z [N, F]) and A' = S^T (A S), A the graph's adjacency with edge (src, dst) at A[src, dst] and duplicates summed.
    index: the batch's DiffPoolIndex.  The fused kernels where diffpool_fused_enabled() and diffpool_fused_supported (fp32,
    C <= 256, F <= 512), else the composed path.  Autograd to logits and z either way."""
    if diffpool_fused_enabled() and diffpool_fused_supported(logits, z) and index.edge is not None:
        return _DiffPoolAssignFn.apply(logits, z, index)
    return diffpool_assign_composed(logits, z, index)


# ----------------------------------------------------------------------------------------------
# HGP-SL pooling on ragged per-graph blocks (dn_hgpsl.hip)
# ----------------------------------------------------------------------------------------------
HGPSL_MAX_H = 512
HGPSL_WAVE_KEYS = 64
HGPSL_MAX_KEYS = 1024
HGPSL_TOPK_MAX_NODES = 4096
HGPSL_ATT_SLABS = 64

# The default of the HGP-SL ops, by the rule of ATTN_FUSED_DEFAULT / DIFFPOOL_FUSED_DEFAULT: on only if every fused round beats every
# composed round.  Measured with tools/gc_hgpsl_bench.py on the config-2 and config-4 batches (docs/LAB_NOTES.md "GC: HGP-SL"; 512
# dummy-augmented graphs, H = 128, ratio 0.8, fused and composed alternated in one process), softmax / sparsemax: score + top-k 0.21
# against 0.48 / 0.46 ms (config 2) and 0.09 against 0.38 / 0.37 ms (config 4); structure forward + backward 0.26 / 0.26 against
# 23.5 / 34.0 ms and 0.25 / 0.16 against 12.9 / 15.5 ms; the two-level stack's training step 6.74 / 4.91 against 63.0 / 62.8 ms and
# 4.31 / 3.84 against 28.0 / 34.7 ms -- every fused round faster than every composed round in all twelve, so the kernels are the default.
HGPSL_FUSED_DEFAULT = True


def hgpsl_fused_enabled():
    return hgpsl_fused.override(HGPSL_FUSED_DEFAULT)


class hgpsl_fused(_ThreadSwitch):
    """Context manager: hgpsl_score / hgpsl_topk / hgpsl_structure calls made inside it (on this thread) run on dn_hgpsl.hip (on=True)
    where hgpsl_fused_supported allows it, or on the composed path (on=False: the same ragged mathematics in torch ops)."""
    _slot = "hgpsl_fused"


def hgpsl_fused_supported(x):
    """The predicate of the fused HGP-SL kernels: fp32 rows on the GPU with 1 <= H <= 512 feature columns."""
    return x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and 1 <= int(x.shape[1]) <= HGPSL_MAX_H


def hgpsl_k(ratio, sizes):
    """The kept nodes per graph, ceil(float32(ratio) float32(n)) in float32 exactly as torch computes (ratio * n.float()).ceil():
    0.3 x 50 -> 16, not 15.  Host integers in, host integers out."""
    if not sizes:
        return []
    k = (ratio * torch.tensor(sizes, dtype=torch.float32)).ceil().long().tolist()
    return [min(int(a), int(n)) for a, n in zip(k, sizes)]


def _dev_i32(values, device):
    return torch.from_numpy(_np.asarray(values, dtype=_np.int32)).to(device)


class HgpslPooled:
    """The sizes of a batch after one HGP-SL pooling at `ratio`, all from the host copy of the graph sizes (no read-back): k per
    graph, the pooled graph boundaries, the offsets of the ragged k x k blocks, and the class lists of the kernels."""

    def __init__(self, index, ratio):
        dev = index.graph_ptr.device
        self.ratio = ratio
        self.ks = hgpsl_k(ratio, index.sizes)
        ks = _np.asarray(self.ks, dtype=_np.int64).reshape(-1)
        ns = _np.asarray(index.sizes, dtype=_np.int64).reshape(-1)
        self.ptr_host = [0] + _np.cumsum(ks).tolist()
        self.blk_host = [0] + _np.cumsum(ks * ks).tolist()
        self.num_rows, self.num_pairs, self.num_graphs = self.ptr_host[-1], self.blk_host[-1], len(self.ks)
        self.graph_ptr = _dev_i32(self.ptr_host, dev)
        self.blk_ptr = torch.from_numpy(_np.asarray(self.blk_host, dtype=_np.int64)).to(dev)
        self.max_k = int(ks.max()) if ks.size else 0
        # top-k classes by the graph's size, structure classes by its kept size
        gid = _np.arange(ks.size)
        self.topk_lists = []                                                  # (graphs int32 on the device, their largest size)
        self.topk_big = gid[ns > HGPSL_TOPK_MAX_NODES].tolist()
        self.rows_wave = self.rows_block = self.rows_fused = None
        self.max_wave = self.max_block = 0
        self.big = gid[ks > HGPSL_MAX_KEYS].tolist()
        if dev.type == "cuda":
            for m in ((ns >= 1) & (ns <= HGPSL_WAVE_KEYS), (ns > HGPSL_WAVE_KEYS) & (ns <= HGPSL_TOPK_MAX_NODES)):
                if m.any():
                    self.topk_lists.append((_dev_i32(gid[m], dev), int(ns[m].max())))
            krow = _np.repeat(ks, ks)
            rows = _np.arange(self.num_rows)
            wave, block = krow <= HGPSL_WAVE_KEYS, (krow > HGPSL_WAVE_KEYS) & (krow <= HGPSL_MAX_KEYS)
            if wave.any():
                self.rows_wave, self.max_wave = _dev_i32(rows[wave], dev), int(krow[wave].max())
            if block.any():
                self.rows_block, self.max_block = _dev_i32(rows[block], dev), int(krow[block].max())
            if wave.any() or block.any():
                self.rows_fused = _dev_i32(rows[wave | block], dev)
        self._groups = {}

    def groups(self, graphs=None):
        """[(k, graphs of that k as a host list)] for k >= 1, over all graphs or the listed ones."""
        key = None if graphs is None else tuple(graphs)
        hit = self._groups.get(key)
        if hit is None:
            by_k = {}
            for g in (range(self.num_graphs) if graphs is None else graphs):
                if self.ks[g] >= 1:
                    by_k.setdefault(self.ks[g], []).append(g)
            hit = self._groups[key] = sorted(by_k.items())
        return hit

    def group_chunks(self, graphs=None):
        """[(k, first pooled rows [G], block offsets [G])] on the device: the groups cut into chunks of at most HGPSL_COMPOSED_CHUNK
        elements of a dense [G, k, k] tensor.  Cached: a second call copies nothing to the device."""
        key = ("chunks", None if graphs is None else tuple(graphs))
        hit = self._groups.get(key)
        if hit is None:
            hit, dev = [], self.graph_ptr.device
            for k, gs in self.groups(graphs):
                step = max(1, HGPSL_COMPOSED_CHUNK // (k * k))
                for s in range(0, len(gs), step):
                    part = gs[s:s + step]
                    hit.append((k, torch.tensor([self.ptr_host[g] for g in part], device=dev),
                                torch.tensor([self.blk_host[g] for g in part], device=dev)))
            self._groups[key] = hit
        return hit


class HgpslIndex:
    """What HGPSLPool needs of a batch, built once per batch (graph.hgpsl_index_of caches it on the data object): the graph boundaries
    (int32 on the device AND as host integers), the graph of every row, the edges, on the GPU their CSR by destination (col) and by
    source (row), and the checks of the layer's precondition -- every edge names rows of the batch, no edge joins two graphs, no
    (row, col) pair is repeated -- all in ONE read-back.  sizes: the host sizes when the caller already has them AND the edges are
    the layer's own output (unique and inside their graphs by construction): then nothing is read back at all."""

    def __init__(self, row, col, graph_ptr, num_nodes, sizes=None):
        dev = graph_ptr.device
        self.num_nodes, self.num_graphs = int(num_nodes), int(graph_ptr.numel() - 1)
        self.row, self.col = row.long(), col.long()
        self.num_edges = int(self.row.numel())
        if sizes is None:
            p = graph_ptr.long()
            ok = torch.ones(3, dtype=torch.long, device=dev)
            if self.num_edges and self.num_nodes:
                hi = self.num_nodes - 1
                in_range = ((self.row >= 0) & (self.row <= hi) & (self.col >= 0) & (self.col <= hi)).all()
                r, c = self.row.clamp(0, hi), self.col.clamp(0, hi)
                b = torch.searchsorted(p[1:].contiguous(), r, right=True)
                inside = (b == torch.searchsorted(p[1:].contiguous(), c, right=True)).all()
                key = torch.sort(r * self.num_nodes + c).values
                unique = ~(key[1:] == key[:-1]).any()
                ok = torch.stack([in_range, inside, unique]).long()
            elif self.num_edges:
                ok[0] = 0
            host = torch.cat([p, ok]).tolist()                                    # the one read-back
            flags, host = host[-3:], host[:-3]
            if not flags[0]:
                raise _lib.DnHipError("HGP-SL: an edge names a node outside the batch's %d rows" % self.num_nodes)
            if not flags[1]:
                raise _lib.DnHipError("HGP-SL: an edge joins two graphs of the batch")
            if not flags[2]:
                raise _lib.DnHipError("HGP-SL: a (row, col) pair is repeated (coalesce the edges first)")
            if host[0] != 0 or host[-1] != self.num_nodes or any(b < a for a, b in zip(host[:-1], host[1:])):
                raise _lib.DnHipError("HGP-SL: the graph boundaries must rise from 0 to the number of rows")
            sizes = [b - a for a, b in zip(host[:-1], host[1:])]
        self.sizes = [int(s) for s in sizes]
        self.ptr_host = [0] + _np.cumsum(_np.asarray(self.sizes, dtype=_np.int64)).tolist() if self.sizes else [0]
        self.graph_ptr = graph_ptr.to(I32).contiguous()
        self.batch = torch.repeat_interleave(torch.arange(self.num_graphs, device=dev), graph_ptr.long()[1:] - graph_ptr.long()[:-1],
                                             output_size=self.num_nodes)
        self._pooled = {}
        self.row32 = self.col32 = self.in_ptr = self.in_perm = self.src_by_dst = self.out_ptr = self.out_perm = self.dst_by_src = None
        if dev.type == "cuda" and self.num_nodes:
            self.row32, self.col32 = self.row.to(I32).contiguous(), self.col.to(I32).contiguous()
            if self.num_edges:
                self.in_ptr, self.in_perm = csr_build(self.col32, self.num_nodes)
                self.out_ptr, self.out_perm = csr_build(self.row32, self.num_nodes)
            else:
                self.in_ptr = self.out_ptr = torch.zeros(self.num_nodes + 1, dtype=I32, device=dev)
                self.in_perm = self.out_perm = torch.zeros(0, dtype=I32, device=dev)
            self.src_by_dst = gather_rows_i32(self.row32, self.in_perm)
            self.dst_by_src = gather_rows_i32(self.col32, self.out_perm)

    @classmethod
    def from_batch(cls, edge_index, batch, num_nodes):
        """From PyG's (edge_index, batch) when no graph boundaries are at hand: the number of graphs costs a read-back of its own."""
        if batch is None:
            batch = edge_index.new_zeros(num_nodes)
        ng = int(batch.max().item()) + 1 if batch.numel() else 1
        cnt = torch.bincount(batch, minlength=ng)
        p = torch.cat([cnt.new_zeros(1), torch.cumsum(cnt, 0)])
        return cls(edge_index[0], edge_index[1], p, num_nodes)

    def pooled(self, ratio):
        """The HgpslPooled of this batch at `ratio` (cached): the next level's sizes on the host, no read-back."""
        hit = self._pooled.get(ratio)
        if hit is None:
            hit = self._pooled[ratio] = HgpslPooled(self, ratio)
        return hit


def _hgpsl_weights(index, edge_attr, like):
    if edge_attr is None:
        return None
    if edge_attr.dim() != 1 or edge_attr.numel() != index.num_edges:
        raise _lib.DnHipError("HGP-SL: edge_attr must hold one weight per edge ([%d], got %s)" % (index.num_edges, tuple(edge_attr.shape)))
    return edge_attr.to(like.dtype)


def hgpsl_score_composed(x, index, edge_attr=None):
    """The node information score from torch ops (any dtype, any device)."""
    x = x.detach()
    w = _hgpsl_weights(index, edge_attr, x)
    w = x.new_ones(index.num_edges) if w is None else w.detach()
    deg = x.new_zeros(index.num_nodes).index_add_(0, index.row, w)
    dinv = deg.pow(-0.5)
    dinv[dinv == float("inf")] = 0
    coef = dinv[index.row] * w * dinv[index.col]
    agg = torch.zeros_like(x).index_add_(0, index.col, coef.view(-1, 1) * x.index_select(0, index.row))
    return (x - agg).abs().sum(dim=1)


def hgpsl_score(x, index, edge_attr=None):
    """score [N] = || ((I - D^-1/2 A D^-1/2) x)_i ||_1 with the degree taken over the edges' rows (NodeInformationScore of the
    reference); no gradient.  Fused: one small launch for D^-1/2 and ONE launch for the weighted gather fused with the row sum."""
    if x.dim() != 2 or x.shape[0] != index.num_nodes:
        raise _lib.DnHipError("hgpsl_score: x [N, H] with the batch's N = %d rows expected" % index.num_nodes)
    if not (hgpsl_fused_enabled() and hgpsl_fused_supported(x)) or index.num_nodes == 0:
        return hgpsl_score_composed(x, index, edge_attr)
    x = x.detach().contiguous()
    w = _hgpsl_weights(index, edge_attr, x)
    w = None if w is None else w.detach().contiguous()
    require_gpu(x, w, index.in_ptr)
    N, E, H = index.num_nodes, index.num_edges, x.shape[1]
    dinv = torch.empty(N, dtype=torch.float32, device=x.device)
    score = torch.empty(N, dtype=torch.float32, device=x.device)
    launch_tagged("hgpsl_dinv", lambda: check(lib().dn_hgpsl_dinv_f32(N, E, ptr(index.out_ptr), ptr(index.out_perm), ptr(w), ptr(dinv),
                                                                     stream_ptr()), "dn_hgpsl_dinv_f32"))
    launch_tagged("hgpsl_score", lambda: check(lib().dn_hgpsl_score_f32(N, E, H, ptr(index.in_ptr), ptr(index.in_perm), ptr(index.src_by_dst),
                                                                       ptr(w), ptr(dinv), ptr(x), ptr(score), stream_ptr()),
                                               "dn_hgpsl_score_f32"))
    return score


class HgpslSelection:
    """The kept nodes of one pooling: perm [N'] (each graph's kept nodes by descending score, ties to the lower node), batch [N'] and
    inv [N] (the pooled row of a kept node, -1 of a dropped one); int64 for indexing, int32 for the kernels."""

    def __init__(self, perm, batch, inv):
        self.perm32, self.batch32, self.inv32 = perm, batch, inv
        self.perm, self.batch, self.inv = perm.long(), batch.long(), inv.long()


def _hgpsl_topk_torch(score, index, pooled, graphs, perm, batch, inv):
    """The selection of the listed graphs (None: all) from two stable sorts, written into perm / batch / inv (int32)."""
    dev = score.device
    if graphs is None:
        nodes, gb = torch.arange(index.num_nodes, device=dev), index.batch
    else:
        ranges = [_np.arange(index.ptr_host[g], index.ptr_host[g + 1]) for g in graphs]
        nodes = torch.from_numpy(_np.concatenate(ranges) if ranges else _np.zeros(0, dtype=_np.int64)).to(dev)
        gb = index.batch.index_select(0, nodes)
    if nodes.numel() == 0:
        return
    o1 = torch.sort(score.index_select(0, nodes), descending=True, stable=True).indices       # ties keep the lower node first
    o2 = torch.sort(gb.index_select(0, o1), stable=True).indices
    order = nodes.index_select(0, o1.index_select(0, o2))                                      # by graph, then by descending score
    g_of = index.batch.index_select(0, order)
    gptr, pptr = index.graph_ptr.long(), pooled.graph_ptr.long()
    # `order` lists the chosen graphs' nodes graph by graph: the rank of an entry is its distance from its graph's first entry
    sizes = gptr[1:] - gptr[:-1]
    if graphs is not None:
        chosen = torch.as_tensor(list(graphs), device=dev)
        sizes = torch.zeros_like(sizes).index_copy_(0, chosen, sizes.index_select(0, chosen))
    start = torch.cumsum(sizes, 0) - sizes
    rank = torch.arange(order.numel(), device=dev) - start.index_select(0, g_of)
    keep = rank < (pptr[1:] - pptr[:-1]).index_select(0, g_of)
    slot = pptr.index_select(0, g_of) + rank
    inv.index_copy_(0, order, torch.where(keep, slot, torch.full_like(slot, -1)).to(I32))
    tgt = torch.where(keep, slot, torch.full_like(slot, pooled.num_rows))                      # dropped entries land in a spare slot
    perm_x, batch_x = torch.cat([perm, perm.new_zeros(1)]), torch.cat([batch, batch.new_zeros(1)])
    perm_x.scatter_(0, tgt, order.to(I32))
    batch_x.scatter_(0, tgt, g_of.to(I32))
    perm.copy_(perm_x[:-1])
    batch.copy_(batch_x[:-1])


def hgpsl_topk(score, index, pooled):
    """HgpslSelection of the pooling: per graph the k = pooled.ks[g] nodes of the highest scores.  Fused: the u64 keys
    (~score bits << 32) | local index sorted per graph by a wavefront (<= 64 nodes) or a workgroup in LDS (<= 4096 nodes); larger
    graphs, and everything on the composed path, by two stable torch sorts.  No read-back."""
    dev = score.device
    N, Np = index.num_nodes, pooled.num_rows
    perm = torch.zeros(Np, dtype=I32, device=dev)
    batch = torch.zeros(Np, dtype=I32, device=dev)
    inv = torch.full((N,), -1, dtype=I32, device=dev)
    if N == 0 or Np == 0:
        return HgpslSelection(perm, batch, inv)
    fused = hgpsl_fused_enabled() and score.is_cuda and score.dtype == torch.float32
    if not fused:
        _hgpsl_topk_torch(score, index, pooled, None, perm, batch, inv)
        return HgpslSelection(perm, batch, inv)
    score = score.contiguous()
    require_gpu(score, index.graph_ptr, pooled.graph_ptr)
    for graphs, max_nodes in pooled.topk_lists:
        launch_tagged("hgpsl_topk", lambda: check(lib().dn_hgpsl_topk_f32(
            index.num_graphs, N, Np, graphs.numel(), max_nodes, ptr(graphs), ptr(index.graph_ptr), ptr(pooled.graph_ptr), ptr(score),
            ptr(perm), ptr(batch), ptr(inv), stream_ptr()), "dn_hgpsl_topk_f32"))
    if pooled.topk_big:
        _hgpsl_topk_torch(score, index, pooled, pooled.topk_big, perm, batch, inv)
    return HgpslSelection(perm, batch, inv)


def hgpsl_filter(index, sel, edge_attr=None):
    """filter_adj: the edges with both ends kept, renumbered through perm, their order kept (one sync for the count)."""
    r, c = sel.inv.index_select(0, index.row), sel.inv.index_select(0, index.col)
    mask = (r >= 0) & (c >= 0)
    return torch.stack([r[mask], c[mask]]), (None if edge_attr is None else edge_attr[mask])


def _sparsemax_rows(z):
    """sparsemax over the last dimension (Martins & Astudillo 2016, as sparse_softmax.py computes it)."""
    z = z - z.max(dim=-1, keepdim=True).values
    srt = torch.sort(z, dim=-1, descending=True).values
    cs = srt.cumsum(dim=-1) - 1.0
    rho = torch.arange(1, z.shape[-1] + 1, dtype=z.dtype, device=z.device)
    kk = (rho * srt > cs).sum(dim=-1, keepdim=True).clamp(min=1)
    tau = cs.gather(-1, kk - 1) / kk.to(z.dtype)
    return torch.clamp(z - tau, min=0)


def _softmax_rows(z):
    """PyG's grouped softmax on a dense group: the maximum subtracted, 1e-16 added to the sum."""
    e = (z - z.max(dim=-1, keepdim=True).values).exp()
    return e / (e.sum(dim=-1, keepdim=True) + 1e-16)


def _hgpsl_adjacency(index, pooled, sel, w, dtype):
    """lamb-free A as ragged blocks [T + 1] (a spare slot takes the edges with a dropped end): the pairs are unique, so every slot but
    the spare one has at most one writer."""
    r, c = sel.inv.index_select(0, index.row), sel.inv.index_select(0, index.col)
    valid = (r >= 0) & (c >= 0)
    rr, cc = r.clamp(min=0), c.clamp(min=0)
    g = sel.batch.index_select(0, rr) if pooled.num_rows else rr
    c0, kg = pooled.graph_ptr.long().index_select(0, g), (pooled.graph_ptr.long()[1:] - pooled.graph_ptr.long()[:-1]).index_select(0, g)
    pos = pooled.blk_ptr.index_select(0, g) + (rr - c0) * kg + (cc - c0)
    pos = torch.where(valid, pos, torch.full_like(pos, pooled.num_pairs))
    vals = valid.to(dtype) if w is None else w * valid.to(dtype)
    return torch.zeros(pooled.num_pairs + 1, dtype=dtype, device=r.device).index_put((pos,), vals, accumulate=True)


HGPSL_COMPOSED_CHUNK = 1 << 22               # elements of one dense [G, k, k] group of the composed path


def hgpsl_structure_composed(xp, att, edge_attr, index, pooled, sel, sparse=False, lamb=1.0, negative_slop=0.2, graphs=None,
                             positions=False):
    """The ragged blocks [sum k^2] from torch ops (any dtype, any device; autograd to xp, att and edge_attr): the graphs grouped by
    k, each group a dense [G, k, k] chunk -- no Python loop over single graphs, nothing of size N'^2.  graphs: only those (host
    list); the other blocks stay zero.  positions=True: returns (flat positions, values) of the computed blocks instead."""
    H = xp.shape[1]
    a = att.reshape(-1).to(xp.dtype)
    p, q = xp @ a[:H], xp @ a[H:]
    dev = xp.device
    w = _hgpsl_weights(index, edge_attr, xp)
    A = _hgpsl_adjacency(index, pooled, sel, w, xp.dtype) if index.num_edges and pooled.num_rows else None
    pos_all, val_all = [], []
    for k, c0, b0 in pooled.group_chunks(graphs):
        rows = (c0.view(-1, 1) + torch.arange(k, device=dev)).reshape(-1)
        P, Q = p.index_select(0, rows).view(-1, k, 1), q.index_select(0, rows).view(-1, 1, k)
        z = torch.nn.functional.leaky_relu(P + Q, negative_slop)
        bpos = (b0.view(-1, 1) + torch.arange(k * k, device=dev)).reshape(-1)
        if A is not None:
            z = z + A.index_select(0, bpos).view(-1, k, k) * lamb
        o = _sparsemax_rows(z) if sparse else _softmax_rows(z)
        pos_all.append(bpos)
        val_all.append(o.reshape(-1))
    if not pos_all:
        pos_cat, val_cat = torch.zeros(0, dtype=torch.long, device=dev), xp.new_zeros(0)
    else:
        pos_cat, val_cat = torch.cat(pos_all), torch.cat(val_all)
    if positions:
        return pos_cat, val_cat
    return xp.new_zeros(pooled.num_pairs).index_copy(0, pos_cat, val_cat)


class _HgpslStructureFn(torch.autograd.Function):
    """The ragged blocks of the graphs with k <= 1024 (the others' stay zero).  Forward: p, q (one launch), then one launch per
    class (a wavefront or a workgroup per row).  Saved: xp, att, p, q and the blocks themselves -- the output decides the Jacobian
    (softmax: o (g - <o, g>); sparsemax: g - mean over o > 0) and the sign of p_i + q_j the leaky slope, so no logit is kept or
    recomputed.  Backward: the row pass (dl, dp, the row terms), the column pass (dq), the edge pass (lamb dz at each induced edge)
    and the fixed-order reduction for att."""

    @staticmethod
    def forward(ctx, xp, att, w, index, pooled, sel, sparse, lamb, slope):
        ctx.att_shape = att.shape
        xp, att = xp.contiguous(), att.contiguous().view(-1)
        w = None if w is None else w.contiguous()
        require_gpu(xp, att, w, sel.perm32, sel.inv32)
        Np, H = xp.shape
        N, E, B, T = index.num_nodes, index.num_edges, index.num_graphs, pooled.num_pairs
        dev = xp.device
        mode = SEG_SCORES["sparsemax" if sparse else "softmax"]
        p = torch.empty(Np, dtype=torch.float32, device=dev)
        q = torch.empty(Np, dtype=torch.float32, device=dev)
        launch_tagged("hgpsl_pq", lambda: check(lib().dn_hgpsl_pq_f32(Np, H, ptr(xp), ptr(att), ptr(p), ptr(q), stream_ptr()), "dn_hgpsl_pq_f32"))
        blocks = torch.zeros(T, dtype=torch.float32, device=dev) if pooled.big else torch.empty(T, dtype=torch.float32, device=dev)
        for rows, max_keys in ((pooled.rows_wave, pooled.max_wave), (pooled.rows_block, pooled.max_block)):
            if rows is None:
                continue
            launch_tagged("hgpsl_structure_fwd", lambda: check(lib().dn_hgpsl_structure_fwd_f32(
                B, N, E, Np, T, rows.numel(), max_keys, mode, ptr(rows), ptr(pooled.graph_ptr), ptr(pooled.blk_ptr), ptr(sel.batch32),
                ptr(sel.perm32), ptr(sel.inv32), ptr(index.out_ptr), ptr(index.out_perm), ptr(index.dst_by_src), ptr(w), ptr(p), ptr(q),
                lamb, slope, ptr(blocks), stream_ptr()), "dn_hgpsl_structure_fwd_f32"))
        ctx.args = (index, pooled, sel, mode, lamb, slope, w is not None)
        ctx.save_for_backward(xp, att, p, q, blocks)
        return blocks

    @staticmethod
    def backward(ctx, dblocks):
        xp, att, p, q, blocks = ctx.saved_tensors
        index, pooled, sel, mode, lamb, slope, has_w = ctx.args
        Np, H = xp.shape
        N, E, B, T = index.num_nodes, index.num_edges, index.num_graphs, pooled.num_pairs
        dev = xp.device
        dblocks = dblocks.contiguous()
        rows = pooled.rows_fused
        dp = torch.zeros(Np, dtype=torch.float32, device=dev)
        dq = torch.zeros(Np, dtype=torch.float32, device=dev)
        rterm = torch.zeros(Np, dtype=torch.float32, device=dev)
        dl = torch.empty(T, dtype=torch.float32, device=dev)
        dxp = datt = dw = None
        if rows is not None:
            launch_tagged("hgpsl_structure_bwd_rows", lambda: check(lib().dn_hgpsl_structure_bwd_rows_f32(
                B, Np, T, rows.numel(), mode, ptr(rows), ptr(pooled.graph_ptr), ptr(pooled.blk_ptr), ptr(sel.batch32), ptr(p), ptr(q), slope,
                ptr(blocks), ptr(dblocks), ptr(dl), ptr(dp), ptr(rterm), stream_ptr()), "dn_hgpsl_structure_bwd_rows_f32"))
            launch_tagged("hgpsl_structure_bwd_cols", lambda: check(lib().dn_hgpsl_structure_bwd_cols_f32(
                B, Np, T, rows.numel(), ptr(rows), ptr(pooled.graph_ptr), ptr(pooled.blk_ptr), ptr(sel.batch32), ptr(dl), ptr(dq),
                stream_ptr()), "dn_hgpsl_structure_bwd_cols_f32"))
        if has_w and ctx.needs_input_grad[2]:
            dw = torch.zeros(E, dtype=torch.float32, device=dev)
            if E and rows is not None:
                launch_tagged("hgpsl_structure_bwd_edges", lambda: check(lib().dn_hgpsl_structure_bwd_edges_f32(
                    B, N, E, Np, T, mode, ptr(index.row32), ptr(index.col32), ptr(sel.inv32), ptr(pooled.graph_ptr), ptr(pooled.blk_ptr),
                    ptr(sel.batch32), ptr(blocks), ptr(dblocks), ptr(rterm), lamb, ptr(dw), stream_ptr()),
                    "dn_hgpsl_structure_bwd_edges_f32"))
        if ctx.needs_input_grad[0]:
            dxp = torch.addcmul(dp.view(-1, 1) * att[:H].view(1, -1), dq.view(-1, 1), att[H:].view(1, -1))
        if ctx.needs_input_grad[1]:
            datt = torch.empty(2 * H, dtype=torch.float32, device=dev)
            ws = torch.empty(HGPSL_ATT_SLABS * 2 * H, dtype=torch.float32, device=dev)
            launch_tagged("hgpsl_att_grad", lambda: check(lib().dn_hgpsl_att_grad_f32(Np, H, ptr(xp), ptr(dp), ptr(dq), ptr(ws), ptr(datt),
                                                                                     stream_ptr()), "dn_hgpsl_att_grad_f32"))
            datt = datt.view(ctx.att_shape)
        return dxp, datt, dw, None, None, None, None, None, None


def hgpsl_structure(xp, att, edge_attr, index, pooled, sel, sparse=False, lamb=1.0, negative_slop=0.2):
    """The learned structure of the pooled batch as ragged blocks [sum k_g^2]: graph g's k_g x k_g block, row-major, at
    pooled.blk_host[g]; row i holds softmax_j or sparsemax_j of leaky_relu(<xp_i, att_l> + <xp_j, att_r>) + lamb A_ij over the kept
    nodes j of the row's graph.  xp [N', H] = x[perm], att [1, 2 H] (or [2 H]), edge_attr [E] or None (ones).  Autograd to xp, att and
    edge_attr.  The fused kernels where hgpsl_fused_enabled() and hgpsl_fused_supported (fp32, GPU, H <= 512); graphs with more than
    1024 kept nodes take hgpsl_structure_composed on their own, within the same call."""
    if xp.dim() != 2 or xp.shape[0] != pooled.num_rows or att.numel() != 2 * xp.shape[1]:
        raise _lib.DnHipError("hgpsl_structure: xp [N', H] with the pooled batch's N' = %d rows and att [2 H] expected" % pooled.num_rows)
    if not (hgpsl_fused_enabled() and hgpsl_fused_supported(xp) and att.dtype == torch.float32) or pooled.num_rows == 0:
        return hgpsl_structure_composed(xp, att, edge_attr, index, pooled, sel, sparse, lamb, negative_slop)
    w = _hgpsl_weights(index, edge_attr, xp)
    blocks = _HgpslStructureFn.apply(xp, att, w, index, pooled, sel, bool(sparse), float(lamb), float(negative_slop))
    if pooled.big:
        pos, val = hgpsl_structure_composed(xp, att, edge_attr, index, pooled, sel, sparse, lamb, negative_slop, graphs=pooled.big,
                                            positions=True)
        blocks = blocks.index_copy(0, pos, val)
    return blocks


def hgpsl_compact(blocks, pooled):
    """dense_to_sparse on the ragged blocks: (edge_index [2, M] over the pooled rows, weights [M]) of the entries that are not
    exactly zero, in row-major order.  The data-dependent count costs the layer's one unavoidable sync."""
    nz = blocks.detach().nonzero().view(-1)
    g = torch.searchsorted(pooled.blk_ptr[1:].contiguous(), nz, right=True)
    pptr = pooled.graph_ptr.long()
    c0, k = pptr.index_select(0, g), (pptr[1:] - pptr[:-1]).index_select(0, g)
    off = nz - pooled.blk_ptr.index_select(0, g)
    r = torch.div(off, k.clamp(min=1), rounding_mode="floor")
    return torch.stack([c0 + r, c0 + off - r * k]), blocks.index_select(0, nz)


# ----------------------------------------------------------------------------------------------
# The CNN count model on edge sequences: conv -> act -> max pool -> gate (-> residual) per layer, and the label filter (dn_eseq.hip)
# ----------------------------------------------------------------------------------------------
ESEQ_MAX_C = 128
ESEQ_MAX_K = 5
ESEQ_MAX_B = 65535                                               # sequences of a launch (the grid's second dimension)
ESEQ_ACTS = {"none": 0, "relu": 1, "leaky_relu": 2}
ESEQ_LEAKY_SLOPE = 1 / 5.5                                       # the reference's leaky_relu slope (act.LEAKY_RELU_A, constants.py:10)
ESEQ_WGRAD_SLICES = 128                                          # slices of the batch whose weight-gradient partials are kept apart

# The model's default.  Measured on the scale batch (docs/LAB_NOTES.md "SI count models: CNN"; 512 pairs, H = 64, graph sequences of
# 302 tuples, fused and composed alternated in one process, 4 rounds): the layer step 0.52 against 0.97 ms (k = 2) and 0.68 against
# 1.11 ms (k = 3), the model step 5.6 against 8.6 ms and 6.1 against 9.3 ms, every fused round faster than every composed round -- so
# by the project's rule the kernels are the default (as HGT_FUSED_DEFAULT).
ESEQ_FUSED_DEFAULT = True


def eseq_fused_enabled():
    return eseq_fused.override(ESEQ_FUSED_DEFAULT)


class eseq_fused(_ThreadSwitch):
    """Context manager: EdgeSeqModel forwards started inside it (on this thread) run the label filter, the code embedding and the
    CNN layers on the HIP kernels (on=True) where the predicates allow it, or on the composed path (on=False: torch ops)."""
    _slot = "eseq_fused"


def eseq_out_lens(L, k, padding, stride=1):
    """(L1, L2): the conv rows and the outputs of a layer on sequences of L positions."""
    L1 = (L + 2 * padding - k) // stride + 1
    return L1, L1 + 2 * padding - k // stride + 1


def eseq_fused_supported(x, weight, padding, act, stride=1, dilation=1, groups=1):
    """The predicate of eseq_conv_pool's kernels: fp32 on the GPU, C_in == C_out a multiple of 16 in 16 .. 128, 2 <= k <= 5,
    0 <= padding <= k // 2, stride = dilation = groups = 1, act in relu | leaky_relu | none, at least one output position, at most 65 535 sequences."""
    if weight.dim() != 3 or x.dim() != 3:
        return False
    Co, Ci, k = (int(s) for s in weight.shape)
    return (x.is_cuda and weight.is_cuda and x.dtype == weight.dtype == torch.float32 and Co == Ci == int(x.shape[2])
            and Co % 16 == 0 and 16 <= Co <= ESEQ_MAX_C and 2 <= k <= ESEQ_MAX_K and 0 <= padding <= k // 2
            and stride == 1 and dilation == 1 and groups == 1 and act in ESEQ_ACTS and 0 < x.shape[0] <= ESEQ_MAX_B
            and x.shape[0] * (x.shape[1] + 2 * ESEQ_MAX_K) * ESEQ_MAX_C < 2 ** 31       # (the kernels' grids and 32-bit tile offsets)
            and eseq_out_lens(int(x.shape[1]), k, padding)[1] >= 1)


def _eseq_windows(x, k, p, fill):
    return torch.nn.functional.pad(x, (0, 0, p, p), value=fill).unfold(1, k, 1)


def eseq_conv_pool_composed(x, weight, bias, gate_in, padding, act, residual):
    """eseq_conv_pool in torch ops on rows layout (any device and dtype; act: any name of the activation table)."""
    from .subgraph_isomorphism.act import map_activation_str_to_layer
    k, p = int(weight.shape[2]), int(padding)
    g = gate_in.reshape(x.shape[0], x.shape[1], 1).to(x.dtype)
    x0 = x * g
    conv = torch.einsum("blcj,ocj->blo", _eseq_windows(x0, k, p, 0.0), weight) + bias
    pooled = _eseq_windows(map_activation_str_to_layer(act)(conv), k, p, float("-inf")).max(dim=-1)[0]
    g2 = _eseq_windows(_eseq_windows(g, k, p, float("-inf")).max(dim=-1)[0], k, p, float("-inf")).max(dim=-1)[0]
    y = pooled * g2
    if residual and y.shape == x0.shape:
        y = y + x0
    return y, g2


class _EseqConvPoolFn(torch.autograd.Function):
    """One CNN layer in rows layout.  forward: ONE kernel launch (dn_eseq_conv_pool_fwd_f32) behind a re-laid copy of the weight;
    backward: FOUR (dconv gather, input gradient, weight-gradient partials, their in-order combine) behind a second re-laid copy.
    No atomics: bit-identical from run to run."""

    @staticmethod
    def forward(ctx, x, weight, bias, gate, lo, padding, act, residual):
        B, L, C = (int(s) for s in x.shape)
        k = int(weight.shape[2])
        L1, L2 = eseq_out_lens(L, k, padding)
        wt = weight.permute(2, 1, 0).contiguous()                   # [j][ci][co]
        y = torch.empty((B, L2, C), dtype=torch.float32, device=x.device)
        gate_out = torch.empty((B, L2), dtype=torch.float32, device=x.device)
        arg = torch.empty((B, L2, C), dtype=torch.uint8, device=x.device)
        code = ESEQ_ACTS[act]
        launch_tagged("eseq_conv_pool_fwd", lambda: check(lib().dn_eseq_conv_pool_fwd_f32(
            B, L, C, k, padding, code, ESEQ_LEAKY_SLOPE, 1 if residual else 0, ptr(x), ptr(gate), ptr(wt), ptr(bias), ptr(lo), ptr(y),
            ptr(gate_out), ptr(arg), stream_ptr()), "dn_eseq_conv_pool_fwd_f32"))
        ctx.geo = (B, L, C, k, int(padding), code, bool(residual))
        ctx.save_for_backward(x, weight, gate, lo, gate_out, arg)
        ctx.mark_non_differentiable(gate_out)
        return y, gate_out

    @staticmethod
    def backward(ctx, dy, _dgate):
        x, weight, gate, lo, gate_out, arg = ctx.saved_tensors
        B, L, C, k, p, code, residual = ctx.geo
        L1, L2 = eseq_out_lens(L, k, p)
        dy = dy.contiguous()
        dev = x.device
        dconv = torch.empty((B, L1, C), dtype=torch.float32, device=dev)
        launch_tagged("eseq_dconv", lambda: check(lib().dn_eseq_dconv_f32(
            B, L, C, k, p, code, ESEQ_LEAKY_SLOPE, ptr(dy), ptr(gate_out), ptr(arg), ptr(dconv), stream_ptr()), "dn_eseq_dconv_f32"))
        dx = dW = db = None
        if ctx.needs_input_grad[0]:
            wd = weight.flip(2).permute(2, 0, 1).contiguous()       # [j][co][ci], j reversed
            dx = torch.empty_like(x)
            launch_tagged("eseq_dgrad", lambda: check(lib().dn_eseq_dgrad_f32(
                B, L, C, k, p, 1 if residual else 0, ptr(dconv), ptr(dy), ptr(gate), ptr(wd), ptr(lo), ptr(dx), stream_ptr()),
                "dn_eseq_dgrad_f32"))
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            G = max(1, min(ESEQ_WGRAD_SLICES, B * ((L1 + 31) // 32)))
            part = torch.empty((G, k, C, C), dtype=torch.float32, device=dev)
            part_b = torch.empty((G, C), dtype=torch.float32, device=dev)
            launch_tagged("eseq_wgrad", lambda: check(lib().dn_eseq_wgrad_f32(
                B, L, C, k, p, ptr(x), ptr(gate), ptr(dconv), ptr(lo), G, ptr(part), ptr(part_b), stream_ptr()), "dn_eseq_wgrad_f32"))
            dW, db = torch.empty_like(weight), torch.empty((C,), dtype=torch.float32, device=dev)
            launch_tagged("eseq_wgrad_combine", lambda: check(lib().dn_eseq_wgrad_combine_f32(
                C, k, G, ptr(part), ptr(part_b), ptr(dW), ptr(db), stream_ptr()), "dn_eseq_wgrad_combine_f32"))
        return dx, dW, db, None, None, None, None, None


def eseq_conv_pool(x, lens, weight, bias, gate_in, padding, act, residual):
    """One CNN layer on right-aligned sequences in rows layout: (y [B, L2, C], gate_out [B, L2, 1]) with x0 = x * gate_in,
    y = maxpool_k(act(conv1d(x0, weight, bias, padding)), padding) * gate_out (+ x0 when residual and L2 == L) and gate_out = gate_in
    through the same two max windows (DESIGN.md "SI count models: CNN").  x [B, L, C]; weight [C, C, k]; gate_in [B, L] or [B, L, 1],
    0 / 1 floats; lens: B host integers -- every non-zero of gate_in lies in the last lens[b] positions of its row (None: no bound).
    Gradients reach x, weight and bias.  The kernels where eseq_fused_supported holds, else eseq_conv_pool_composed."""
    B, L = int(x.shape[0]), int(x.shape[1])
    residual = bool(residual) and eseq_out_lens(L, int(weight.shape[2]), int(padding))[1] == L
    if not eseq_fused_supported(x, weight, int(padding), act):
        return launch_tagged("eseq_layer_composed", lambda: eseq_conv_pool_composed(x, weight, bias, gate_in, padding, act, residual))
    lens = [L] * B if lens is None else [int(v) for v in lens]
    if len(lens) != B or min(lens) < 0 or max(lens) > L:
        raise _lib.DnHipError("eseq_conv_pool: lens needs one length in [0, L] per sequence")
    lo = torch.tensor([L - v for v in lens], dtype=I32).to(x.device, non_blocking=True)
    gate = gate_in.reshape(B, L).to(torch.float32).contiguous()
    require_gpu(x, weight, bias, gate)
    y, gate_out = _EseqConvPoolFn.apply(x.contiguous(), weight.contiguous(), bias.contiguous(), gate, lo, int(padding), act, residual)
    return y, gate_out.unsqueeze(-1)


def eseq_filter_max_labels():
    """The cap of eseq_filter_gate's kernel: labels in [0, cap) fit its LDS bit sets (4096)."""
    return int(lib().dn_eseq_filter_max_labels())


def eseq_filter_supported(p_ul, p_el, p_vl, g_ul, g_el, g_vl, num_labels):
    """int64 [B, Lp] / [B, Lg] label tensors on the GPU, and label tables of at most eseq_filter_max_labels() entries."""
    ts = (p_ul, p_el, p_vl, g_ul, g_el, g_vl)
    return (all(t.is_cuda and t.dtype == torch.int64 and t.dim() == 2 for t in ts) and p_ul.shape == p_el.shape == p_vl.shape
            and g_ul.shape == g_el.shape == g_vl.shape and p_ul.shape[0] == g_ul.shape[0] and p_ul.numel() > 0 and g_ul.numel() > 0
            and p_ul.shape[0] <= ESEQ_MAX_B and max(p_ul.numel(), g_ul.numel()) < 2 ** 31
            and int(num_labels) <= eseq_filter_max_labels())


def eseq_filter_gate_composed(p_ul, p_el, p_vl, g_ul, g_el, g_vl):
    """get_filter_gate of the reference in torch ops: three ScalarFilters ([B, Lg, Lp] differences each), and-ed."""
    def one(p_x, g_x):
        return torch.max((g_x.unsqueeze(2) - p_x.unsqueeze(1)) == 0, dim=2)[0]
    return (one(p_ul, g_ul) & one(p_vl, g_vl)) & one(p_el, g_el)


def eseq_filter_gate(p_ul, p_el, p_vl, g_ul, g_el, g_vl):
    """[B, Lg] bool: graph position (b, t) passes when each of its three labels occurs in the matching PADDED pattern row b (the
    padded zeros count, as in the reference).  One launch of dn_eseq_filter_gate_i64; labels must lie in [0, eseq_filter_max_labels())
    (eseq_filter_supported with the label table size; larger tables: eseq_filter_gate_composed)."""
    ts = [t.contiguous() for t in (p_ul, p_el, p_vl, g_ul, g_el, g_vl)]
    require_gpu(*ts)
    if not eseq_filter_supported(*ts, num_labels=0):
        raise _lib.DnHipError("eseq_filter_gate: int64 [B, Lp] / [B, Lg] label tensors on the GPU expected")
    B, Lp, Lg = int(ts[0].shape[0]), int(ts[0].shape[1]), int(ts[3].shape[1])
    out = torch.empty((B, Lg), dtype=torch.bool, device=ts[0].device)
    launch_tagged("eseq_filter_gate", lambda: check(lib().dn_eseq_filter_gate_i64(B, Lp, Lg, *[ptr(t) for t in ts], ptr(out), stream_ptr()),
                                                   "dn_eseq_filter_gate_i64"))
    return out


# ----------------------------------------------------------------------------------------------
# The RNN count model on edge sequences: LSTM / GRU / tanh recurrence with the gate (and the residual) per layer (dn_eseq_rnn.hip)
# ----------------------------------------------------------------------------------------------
ESEQ_RNN_CELLS = {"LSTM": 0, "GRU": 1, "RNN": 2}
ESEQ_RNN_GATES = {"LSTM": 4, "GRU": 3, "RNN": 1}
ESEQ_RNN_WIDTHS = (16, 32, 48, 64)                               # hidden units per direction: W_hh stays in a workgroup's registers
ESEQ_RNN_MAX_IN = 128

# The RNN layers' default behind the same switch (`with ops.eseq_fused(on)`).  Measured on the scale batch (docs/LAB_NOTES.md "SI count
# models: RNN"; 512 pairs, H = 64, graph sequences of 302 tuples, three paths alternated in one process, 3 rounds): the layer step
# 3.54 ms fused against 11.4 ms on torch's module (MIOpen) at LSTM and 3.22 against 41.9 ms at GRU, the model step (3 layers) 14.3
# against 53.8 ms and 13.6 against 116.7 ms; torch's native per-step kernels took 63 - 68 ms a layer step.  Every fused round was faster
# than every composed round, so by the project's rule the kernels are the default.
ESEQ_RNN_FUSED_DEFAULT = True


# The composed path on the GPU: torch's own layer goes to MIOpen (False) or, with the cuDNN / MIOpen backend switched off around
# the call, to torch's native per-step kernels (True).  MIOpen: it ran every test and was 1.6 - 5.8 times faster than the native path
# on the scale batch (docs/LAB_NOTES.md "SI count models: RNN").  The one exception is made where it is needed (RNNLayer.forward): a
# backward pass through a module in eval mode, which torch refuses on MIOpen.
ESEQ_RNN_COMPOSED_NATIVE = False


def eseq_rnn_fused_enabled():
    return eseq_fused.override(ESEQ_RNN_FUSED_DEFAULT)


def eseq_rnn_composed_backend(native=None):
    """The context the composed path runs torch's recurrent layer in (native: None = ESEQ_RNN_COMPOSED_NATIVE)."""
    if ESEQ_RNN_COMPOSED_NATIVE if native is None else native:
        return torch.backends.cudnn.flags(enabled=False)
    return _contextlib.nullcontext()


def _eseq_rnn_names(bidirectional):
    return [n + s for s in (("", "_reverse") if bidirectional else ("",)) for n in ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")]


def eseq_rnn_supported(x, params, cell, bidirectional):
    """The predicate of eseq_rnn's kernels: fp32 on the GPU, cell in LSTM | GRU | RNN, hidden width per direction in {16, 32, 48, 64},
    input width a multiple of 16 up to 128, 1 <= B <= 65535, L >= 1, and B L max(D 5 Hd, H) below 2^31 (the launches' 32-bit bound).
    params: the torch module's tensors by name (weight_ih_l0, weight_hh_l0, bias_ih_l0, bias_hh_l0, and the _reverse set)."""
    if cell not in ESEQ_RNN_CELLS or x.dim() != 3 or any(n not in params for n in _eseq_rnn_names(bidirectional)):
        return False
    G, D = ESEQ_RNN_GATES[cell], 2 if bidirectional else 1
    B, L, H = (int(s) for s in x.shape)
    w_hh = params["weight_hh_l0"]
    Hd = int(w_hh.shape[1])
    ts = [params[n] for n in _eseq_rnn_names(bidirectional)]
    return (x.is_cuda and x.dtype == torch.float32 and all(t.is_cuda and t.dtype == torch.float32 for t in ts)
            and Hd in ESEQ_RNN_WIDTHS and H % 16 == 0 and 16 <= H <= ESEQ_RNN_MAX_IN
            and tuple(params["weight_ih_l0"].shape) == (G * Hd, H) and tuple(w_hh.shape) == (G * Hd, Hd)
            and 1 <= B <= ESEQ_MAX_B and L >= 1 and B * L * max(D * 5 * Hd, H) < 2 ** 31)


def eseq_rnn_composed(x, params, gate, cell, bidirectional, residual, native=None):
    """eseq_rnn on torch's own recurrent layer (any device and dtype): y = RNN(x * gate)[0] * gate (+ x * gate when residual and the
    widths agree).  On the GPU torch sends the layer to MIOpen; native=True runs torch's per-step kernels instead (None: the module's
    ESEQ_RNN_COMPOSED_NATIVE)."""
    if cell not in ESEQ_RNN_CELLS:
        raise ValueError("eseq_rnn: cell must be LSTM, GRU or RNN (got %r)" % (cell,))
    g = gate.reshape(x.shape[0], x.shape[1], 1).to(x.dtype)
    x0 = x * g
    flat = [params[n] for n in _eseq_rnn_names(bidirectional)]
    Hd = int(params["weight_hh_l0"].shape[1])
    D = 2 if bidirectional else 1
    h0 = x0.new_zeros((D, x.shape[0], Hd))
    fn = {"LSTM": torch._VF.lstm, "GRU": torch._VF.gru, "RNN": torch._VF.rnn_tanh}[cell]
    # (has_biases, num_layers, dropout, train, bidirectional, batch_first; train: torch refuses MIOpen's backward outside training mode)
    args = (x0, (h0, h0) if cell == "LSTM" else h0, flat, True, 1, 0.0, True, bool(bidirectional), True)
    with eseq_rnn_composed_backend(native if x.is_cuda else False):
        o = fn(*args)[0]
    y = o * g
    return y + x0 if residual and y.shape == x0.shape else y


class _EseqRnnFn(torch.autograd.Function):
    """The recurrence of one layer.  forward: ONE launch (dn_eseq_rnn_fwd_f32) over P = x0 W_ih^T + b; backward: ONE launch
    (dn_eseq_rnn_bwd_f32) for the pre-activation gradients, then per direction the W_hh gradient (and the GRU's b_hn) on the
    deterministic row kernel.  dx, dW_ih and the folded biases follow through linear_any's own backward.  No atomics."""

    @staticmethod
    def forward(ctx, P, whh, bhn, x0, gate, lo, cell, D, Hd, residual):
        B, L = int(P.shape[0]), int(P.shape[1])
        code, dev = ESEQ_RNN_CELLS[cell], P.device
        S = int(lib().dn_eseq_rnn_saved_per_unit(code))
        y = torch.empty((B, L, D * Hd), dtype=torch.float32, device=dev)
        h = torch.empty((B, L, D * Hd), dtype=torch.float32, device=dev)
        sv = torch.empty((B, L, D, S * Hd), dtype=torch.float32, device=dev) if S else None
        launch_tagged("eseq_rnn_fwd", lambda: check(lib().dn_eseq_rnn_fwd_f32(
            B, L, Hd, D, code, 1 if residual else 0, ptr(P), ptr(whh), ptr(bhn), ptr(x0) if residual else None, ptr(gate), ptr(lo),
            ptr(y), ptr(h), ptr(sv), stream_ptr()), "dn_eseq_rnn_fwd_f32"))
        ctx.geo = (B, L, D, Hd, cell, bool(residual))
        ctx.has_bhn = bhn is not None
        ctx.save_for_backward(whh, gate, lo, h, sv)
        return y

    @staticmethod
    def backward(ctx, dy):
        whh, gate, lo, h, sv = ctx.saved_tensors
        B, L, D, Hd, cell, residual = ctx.geo
        code, G, dev = ESEQ_RNN_CELLS[cell], ESEQ_RNN_GATES[cell], dy.device
        dy = dy.contiguous()
        dP = torch.empty((B, L, D * G * Hd), dtype=torch.float32, device=dev)
        dhn = torch.empty((B, L, D * Hd), dtype=torch.float32, device=dev) if cell == "GRU" else None
        launch_tagged("eseq_rnn_bwd", lambda: check(lib().dn_eseq_rnn_bwd_f32(
            B, L, Hd, D, code, ptr(dy), ptr(gate), ptr(lo), ptr(whh), ptr(h), ptr(sv), ptr(dP), ptr(dhn), stream_ptr()),
            "dn_eseq_rnn_bwd_f32"))
        dwhh = dbhn = None
        if ctx.needs_input_grad[1] or (ctx.has_bhn and ctx.needs_input_grad[2]):
            def _wgrad():
                _, chunks = _single_rel_table(B * L, dev)
                zero = h.new_zeros((B, 1, Hd))
                gw, gb = [], []
                for d in range(D):
                    hd = h[:, :, d * Hd:(d + 1) * Hd]
                    prev = torch.cat([zero, hd[:, :-1]], 1) if d == 0 else torch.cat([hd[:, 1:], zero], 1)   # h of the step before
                    a = dP[:, :, d * G * Hd:(d + 1) * G * Hd]
                    if cell == "GRU":                             # the hidden side of n sits inside r * (W_hn h + b_hn)
                        a = torch.cat([a[:, :, :2 * Hd], dhn[:, :, d * Hd:(d + 1) * Hd]], 2)
                    w, cs = rows_wgrad_any(a.reshape(B * L, G * Hd), prev.reshape(B * L, Hd), chunks, 1, want_colsum=True)
                    gw.append(w[0])
                    gb.append(cs[0, 2 * Hd:] if cell == "GRU" else None)
                return torch.stack(gw), (torch.stack(gb) if cell == "GRU" else None)
            dwhh, dbhn = launch_tagged("eseq_rnn_wgrad", _wgrad)
        return dP, dwhh, dbhn, (dy if residual else None), None, None, None, None, None, None


def eseq_rnn(x, lens, params, gate, cell, bidirectional, residual):
    """One RNN layer on right-aligned sequences in rows layout: y [B, L, D Hd] = RNN(x * gate)[0] * gate (+ x * gate when residual and
    D Hd == H), the recurrent layer being torch's nn.LSTM / nn.GRU / nn.RNN(batch_first=True, bidirectional) with the tensors `params`
    (a dict by torch's names: weight_ih_l0 [G Hd, H], weight_hh_l0 [G Hd, Hd], bias_ih_l0, bias_hh_l0, the _reverse set).  x [B, L, H];
    gate [B, L] or [B, L, 1], 0 / 1 floats; lens: B host integers -- every non-zero of gate lies in the last lens[b] positions of its
    row (None: no bound; only the reverse direction uses it).  Pad steps are computed, not skipped: the biases drive the state
    through them.  Gradients reach x and every weight and bias.  The kernels where eseq_rnn_supported holds, else
    eseq_rnn_composed (torch's own layer)."""
    if cell not in ESEQ_RNN_CELLS:
        raise ValueError("eseq_rnn: cell must be LSTM, GRU or RNN (got %r)" % (cell,))
    if not eseq_rnn_supported(x, params, cell, bidirectional):
        return launch_tagged("eseq_rnn_composed", lambda: eseq_rnn_composed(x, params, gate, cell, bidirectional, residual))
    B, L, H = (int(s) for s in x.shape)
    G, D, Hd = ESEQ_RNN_GATES[cell], 2 if bidirectional else 1, int(params["weight_hh_l0"].shape[1])
    lens = [L] * B if lens is None else [int(v) for v in lens]
    if len(lens) != B or min(lens) < 0 or max(lens) > L:
        raise _lib.DnHipError("eseq_rnn: lens needs one length in [0, L] per sequence")
    lo = torch.tensor([L - v for v in lens], dtype=I32).to(x.device, non_blocking=True)
    g = gate.reshape(B, L).to(torch.float32).contiguous()
    require_gpu(x, g)
    residual = bool(residual) and D * Hd == H
    sfx = ("", "_reverse")[:D]

    def _proj():
        x0 = x * g.unsqueeze(-1)
        w_ih = torch.cat([params["weight_ih_l0" + s] for s in sfx], 0)
        bs = []
        for s in sfx:
            b_ih, b_hh = params["bias_ih_l0" + s], params["bias_hh_l0" + s]
            bs.append(torch.cat([b_ih[:2 * Hd] + b_hh[:2 * Hd], b_ih[2 * Hd:]]) if cell == "GRU" else b_ih + b_hh)
        P = linear_any(x0.reshape(B * L, H), w_ih, torch.cat(bs), exact=True).view(B, L, D * G * Hd)
        whh = torch.stack([params["weight_hh_l0" + s] for s in sfx])
        bhn = torch.stack([params["bias_hh_l0" + s][2 * Hd:] for s in sfx]) if cell == "GRU" else None
        return x0, P, whh, bhn

    x0, P, whh, bhn = launch_tagged("eseq_rnn_proj", _proj)
    return _EseqRnnFn.apply(P, whh, bhn, x0 if residual else None, g, lo, cell, D, Hd, residual)


# ----------------------------------------------------------------------------------------------
# The TransformerXL count model on edge sequences: relative-position attention over a sliding memory (dn_txl.hip)
# ----------------------------------------------------------------------------------------------
TXL_HEAD_WIDTHS = (16, 32, 64)
TXL_MAX_SEG = 64
TXL_MAX_WINDOW = 128

# The TXL layers' default behind the same switch (`with ops.eseq_fused(on)`).  Measured on the scale batch (docs/LAB_NOTES.md "SI count
# models: TXL"; 512 pairs, H = 64, graph sequences of 302 tuples = 5 segments, the two paths alternated in one process, 3 rounds of 10
# steps): the layer step 5.81 ms fused against 11.30 ms composed at 1 head and 6.17 against 13.70 ms at 4 heads, the model step (3
# layers) 24.97 against 42.52 ms and 26.16 against 50.28 ms.  Every fused round was faster than every composed round on both settings,
# so by the project's rule the kernels are the default.
TXL_FUSED_DEFAULT = True


def txl_fused_enabled():
    return eseq_fused.override(TXL_FUSED_DEFAULT)


def txl_windows(Lp, seg_len, mem_len):
    """[(first key row, memory rows, first query row)] per segment: segment s attends [s seg - mlen, (s + 1) seg), mlen = min(mem, s seg)."""
    return [(s * seg_len - min(mem_len, s * seg_len), min(mem_len, s * seg_len), s * seg_len) for s in range(Lp // seg_len)]


def txl_attention_supported(q, k, v, k_mem, v_mem, rk, r_w_bias, r_r_bias, seg_len, mem_len):
    """The predicate of txl_attention's kernels: fp32 on the GPU, q / k / v (/ k_mem / v_mem) [B, Lp, n, d] with d in {16, 32, 64},
    seg_len in {16, 32, 48, 64}, Lp a multiple of it, mem_len a multiple of 16 (narrower than "any memory": a window is whole 16-key
    tiles) with seg_len + mem_len <= 128, rk [P >= seg_len + mem_len, n, d], biases [n, d], sizes below 2^31."""
    if q.dim() != 4:
        return False
    B, Lp, n, d = (int(s) for s in q.shape)
    seg_len, mem_len = int(seg_len), int(mem_len)
    ts = [q, k, v, rk, r_w_bias, r_r_bias] + ([k_mem, v_mem] if mem_len > 0 else [])
    if any(t is None for t in ts) or not all(t.is_cuda and t.dtype == torch.float32 for t in ts):
        return False
    P = int(rk.shape[0])
    return (d in TXL_HEAD_WIDTHS and seg_len % 16 == 0 and 16 <= seg_len <= TXL_MAX_SEG and mem_len >= 0 and mem_len % 16 == 0
            and seg_len + mem_len <= TXL_MAX_WINDOW and B >= 1 and Lp >= seg_len and Lp % seg_len == 0
            and all(tuple(t.shape) == (B, Lp, n, d) for t in ts[:3] + ts[6:]) and tuple(rk.shape) == (P, n, d) and P >= seg_len + mem_len
            and tuple(r_w_bias.shape) == (n, d) and tuple(r_r_bias.shape) == (n, d) and Lp // seg_len <= 65535 and n <= 65535
            and B * Lp * n * d < 2 ** 31 and B * (Lp // seg_len) * n * P * d < 2 ** 31)


def txl_rel_shift(x):
    """The reference's rel_shift on [B, qlen, klen, n]: pad a zero column, view as [klen + 1, qlen], drop the first row, view back."""
    B, ql, kl, n = x.shape
    x = torch.cat([x.new_zeros((B, ql, 1, n)), x], dim=2).view(B, kl + 1, ql, n)
    return x[:, 1:].reshape(B, ql, kl, n)


def txl_attention_composed(q, k, v, k_mem, v_mem, rk, r_w_bias, r_r_bias, seg_len, mem_len, scale):
    """txl_attention in torch ops, segment by segment (any device and dtype)."""
    B, Lp, n, d = q.shape
    outs = []
    for k0, mlen, q0 in txl_windows(int(Lp), int(seg_len), int(mem_len)):
        qs = q[:, q0:q0 + seg_len]
        ks, vs = k[:, q0:q0 + seg_len], v[:, q0:q0 + seg_len]
        if mlen > 0:
            ks, vs = torch.cat([k_mem[:, k0:q0], ks], 1), torch.cat([v_mem[:, k0:q0], vs], 1)
        klen = seg_len + mlen
        ac = torch.einsum("bind,bjnd->bijn", qs + r_w_bias, ks)
        bd = txl_rel_shift(torch.einsum("bind,jnd->bijn", qs + r_r_bias, rk[:klen].flip(0)))
        prob = torch.softmax((ac + bd) * scale, dim=2)
        outs.append(torch.einsum("bijn,bjnd->bind", prob, vs).reshape(B, seg_len, n * d))
    return torch.cat(outs, 1)


class _TxlAttnFn(torch.autograd.Function):
    """forward: ONE launch (dn_txl_attn_fwd_f32).  backward: dn_txl_attn_bwd_f32, then the two fixed-order sums (the memory rows'
    gradient, d rk); the bias gradients are the row sums of the two parts of dq.  No atomics."""

    @staticmethod
    def forward(ctx, q, k, v, k_mem, v_mem, rk, rwb, rrb, seg, mem, scale):
        B, Lp, n, d = (int(s) for s in q.shape)
        P = int(rk.shape[0])
        q, k, v, rk, rwb, rrb = (t.contiguous() for t in (q, k, v, rk, rwb, rrb))
        k_mem, v_mem = (k_mem.contiguous(), v_mem.contiguous()) if mem > 0 else (None, None)
        require_gpu(q, k, v, k_mem, v_mem, rk, rwb, rrb)
        out = torch.empty((B, Lp, n * d), dtype=torch.float32, device=q.device)
        stats = torch.empty((B, Lp, n, 2), dtype=torch.float32, device=q.device)
        launch_tagged("txl_attn_fwd", lambda: check(lib().dn_txl_attn_fwd_f32(
            B, Lp, n, d, seg, mem, P, scale, ptr(q), ptr(k), ptr(v), ptr(k_mem), ptr(v_mem), ptr(rk), ptr(rwb), ptr(rrb), ptr(out),
            ptr(stats), stream_ptr()), "dn_txl_attn_fwd_f32"))
        ctx.geo = (B, Lp, n, d, P, seg, mem, scale)
        ctx.save_for_backward(q, k, v, k_mem, v_mem, rk, rwb, rrb, out, stats)
        return out

    @staticmethod
    def backward(ctx, dout):
        q, k, v, k_mem, v_mem, rk, rwb, rrb, out, stats = ctx.saved_tensors
        B, Lp, n, d, P, seg, mem, scale = ctx.geo
        S, dev = Lp // seg, dout.device
        dout = dout.contiguous()
        new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)  # noqa: E731
        dq_ac, dq_bd, dk, dv = new(B, Lp, n, d), new(B, Lp, n, d), new(B, Lp, n, d), new(B, Lp, n, d)
        k_part, v_part = (new(B, S, n, mem, d), new(B, S, n, mem, d)) if mem > 0 else (None, None)
        rk_part = new(B, S, n, P, d)

        def _bwd():
            check(lib().dn_txl_attn_bwd_f32(
                B, Lp, n, d, seg, mem, P, scale, ptr(dout), ptr(q), ptr(k), ptr(v), ptr(k_mem), ptr(v_mem), ptr(rk), ptr(rwb), ptr(rrb),
                ptr(out), ptr(stats), ptr(dq_ac), ptr(dq_bd), ptr(dk), ptr(dv), ptr(k_part), ptr(v_part), ptr(rk_part), stream_ptr()),
                "dn_txl_attn_bwd_f32")
            dkm = dvm = None
            if mem > 0 and (ctx.needs_input_grad[3] or ctx.needs_input_grad[4]):
                dkm, dvm = new(B, Lp, n, d), new(B, Lp, n, d)
                check(lib().dn_txl_fold_mem_f32(B, Lp, n, d, seg, mem, ptr(k_part), ptr(v_part), ptr(dkm), ptr(dvm), stream_ptr()),
                      "dn_txl_fold_mem_f32")
            drk = None
            if ctx.needs_input_grad[5]:
                drk = new(P, n, d)
                check(lib().dn_txl_reduce_rk_f32(B, Lp, n, d, seg, mem, P, ptr(rk_part), ptr(drk), stream_ptr()), "dn_txl_reduce_rk_f32")
            return dkm, dvm, drk

        dkm, dvm, drk = launch_tagged("txl_attn_bwd", _bwd)
        need = ctx.needs_input_grad
        return (dq_ac + dq_bd if need[0] else None, dk if need[1] else None, dv if need[2] else None, dkm if need[3] else None,
                dvm if need[4] else None, drk, dq_ac.sum((0, 1)) if need[6] else None, dq_bd.sum((0, 1)) if need[7] else None,
                None, None, None)


def txl_attention(q, k, v, k_mem, v_mem, rk, r_w_bias, r_r_bias, seg_len, mem_len, scale):
    """TransformerXL's relative-position attention of one layer over the whole padded sequence: out [B, Lp, n d].  q, k, v [B, Lp, n, d]:
    the projections of every row; k_mem, v_mem [B, Lp, n, d]: the same rows as the MEMORY sees them (in the model: projected from the
    detached input, so that their gradient reaches the weights and not the input; None when mem_len == 0); rk [P, n, d]: the
    projected position table, row p = relative position p; r_w_bias, r_r_bias [n, d].  The queries of segment s (seg_len rows) attend
    the rows [s seg_len - mlen, (s + 1) seg_len), mlen = min(mem_len, s seg_len), the first mlen of them through k_mem / v_mem:

        score = scale ((q + r_w_bias) K^T + rel_shift((q + r_r_bias) rk[klen - 1 .. 0]^T)),   out = softmax(score) V

    with the reference's pad-and-view rel_shift and NO mask (the wrapped entries take part).  Gradients reach every tensor argument.
    The kernels where txl_attention_supported holds, else txl_attention_composed."""
    seg_len, mem_len = int(seg_len), int(mem_len)
    if not txl_attention_supported(q, k, v, k_mem, v_mem, rk, r_w_bias, r_r_bias, seg_len, mem_len):
        return launch_tagged("txl_composed", lambda: txl_attention_composed(q, k, v, k_mem, v_mem, rk, r_w_bias, r_r_bias, seg_len,
                                                                             mem_len, scale))
    return _TxlAttnFn.apply(q, k, v, k_mem, v_mem, rk, r_w_bias, r_r_bias, seg_len, mem_len, float(scale))


# ------------------------------------------------------------------------------------------------ kernel-SVM evaluation: batched SMO
# (dn_svm.hip; the evaluation -- reader, splits, one-vs-one votes, tables, command line -- is graph_kernels_svm.py)
# The default of graph_kernels_svm.evaluate_dataset, and the iterations a launch of dn_svm_smo_f64 may run per solve: both measured by
# tools/graph_kernel_svm_bench.py (docs/LAB_NOTES.md "Graph kernels: SVM evaluation"; 4110 NCI1-shaped graphs, WL at H = 5, 3288 training
# rows).  On the subset the composed path can finish (1 seed x 6 matrices x C in {1, 0.1, 0.01, 0.001}: 24 duals, 39,537 iterations)
# fused and composed alternated in one process took 0.040 against 1.91 s, every fused round faster than every composed round, so the
# kernel is the default.  The whole search (420 duals, 8.68 M iterations) took 8.7 s in 44 launches of at most 20,000 iterations, the
# longest 284 ms; at 5,000 it took 8.7 s in 173 launches, the longest 112 ms: far below a second at no cost, so that is the default.
SVM_FUSED_DEFAULT = True
SVM_ITERS_PER_LAUNCH = 5000
SVM_TAU = 1e-12
SVM_CONVERGED, SVM_RUNNING, SVM_CAPPED, SVM_BAD_ROW = 0, 1, 2, 3


def svm_fused_enabled():
    return svm_fused.override(SVM_FUSED_DEFAULT)


class svm_fused(_ThreadSwitch):
    """Context manager: SVM evaluations started inside it (on this thread) solve with dn_svm_smo_f64 (on=True; a solve with more than
    svm_max_rows() training rows, or on CPU tensors, takes the composed path either way) or with svm_smo_composed (on=False)."""
    _slot = "svm_fused"


def svm_max_rows():
    """The longest training-row list the SMO kernel keeps in LDS (28 bytes a row)."""
    return int(lib().dn_svm_max_rows())


def svm_smo_supported(K, max_len):
    """Whether svm_smo takes these solves: a device tensor and no row list above svm_max_rows() rows (its state lives in LDS)."""
    return bool(K.is_cuda) and int(max_len) <= svm_max_rows()


def _svm_table(K, table, rows):
    """The host's view of a solve table, checked: (matrix, offset, length, positives, C) numpy arrays.  ValueError on anything a
    kernel could read out of bounds through (the kernel checks again and reports status 3)."""
    if K.dim() != 3 or K.shape[1] != K.shape[2] or K.dtype != torch.float64:
        raise ValueError("K must be [num_matrices, n, n] float64 (got %s %s)" % (tuple(K.shape), K.dtype))
    if table.dim() != 2 or table.shape[1] != 5 or table.dtype != torch.float64 or table.shape[0] < 1:
        raise ValueError("table must be [num_solves >= 1, 5] float64 {matrix, offset, length, positives, C}")
    if rows.dim() != 1 or rows.dtype != I32 or rows.numel() < 1:
        raise ValueError("rows must be a non-empty int32 vector")
    t = table.detach().cpu().numpy()
    if not _np.isfinite(t).all() or (t[:, :4] != _np.floor(t[:, :4])).any():
        raise ValueError("table: matrix, offset, length and positives must be integers, C finite")
    mat, off, length, npos = (t[:, c].astype(_np.int64) for c in range(4))
    C = t[:, 4].copy()
    R, M, n = int(rows.numel()), int(K.shape[0]), int(K.shape[1])
    if (mat < 0).any() or (mat >= M).any() or (off < 0).any() or (length < 1).any() or (off + length > R).any() or (npos < 0).any() or \
            (npos > length).any() or not (C > 0).all():
        raise ValueError("table: a solve names a matrix outside 0..%d, rows outside 0..%d, more positives than rows or C <= 0" % (M - 1, R - 1))
    if bool(((rows < 0) | (rows >= n)).any()):
        raise ValueError("rows: an index outside 0..%d" % (n - 1))
    return mat, off, length, npos, C


def _svm_warn_capped(status):
    if bool((status == SVM_CAPPED).any()):
        import warnings
        warnings.warn("WARNING: reaching max number of iterations")


def svm_smo(K, table, rows, eps, iters_per_launch=None):
    """Every C-SVC dual of `table` by SMO, one workgroup per solve (dn_svm_smo_f64): K [M, n, n] float64, table [S, 5] float64
    {matrix, offset, length, positives, C}, rows int32 (solve s trains on rows[offset .. offset + length), the first `positives` of
    them its +1 class; the lists of two solves must not overlap: alpha lives at the same offsets).  Returns (alpha [len(rows)], rho [S],
    iterations [S] int64, status [S] int32).  A launch runs at most iters_per_launch iterations per solve; the solves still running
    are listed and launched again (one count read back per launch) until none run or libsvm's cap max(10^7, 100 l) stops them
    (status 2, a warning in libsvm's words, the solve is used as it stands).  The result does not depend on iters_per_launch."""
    require_gpu(K, table, rows)
    mat, off, length, npos, C = _svm_table(K, table, rows)
    if not eps > 0:
        raise ValueError("eps must be > 0 (got %r)" % (eps,))
    ipl = SVM_ITERS_PER_LAUNCH if iters_per_launch is None else int(iters_per_launch)
    if ipl < 1:
        raise ValueError("iters_per_launch must be >= 1 (got %d)" % ipl)
    max_len = int(length.max())
    if max_len > svm_max_rows():
        raise _lib.DnHipError("svm_smo: a solve with %d training rows exceeds the kernel's %d (svm_smo_supported; svm_smo_composed has "
                              "no limit)" % (max_len, svm_max_rows()))
    S, R, dev = int(table.shape[0]), int(rows.numel()), K.device
    alpha = torch.zeros(R, dtype=torch.float64, device=dev)
    grad = torch.full((R,), -1.0, dtype=torch.float64, device=dev)
    rho = torch.zeros(S, dtype=torch.float64, device=dev)
    iterations = torch.zeros(S, dtype=torch.int64, device=dev)
    status = torch.full((S,), SVM_RUNNING, dtype=I32, device=dev)
    todo = None
    launches_left = S * (int(max(10 ** 7, 100 * max_len)) // ipl + 2)         # (every launch ends or advances a solve: a plain bound)
    while launches_left > 0:
        n_list = S if todo is None else int(todo.numel())

        def _launch():
            check(lib().dn_svm_smo_f64(int(K.shape[0]), int(K.shape[1]), ptr(K), S, ptr(table), n_list, ptr(todo), R, ptr(rows), max_len,
                                       float(eps), ipl, ptr(alpha), ptr(grad), ptr(rho), ptr(iterations), ptr(status), stream_ptr()),
                  "dn_svm_smo_f64")
        launch_tagged("svm_smo", _launch)
        launches_left -= 1
        todo = torch.nonzero(status == SVM_RUNNING).view(-1).to(I32)          # (the read-back: how many still run)
        if todo.numel() == 0:
            break
    if bool((status == SVM_BAD_ROW).any()):
        raise _lib.DnHipError("dn_svm_smo_f64 refused a table row (status 3)")
    _svm_warn_capped(status)
    return alpha, rho, iterations, status


def svm_smo_composed(K, table, rows, eps, iters_per_launch=None):
    """svm_smo's algorithm in torch ops, every solve of the table side by side as rows of padded [S, longest list] tensors: any
    size, any device, CPU tensors too.  The same selection rule, ties, update, clipping, stopping rule, cap and rho; the sums run in
    torch's order, so the last bits may differ from the kernel's.  iters_per_launch is accepted and ignored (nothing is sliced)."""
    mat, off, length, npos, C = _svm_table(K, table, rows)
    if not eps > 0:
        raise ValueError("eps must be > 0 (got %r)" % (eps,))
    dev, f64 = K.device, torch.float64
    S, L, n = len(mat), int(length.max()), int(K.shape[1])
    ar = _np.arange(L)[None, :]
    valid_h = ar < length[:, None]
    slot_h = _np.where(valid_h, off[:, None] + ar, 0)
    to = lambda a, dt: torch.from_numpy(_np.ascontiguousarray(a)).to(device=dev, dtype=dt)  # noqa: E731
    valid, slot = to(valid_h, torch.bool), to(slot_h, torch.int64)
    idx = torch.where(valid, rows.long()[slot], torch.zeros_like(slot))
    y = to(_np.where(ar < npos[:, None], 1.0, -1.0), f64)
    Cs = to(C[:, None], f64)
    base = to(mat[:, None] * n * n, torch.int64)
    cap = to(_np.maximum(10 ** 7, 100 * length), torch.int64)
    Kf = K.reshape(-1)
    diag = Kf[base + idx * (n + 1)]
    ninf = torch.full((), float("-inf"), dtype=f64, device=dev)
    a = torch.zeros((S, L), dtype=f64, device=dev)
    G = torch.full((S, L), -1.0, dtype=f64, device=dev)
    iters = torch.zeros(S, dtype=torch.int64, device=dev)
    done = torch.zeros(S, dtype=torch.bool, device=dev)
    capped = torch.zeros(S, dtype=torch.bool, device=dev)
    ypos = y > 0
    check_every = 16 if K.is_cuda else 1

    def first_max(x):                     # (torch.max over a dim returns the index of the FIRST maximal value: the lowest index wins a tie)
        return x.max(1, keepdim=True)

    def loop(a, G):
        step = 0
        while True:
            v = -y * G
            up = valid & torch.where(ypos, a < Cs, a > 0)
            low = valid & torch.where(ypos, a > 0, a < Cs)
            gmax, i = first_max(torch.where(up, v, ninf))
            m2 = torch.where(low, -v, ninf).max(1, keepdim=True)[0]
            Ki = Kf[base + idx.gather(1, i) * n + idx]
            Kii = diag.gather(1, i)
            b = gmax - v
            q = Kii + diag - 2.0 * Ki
            score, j = first_max(torch.where(low & (b > 0), (b * b) / q.masked_fill(~(q > 0), SVM_TAU), ninf))
            stop = (~(gmax + m2 >= eps) | (score == ninf)).view(-1)                # (gmax = -inf: no i at all)
            capped.logical_or_(~done & (iters >= cap))                                       # (libsvm leaves its loop at the cap without a look at the rule)
            done.logical_or_(stop | capped)
            frozen = done.view(-1, 1)
            Kj = Kf[base + idx.gather(1, j) * n + idx]
            yi, yj, Gi, Gj, oai, oaj = y.gather(1, i), y.gather(1, j), G.gather(1, i), G.gather(1, j), a.gather(1, i), a.gather(1, j)
            Qij = yi * yj * Ki.gather(1, j)
            Kjj = diag.gather(1, j)
            # y_i != y_j
            qd = Kii + Kjj + 2.0 * Qij
            qd = qd.masked_fill(qd <= 0, SVM_TAU)
            delta = (-Gi - Gj) / qd
            diff = oai - oaj
            ai, aj = oai + delta, oaj + delta
            c1 = (diff > 0) & (aj < 0)
            c2 = ~(diff > 0) & (ai < 0)
            ai, aj = torch.where(c1, diff, ai.masked_fill(c2, 0.0)), torch.where(c2, -diff, aj).masked_fill(c1, 0.0)
            c1 = (diff > 0) & (ai > Cs)
            c2 = ~(diff > 0) & (aj > Cs)
            ai_d, aj_d = torch.where(c1, Cs, torch.where(c2, Cs + diff, ai)), torch.where(c1, Cs - diff, torch.where(c2, Cs, aj))
            # y_i == y_j
            qs = Kii + Kjj - 2.0 * Qij
            qs = qs.masked_fill(qs <= 0, SVM_TAU)
            delta = (Gi - Gj) / qs
            tot = oai + oaj
            ai, aj = oai - delta, oaj + delta
            c1 = (tot > Cs) & (ai > Cs)
            c2 = ~(tot > Cs) & (aj < 0)
            ai, aj = torch.where(c1, Cs, torch.where(c2, tot, ai)), torch.where(c1, tot - Cs, aj.masked_fill(c2, 0.0))
            c1 = (tot > Cs) & (aj > Cs)
            c2 = ~(tot > Cs) & (ai < 0)
            ai_s, aj_s = torch.where(c1, tot - Cs, ai.masked_fill(c2, 0.0)), torch.where(c1, Cs, torch.where(c2, tot, aj))
            same = yi == yj
            ai = torch.where(frozen, oai, torch.where(same, ai_s, ai_d))
            aj = torch.where(frozen, oaj, torch.where(same, aj_s, aj_d))
            G = G + ((y * yi * Ki) * (ai - oai) + (y * yj * Kj) * (aj - oaj))     # (libsvm's association: symmetric problems stay symmetric)
            a = a.scatter(1, i, ai).scatter(1, j, aj)
            iters.add_((~done).to(torch.int64))
            step += 1
            if step % check_every == 0 and bool(done.all()):
                return a, G

    threads = torch.get_num_threads()
    if not K.is_cuda:                      # (a step is some sixty ops on small [S, L] tensors: waking a thread pool for each costs more
        torch.set_num_threads(1)           #  than it computes)
    try:
        a, G = loop(a, G)
    finally:
        torch.set_num_threads(threads)
    status = torch.where(capped, torch.full_like(iters, SVM_CAPPED), torch.full_like(iters, SVM_CONVERGED)).to(I32)
    yG = y * G
    free = valid & (a > 0) & (a < Cs)
    at_c, at_0 = valid & (a >= Cs), valid & (a <= 0)
    inf = torch.full((), float("inf"), dtype=f64, device=dev)
    ub = torch.where((at_c & ~ypos) | (at_0 & ypos), yG, inf).min(1)[0]
    lb = torch.where((at_c & ypos) | (at_0 & ~ypos), yG, ninf).max(1)[0]
    nfree = free.sum(1)
    rho = torch.where(nfree > 0, torch.where(free, yG, torch.zeros_like(yG)).sum(1) / nfree.clamp(min=1), (ub + lb) / 2.0)
    alpha = torch.zeros(int(rows.numel()), dtype=f64, device=dev)
    alpha[slot[valid]] = a[valid]
    _svm_warn_capped(status)
    return alpha, rho, iters, status


# ------------------------------------------------------------------------------------------------ the SI training objective
# (dn_objective.hip; the schedules, SIObjective and the epoch meters are subgraph_isomorphism/objective.py)
# The default of si_objective, by the project's rule: on only if every fused round beats every composed round.  Measured on the scale
# batch (tools/si_objective_bench.py; docs/LAB_NOTES.md "SI training objective"; 512 pairs, 25,600 graph nodes, H = 64, node weights
# present, the reference's default schedules, the two paths alternated in one process, 5 rounds): the objective's forward + backward
# 0.131 ms fused against 0.746 ms composed (6 against 90 device kernels), every fused round faster than every composed round; the RGIN
# model step 3.76 against 4.07 ms, the fused round faster than the composed round next to it in all five, but the step time drifted
# from 5.5 to 3.9 ms over the process, so NOT every fused round beat every composed round.  By the rule the kernels stay opt-in:
# `with ops.objective_fused():`.
SI_OBJECTIVE_FUSED_DEFAULT = False
SI_OBJECTIVE_CRITERIA = {"MAE": 0, "MSE": 1, "SMSE": 2}
SI_OBJECTIVE_TERMS = ("eval", "bp_loss", "match_v_loss", "match_e_loss", "match_v_reg", "match_e_reg", "rep_reg")
SI_OBJECTIVE_MAX_REPS = 4


def objective_fused_enabled():
    return objective_fused.override(SI_OBJECTIVE_FUSED_DEFAULT)


class objective_fused(_ThreadSwitch):
    """Context manager: si_objective / si_eval_errors calls inside it (on this thread) run dn_objective_* (on=True; anything but
    fp32 / bf16 CUDA tensors takes the composed path either way) or the torch ops of si_objective_composed (on=False)."""
    _slot = "objective_fused"


def _objective_dt(t):
    return 0 if t.dtype == torch.float32 else 1


def _objective_float(t):
    return t is None or (t.is_cuda and t.dtype in (torch.float32, torch.bfloat16))


def si_objective_supported(pred_c, counts, reps=(), pred_v=None, v_target=None, pred_e=None, e_target=None):
    """The predicate of the dn_objective_* kernels: fp32 or bf16 CUDA tensors (each its own dtype), at most four representations."""
    ts = [pred_c, counts, pred_v, v_target, pred_e, e_target] + list(reps)
    return len(reps) <= SI_OBJECTIVE_MAX_REPS and all(_objective_float(t) for t in ts) and pred_c.numel() >= 1 and \
        all(r.dim() >= 2 and r.numel() >= 1 for r in reps) and all(t is None or t.numel() >= 1 for t in (pred_v, pred_e))


def _objective_crit(name, what):
    if name not in SI_OBJECTIVE_CRITERIA:
        raise NotImplementedError("%s %r (MAE, MSE or SMSE)" % (what, name))
    return SI_OBJECTIVE_CRITERIA[name]


class _MaskedZeroPassFn(torch.autograd.Function):
    """x with its masked entries (mask False) set to 0, the gradient passed through unchanged: what the reference's in-place
    masked_fill_ under no_grad amounts to (train.py:784), without touching x."""

    @staticmethod
    def forward(ctx, x, mask):
        return x.masked_fill(~mask, 0)

    @staticmethod
    def backward(ctx, g):
        return g, None


def si_objective_composed(pred_c, counts, bp_loss, eval_metric, neg_slp, rep_reg_w, match_loss_w, match_reg_w, reps=(), pred_v=None,
                          v_mask=None, v_target=None, pred_e=None, e_mask=None, e_target=None):
    """si_objective in torch ops, written as the reference writes it (train.py:776-813; on CPU tensors the same bits): any dtype, any
    device.  The caller's tensors are left as they are."""
    F = torch.nn.functional
    fn = {"MAE": F.l1_loss, "MSE": F.mse_loss, "SMSE": F.smooth_l1_loss}
    _objective_crit(bp_loss, "bp_loss"), _objective_crit(eval_metric, "eval_metric")
    eval_crit = lambda pred, target: fn[eval_metric](F.relu(pred), target)  # noqa: E731
    bp_crit = lambda pred, target, slp: fn[bp_loss](F.leaky_relu(pred, slp), target)  # noqa: E731
    pc = pred_c.reshape(-1, 1)
    c = counts.reshape(-1, 1).to(pc.dtype)
    dev = pc.device
    ev = eval_crit(pc.detach(), c)
    bp = bp_crit(pc, c, neg_slp)

    def side(pred, mask, target):
        if pred is None or target is None:
            return torch.tensor([0.0], device=dev), torch.tensor([0.0], device=dev)
        mask = mask if mask.dtype == torch.bool else mask != 0
        w = target.detach().to(pred.dtype).masked_fill(~mask, 0)
        p = _MaskedZeroPassFn.apply(pred, mask)
        return bp_crit(p, w, neg_slp) * p.size(1), bp_crit(F.relu(p - pc), torch.zeros_like(p), 0) * p.size(1)

    v_loss, v_reg = side(pred_v, v_mask, v_target)
    e_loss, e_reg = side(pred_e, e_mask, e_target)
    rep_reg = torch.tensor([0.0], device=dev)
    for rep in reps:
        rep_reg = rep_reg + bp_crit(rep, torch.zeros_like(rep), 1) * rep.size(1)
    bp = bp + rep_reg_w * rep_reg
    bp = bp + match_loss_w * (v_loss + e_loss)
    bp = bp + match_reg_w * (v_reg + e_reg)
    loss = bp.reshape(())
    terms = torch.stack([t.detach().reshape(()).double() for t in (ev, bp, v_loss, e_loss, v_reg, e_reg, rep_reg)])
    return loss, terms


def _objective_side(pred, mask, target):
    """(L, pred, mask bytes, target) of one side for the kernels, contiguous; all None and 0 when the side is absent."""
    if pred is None or target is None:
        return 0, None, None, None
    B, L = int(pred.shape[0]), int(pred.numel() // max(int(pred.shape[0]), 1))
    mask = (mask if mask.dtype == torch.bool else mask != 0).reshape(B, L).contiguous()
    return L, pred.reshape(B, L).contiguous(), mask, target.detach().reshape(B, L).contiguous()


def _objective_rep_arrays(reps, grads=None):
    n = len(reps)
    ptrs = (ctypes.c_void_p * max(n, 1))(*[r.data_ptr() for r in reps])
    numel = (ctypes.c_int64 * max(n, 1))(*[int(r.numel()) for r in reps])
    denom = (ctypes.c_int64 * max(n, 1))(*[int(r.numel()) // int(r.shape[1]) for r in reps])
    dts = (ctypes.c_int32 * max(n, 1))(*[_objective_dt(r) for r in reps])
    gp = None if grads is None else (ctypes.c_void_p * max(n, 1))(*[None if g is None else g.data_ptr() for g in grads])
    return ptrs, numel, denom, dts, gp


class _SiObjectiveFn(torch.autograd.Function):
    """forward: dn_objective_fwd (the pass and its closing launch); backward: ONE launch of dn_objective_bwd, the upstream gradient
    read on the device.  Nothing is read back."""

    @staticmethod
    def forward(ctx, pred_c, counts, pred_v, v_mask, v_target, pred_e, e_mask, e_target, cfg, *reps):
        bp_crit, eval_crit, slope, rrw, mlw, mrw = cfg
        B = int(pred_c.numel())
        pc, c = pred_c.reshape(B).contiguous(), counts.detach().reshape(B).contiguous()
        Lv, pv, mv, wv = _objective_side(pred_v, v_mask, v_target)
        Le, pe, me, we = _objective_side(pred_e, e_mask, e_target)
        reps_c = [r.contiguous() for r in reps]
        dev = require_gpu(pc, c, pv, mv, wv, pe, me, we, *reps_c)
        ptrs, numel, denom, dts, _ = _objective_rep_arrays(reps_c)
        terms = torch.empty(7, dtype=torch.float64, device=dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        nb = int(lib().dn_objective_workspace_bytes(B, len(reps_c), numel))
        if nb == 0:
            check(-1, "dn_objective_workspace_bytes")
        ws = torch.empty(nb // 8, dtype=torch.float64, device=dev)
        dt = lambda t: 0 if t is None else _objective_dt(t)  # noqa: E731
        launch_tagged("si_objective_fwd", lambda: check(lib().dn_objective_fwd(
            B, ptr(pc), dt(pc), ptr(c), dt(c), Lv, ptr(pv), dt(pv), ptr(mv), ptr(wv), dt(wv), Le, ptr(pe), dt(pe), ptr(me), ptr(we), dt(we),
            len(reps_c), ptrs, numel, denom, dts, bp_crit, eval_crit, slope, rrw, mlw, mrw, ptr(terms), ptr(loss), ptr(ws), nb,
            stream_ptr()), "dn_objective_fwd"))
        ctx.cfg, ctx.sides = cfg, (Lv, Le)
        ctx.shapes = (pred_c.shape, None if pred_v is None else pred_v.shape, None if pred_e is None else pred_e.shape)
        ctx.save_for_backward(pc, c, pv, mv, wv, pe, me, we, *reps_c)
        ctx.mark_non_differentiable(terms)
        return loss, terms

    @staticmethod
    def backward(ctx, gloss, _gterms):
        pc, c, pv, mv, wv, pe, me, we, *reps = ctx.saved_tensors
        bp_crit, _, slope, rrw, mlw, mrw = ctx.cfg
        Lv, Le = ctx.sides
        need = ctx.needs_input_grad
        B = int(pc.numel())
        g = gloss.reshape(()).to(torch.float32).contiguous()
        dpc = torch.empty_like(pc) if need[0] else None
        dpv = torch.empty_like(pv) if pv is not None and need[2] else None
        dpe = torch.empty_like(pe) if pe is not None and need[5] else None
        dreps = [torch.empty_like(r) if need[9 + i] else None for i, r in enumerate(reps)]
        ptrs, numel, denom, dts, gp = _objective_rep_arrays(reps, dreps)
        dt = lambda t: 0 if t is None else _objective_dt(t)  # noqa: E731
        launch_tagged("si_objective_bwd", lambda: check(lib().dn_objective_bwd(
            B, ptr(g), ptr(pc), dt(pc), ptr(c), dt(c), Lv, ptr(pv), dt(pv), ptr(mv), ptr(wv), dt(wv), Le, ptr(pe), dt(pe), ptr(me), ptr(we),
            dt(we), len(reps), ptrs, numel, denom, dts, bp_crit, slope, rrw, mlw, mrw, ptr(dpc), ptr(dpv), ptr(dpe), gp, stream_ptr()),
            "dn_objective_bwd"))
        sc, sv, se = ctx.shapes
        return (None if dpc is None else dpc.view(sc), None, None if dpv is None else dpv.view(sv), None, None,
                None if dpe is None else dpe.view(se), None, None, None) + tuple(dreps)


def si_objective(pred_c, counts, bp_loss, eval_metric, neg_slp, rep_reg_w, match_loss_w, match_reg_w, reps=(), pred_v=None, v_mask=None,
                 v_target=None, pred_e=None, e_mask=None, e_target=None):
    """The reference's training objective of one step (train.py:776-813) -> (loss, terms): loss a 0-dim tensor to call backward on,
    terms [7] float64 on the device, no gradient, in the order SI_OBJECTIVE_TERMS (train.py:815-821).  pred_c, counts [B] or [B, 1];
    pred_x, x_mask, x_target [B, L_x], a side with no prediction or no target is skipped; reps: up to four representations
    ([N, H] or [B, L, H]).  bp_loss / eval_metric: "MAE", "MSE" or "SMSE"; the four scalars are Python numbers (schedule_value).
    Gradients reach pred_c, pred_v, pred_e -- at masked positions too, through the regulariser -- and every representation.
    The kernels under `with ops.objective_fused()` (ops.SI_OBJECTIVE_FUSED_DEFAULT) for fp32 / bf16 CUDA tensors, else
    si_objective_composed."""
    reps = tuple(reps)
    bp_c, ev_c = _objective_crit(bp_loss, "bp_loss"), _objective_crit(eval_metric, "eval_metric")
    if pred_v is None or v_target is None:
        pred_v = v_mask = v_target = None
    if pred_e is None or e_target is None:
        pred_e = e_mask = e_target = None
    if not (objective_fused_enabled() and si_objective_supported(pred_c, counts, reps, pred_v, v_target, pred_e, e_target)):
        return launch_tagged("si_objective_composed", lambda: si_objective_composed(
            pred_c, counts, bp_loss, eval_metric, neg_slp, rep_reg_w, match_loss_w, match_reg_w, reps, pred_v, v_mask, v_target, pred_e,
            e_mask, e_target))
    slope = float(_np.float32(neg_slp))                                        # (torch's leaky_relu multiplies by the slope as a float)
    cfg = (bp_c, ev_c, slope, float(rep_reg_w), float(match_loss_w), float(match_reg_w))
    return _SiObjectiveFn.apply(pred_c, counts, pred_v, v_mask, v_target, pred_e, e_mask, e_target, cfg, *reps)


def si_eval_errors_composed(pred_c, counts, pred_v=None, v_target=None, pred_e=None, e_target=None):
    """(AE, SE, NED, EED, cls) per pair in torch ops, as evaluate_epoch computes them (train.py:1111, :1126, :1164-1165); cls =
    (counts > 0) + 2 (relu(pred_c) > 0) as int32."""
    F = torch.nn.functional
    pc = F.relu(pred_c.detach().reshape(-1).float())
    c = counts.reshape(-1).float()
    ae = F.l1_loss(pc, c, reduction="none")
    se = F.mse_loss(pc, c, reduction="none")

    def dist(pred, target):
        if pred is None or target is None:
            return torch.zeros_like(ae)
        return F.l1_loss(F.relu(pred.detach().float()), target.float(), reduction="none").reshape(ae.numel(), -1).sum(dim=1)

    cls = (c > 0).to(I32) + 2 * (pc > 0).to(I32)
    return ae, se, dist(pred_v, v_target), dist(pred_e, e_target), cls


def si_eval_errors(pred_c, counts, pred_v, v_target, pred_e, e_target, offset, ae, se, ned, eed, cls):
    """The per-pair errors of one evaluation batch written at [offset, offset + B) of the epoch's buffers (float32 ae, se, ned, eed and
    int32 cls of one length): ONE launch of dn_objective_eval under `with ops.objective_fused()` for fp32 / bf16 CUDA tensors, else
    si_eval_errors_composed and five slice copies.  NED / EED run over all positions, no mask.  Nothing is read back."""
    if pred_v is None or v_target is None:
        pred_v = v_target = None
    if pred_e is None or e_target is None:
        pred_e = e_target = None
    B, cap = int(pred_c.numel()), int(ae.numel())
    if offset < 0 or offset + B > cap:
        raise ValueError("si_eval_errors: %d pairs at offset %d do not fit the %d entries of the epoch's buffers" % (B, offset, cap))
    if not (objective_fused_enabled() and si_objective_supported(pred_c, counts, (), pred_v, v_target, pred_e, e_target) and ae.is_cuda):
        outs = launch_tagged("si_eval_composed", lambda: si_eval_errors_composed(pred_c, counts, pred_v, v_target, pred_e, e_target))
        for buf, o in zip((ae, se, ned, eed, cls), outs):
            buf[offset:offset + B] = o
        return
    pc, c = pred_c.detach().reshape(B).contiguous(), counts.reshape(B).contiguous()
    side = lambda p, w: (0, None, None) if p is None else (int(p.numel()) // B, p.detach().reshape(B, -1).contiguous(),  # noqa: E731
                                                           w.reshape(B, -1).contiguous())
    (Lv, pv, wv), (Le, pe, we) = side(pred_v, v_target), side(pred_e, e_target)
    require_gpu(pc, c, pv, wv, pe, we, ae, se, ned, eed, cls)
    dt = lambda t: 0 if t is None else _objective_dt(t)  # noqa: E731
    launch_tagged("si_objective_eval", lambda: check(lib().dn_objective_eval(
        B, ptr(pc), dt(pc), ptr(c), dt(c), Lv, ptr(pv), dt(pv), ptr(wv), dt(wv), Le, ptr(pe), dt(pe), ptr(we), dt(we), int(offset), cap,
        ptr(ae), ptr(se), ptr(ned), ptr(eed), ptr(cls), stream_ptr()), "dn_objective_eval"))
