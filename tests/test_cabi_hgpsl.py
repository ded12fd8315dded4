"""Argument checks of the HGP-SL entry points (dn_hgpsl.hip): every call below is refused on the host, before any launch, with
nothing but NULL / dummy pointers (CPU only); the exported limits equal the ops constants."""
import ctypes
import os

import pytest

P16 = ctypes.c_void_p(16)
NAMES = ["dn_hgpsl_att_grad_f32", "dn_hgpsl_att_slabs", "dn_hgpsl_dinv_f32", "dn_hgpsl_max_features", "dn_hgpsl_max_keys", "dn_hgpsl_pq_f32",
         "dn_hgpsl_score_f32", "dn_hgpsl_structure_bwd_cols_f32", "dn_hgpsl_structure_bwd_edges_f32", "dn_hgpsl_structure_bwd_rows_f32",
         "dn_hgpsl_structure_fwd_f32", "dn_hgpsl_topk_f32", "dn_hgpsl_topk_max_nodes", "dn_hgpsl_wave_keys"]
BIG = 1 << 40


@pytest.fixture(scope="module")
def L():
    from dummynode4graphlearning_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.lib()


def _err(L, rc, text):
    assert rc == -1 and text in L.dn_last_error(), (rc, L.dn_last_error())


def test_the_exports_and_the_class_limits(L):
    from dummynode4graphlearning_amd import _lib, ops
    assert [s for s in _lib.exported_symbols() if s.startswith("dn_hgpsl_")] == NAMES
    assert L.dn_hgpsl_topk_max_nodes() == ops.HGPSL_TOPK_MAX_NODES == 4096
    assert L.dn_hgpsl_wave_keys() == ops.HGPSL_WAVE_KEYS == 64
    assert L.dn_hgpsl_max_keys() == ops.HGPSL_MAX_KEYS == 1024
    assert L.dn_hgpsl_max_features() == ops.HGPSL_MAX_H == 512
    assert L.dn_hgpsl_att_slabs() == ops.HGPSL_ATT_SLABS == 64


def test_dinv_and_score_check_their_arguments(L):
    def dinv(N=10, E=20, out_ptr=P16, out_perm=P16, w=None, out=P16):
        return L.dn_hgpsl_dinv_f32(N, E, out_ptr, out_perm, w, out, None)

    def score(N=10, E=20, H=8, in_ptr=P16, in_perm=P16, src=P16, w=None, dinv=P16, x=P16, out=P16):
        return L.dn_hgpsl_score_f32(N, E, H, in_ptr, in_perm, src, w, dinv, x, out, None)

    for call in (dinv, score):
        for kw in (dict(N=0), dict(N=-1), dict(N=BIG), dict(E=-1), dict(E=1 << 31)):
            _err(L, call(**kw), b"bad sizes")
    for H in (0, -1, 513):
        _err(L, score(H=H), b"1 <= H <= 512 feature columns")
    for name in ("out_ptr", "out"):
        _err(L, dinv(**{name: None}), b"NULL pointer")
    _err(L, dinv(w=P16, out_perm=None), b"NULL pointer")                       # weights need the edge ids
    for name in ("in_ptr", "src", "dinv", "x", "out"):
        _err(L, score(**{name: None}), b"NULL pointer")
    _err(L, score(w=P16, in_perm=None), b"NULL pointer")


def test_topk_checks_its_arguments(L):
    def call(B=3, N=10, Np=8, num_list=2, max_nodes=5, graphs=P16, graph_ptr=P16, pooled_ptr=P16, score=P16, perm=P16, batch=P16, inv=P16):
        return L.dn_hgpsl_topk_f32(B, N, Np, num_list, max_nodes, graphs, graph_ptr, pooled_ptr, score, perm, batch, inv, None)

    for kw in (dict(B=0), dict(B=1 << 31), dict(N=0), dict(N=1 << 31), dict(Np=0), dict(Np=11), dict(num_list=0), dict(num_list=4)):
        _err(L, call(**kw), b"bad sizes")
    for m in (0, -1, 4097):
        _err(L, call(max_nodes=m), b"graph over the class limit")
    for name in ("graphs", "graph_ptr", "pooled_ptr", "score", "perm", "batch", "inv"):
        _err(L, call(**{name: None}), b"NULL pointer")


def test_pq_and_att_grad_check_their_arguments(L):
    def pq(Np=10, H=8, xp=P16, att=P16, p=P16, q=P16):
        return L.dn_hgpsl_pq_f32(Np, H, xp, att, p, q, None)

    def ag(Np=10, H=8, xp=P16, dp=P16, dq=P16, ws=P16, datt=P16):
        return L.dn_hgpsl_att_grad_f32(Np, H, xp, dp, dq, ws, datt, None)

    for call, pointers in ((pq, ("xp", "att", "p", "q")), (ag, ("xp", "dp", "dq", "ws", "datt"))):
        for kw in (dict(Np=0), dict(Np=-3), dict(Np=BIG)):
            _err(L, call(**kw), b"bad sizes")
        for H in (0, 513):
            _err(L, call(H=H), b"1 <= H <= 512 feature columns")
        for name in pointers:
            _err(L, call(**{name: None}), b"NULL pointer")


def test_structure_forward_checks_its_arguments(L):
    def call(B=3, N=10, E=20, Np=8, T=30, num_rows=4, max_keys=5, score=1, rows=P16, pooled_ptr=P16, blk_ptr=P16, batch=P16, perm=P16,
             inv=P16, out_ptr=P16, out_perm=P16, dst=P16, w=None, p=P16, q=P16, blocks=P16):
        return L.dn_hgpsl_structure_fwd_f32(B, N, E, Np, T, num_rows, max_keys, score, rows, pooled_ptr, blk_ptr, batch, perm, inv, out_ptr,
                                            out_perm, dst, w, p, q, 1.0, 0.2, blocks, None)

    for kw in (dict(N=0), dict(E=-1), dict(B=0), dict(Np=0), dict(Np=BIG), dict(T=7), dict(T=1 << 41)):
        _err(L, call(**kw), b"bad sizes")
    for n in (0, 9):
        _err(L, call(num_rows=n), b"bad list")
    for m in (0, 1025):
        _err(L, call(max_keys=m), b"key count over the class limit")
    for s in (-1, 2):
        _err(L, call(score=s), b"bad score function")
    for name in ("rows", "pooled_ptr", "blk_ptr", "batch", "perm", "inv", "out_ptr", "dst", "p", "q", "blocks"):
        _err(L, call(**{name: None}), b"NULL pointer")
    _err(L, call(w=P16, out_perm=None), b"NULL pointer")


def test_structure_backward_checks_its_arguments(L):
    def rows(B=3, Np=8, T=30, num_rows=4, score=0, rows=P16, pooled_ptr=P16, blk_ptr=P16, batch=P16, p=P16, q=P16, blocks=P16, dblocks=P16,
             dl=P16, dp=P16, rterm=P16):
        return L.dn_hgpsl_structure_bwd_rows_f32(B, Np, T, num_rows, score, rows, pooled_ptr, blk_ptr, batch, p, q, 0.2, blocks, dblocks, dl,
                                                 dp, rterm, None)

    def cols(B=3, Np=8, T=30, num_rows=4, rows=P16, pooled_ptr=P16, blk_ptr=P16, batch=P16, dl=P16, dq=P16):
        return L.dn_hgpsl_structure_bwd_cols_f32(B, Np, T, num_rows, rows, pooled_ptr, blk_ptr, batch, dl, dq, None)

    def edges(B=3, N=10, E=20, Np=8, T=30, score=0, src=P16, dst=P16, inv=P16, pooled_ptr=P16, blk_ptr=P16, batch=P16, blocks=P16,
              dblocks=P16, rterm=P16, dw=P16):
        return L.dn_hgpsl_structure_bwd_edges_f32(B, N, E, Np, T, score, src, dst, inv, pooled_ptr, blk_ptr, batch, blocks, dblocks, rterm,
                                                  0.5, dw, None)

    for call in (rows, cols, edges):
        for kw in (dict(B=0), dict(Np=0), dict(T=7), dict(T=1 << 41)):
            _err(L, call(**kw), b"bad sizes")
    for call in (rows, cols):
        for n in (0, 9):
            _err(L, call(num_rows=n), b"bad list")
    for call in (rows, edges):
        _err(L, call(score=3), b"bad score function")
    for kw in (dict(N=0), dict(E=0), dict(E=1 << 31)):
        _err(L, edges(**kw), b"bad sizes")
    for name in ("rows", "pooled_ptr", "blk_ptr", "batch", "p", "q", "blocks", "dblocks", "dl", "dp", "rterm"):
        _err(L, rows(**{name: None}), b"NULL pointer")
    for name in ("rows", "pooled_ptr", "blk_ptr", "batch", "dl", "dq"):
        _err(L, cols(**{name: None}), b"NULL pointer")
    for name in ("src", "dst", "inv", "pooled_ptr", "blk_ptr", "batch", "blocks", "dblocks", "rterm", "dw"):
        _err(L, edges(**{name: None}), b"NULL pointer")
