"""The dn_txl_* entry points refuse bad arguments on the host, before any launch, with a message in dn_last_error() (CPU only): NULL
pointers, non-positive sizes, a head width outside {16, 32, 64}, a segment length outside {16, 32, 48, 64}, a memory that is no
multiple of 16 or makes the window longer than 128, a sequence that is no whole number of segments, a position table shorter than the
window, sizes beyond the 32-bit bound; the memory buffers may be NULL when there is no memory."""
import ctypes
import os

import pytest

P16 = ctypes.c_void_p(16)
FWD = ("q", "k", "v", "k_mem", "v_mem", "rk", "r_w_bias", "r_r_bias", "out", "stats")
BWD = ("dout", "q", "k", "v", "k_mem", "v_mem", "rk", "r_w_bias", "r_r_bias", "out", "stats", "dq_ac", "dq_bd", "dk", "dv", "k_part",
       "v_part", "rk_part")
FOLD = ("k_part", "v_part", "dk_mem", "dv_mem")
MEM_ONLY = ("k_mem", "v_mem", "k_part", "v_part")


@pytest.fixture(scope="module")
def L():
    from dummynode4graphlearning_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.lib()


def _ptrs(names, null):
    return [None if null.get(n) else P16 for n in names]


def _fwd(L, B=2, Lp=128, n=1, D=16, seg=64, mem=64, P=128, **null):
    return L.dn_txl_attn_fwd_f32(B, Lp, n, D, seg, mem, P, 0.25, *_ptrs(FWD, null), None)


def _bwd(L, B=2, Lp=128, n=1, D=16, seg=64, mem=64, P=128, **null):
    return L.dn_txl_attn_bwd_f32(B, Lp, n, D, seg, mem, P, 0.25, *_ptrs(BWD, null), None)


def _fold(L, B=2, Lp=128, n=1, D=16, seg=64, mem=64, P=128, **null):
    return L.dn_txl_fold_mem_f32(B, Lp, n, D, seg, mem, *_ptrs(FOLD, null), None)


def _reduce(L, B=2, Lp=128, n=1, D=16, seg=64, mem=64, P=128, **null):
    return L.dn_txl_reduce_rk_f32(B, Lp, n, D, seg, mem, P, *_ptrs(("rk_part", "drk"), null), None)


BAD_SHAPES = [(dict(B=0), b"bad sizes"), (dict(B=-3), b"bad sizes"), (dict(Lp=0), b"bad sizes"), (dict(n=0), b"bad sizes"),
              (dict(D=8), b"16, 32 or 64"), (dict(D=48), b"16, 32 or 64"), (dict(D=128), b"16, 32 or 64"), (dict(D=0), b"16, 32 or 64"),
              (dict(seg=0), b"segment length"), (dict(seg=24, Lp=48), b"segment length"), (dict(seg=128, Lp=128), b"segment length"),
              (dict(mem=-16), b"memory length"), (dict(mem=20), b"memory length"), (dict(mem=80), b"memory length"),
              (dict(seg=48, mem=96, Lp=96, P=144), b"memory length"), (dict(Lp=100), b"no multiple of the segment length"),
              (dict(n=70000, B=1, Lp=64), b"at most 65535"), (dict(B=40000, Lp=4096, n=1, D=64), b"below 2^31"),
              (dict(B=2 ** 31, Lp=64), b"below 2^31")]


@pytest.mark.parametrize("call", [_fwd, _bwd, _fold, _reduce], ids=["fwd", "bwd", "fold", "reduce"])
def test_shapes_are_checked_before_any_launch(L, call):
    for kw, msg in BAD_SHAPES:
        assert call(L, **kw) == -1 and msg in L.dn_last_error(), (kw, L.dn_last_error())


@pytest.mark.parametrize("call", [_fwd, _bwd, _reduce], ids=["fwd", "bwd", "reduce"])
def test_the_position_table_must_cover_the_window(L, call):
    assert call(L, P=127) == -1 and b"rk needs seg + mem = 128 rows" in L.dn_last_error()
    assert call(L, P=0) == -1 and b"bad sizes" in L.dn_last_error()
    assert call(L, seg=16, mem=16, Lp=32, P=31) == -1 and b"rk needs seg + mem = 32 rows" in L.dn_last_error()


def test_null_pointers(L):
    for names, call in ((FWD, _fwd), (BWD, _bwd)):
        for n in names:
            if n in MEM_ONLY:
                assert call(L, **{n: True}) == -1 and b"a memory needs" in L.dn_last_error(), n
            else:
                assert call(L, **{n: True}) == -1 and b"NULL pointer" in L.dn_last_error(), n
                assert call(L, mem=0, P=64, **{n: True}) == -1 and b"NULL pointer" in L.dn_last_error(), n
    for n in FOLD:
        assert _fold(L, **{n: True}) == -1 and b"NULL pointer" in L.dn_last_error(), n
    assert _fold(L, mem=0) == -1 and b"no memory to fold" in L.dn_last_error()
    for n in ("rk_part", "drk"):
        assert _reduce(L, **{n: True}) == -1 and b"NULL pointer" in L.dn_last_error(), n
