"""Argument checks of the ragged attention and window pooling entry points (dn_seg_attn.hip): every call below is refused on the host,
before any launch, with nothing but NULL / dummy pointers (CPU only)."""
import ctypes
import os

import pytest

P16 = ctypes.c_void_p(16)
NAMES = ["dn_seg_attn_bwd_kv_f32", "dn_seg_attn_bwd_q_f32", "dn_seg_attn_fwd_f32", "dn_seg_attn_max_keys", "dn_seg_attn_wave_keys",
         "dn_seg_window_pool_bwd_f32", "dn_seg_window_pool_fwd_f32"]


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
    assert [s for s in _lib.exported_symbols() if s.startswith("dn_seg_")] == NAMES
    assert L.dn_seg_attn_max_keys() == ops.SEG_ATTN_MAX_KEYS == 1024
    assert L.dn_seg_attn_wave_keys() == ops.SEG_ATTN_WAVE_KEYS == 64


def _attn_calls(L):
    def fwd(B=2, Nq=5, Nk=7, H=64, heads=4, max_q=3, max_k=4, score=0, q_ptr=P16, k_ptr=P16, q=P16, k=P16, v=P16, out=P16, stat=P16):
        return L.dn_seg_attn_fwd_f32(B, Nq, Nk, H, heads, max_q, max_k, score, q_ptr, k_ptr, None, None, q, k, v, 0.25, out, stat, None)

    def bwd_q(B=2, Nq=5, Nk=7, H=64, heads=4, max_q=3, max_k=4, score=0, q_ptr=P16, k_ptr=P16, q=P16, k=P16, v=P16, stat=P16, dout=P16,
              dq=P16, rterm=P16):
        return L.dn_seg_attn_bwd_q_f32(B, Nq, Nk, H, heads, max_q, max_k, score, q_ptr, k_ptr, None, None, q, k, v, 0.25, stat, dout, dq,
                                       rterm, None)

    def bwd_kv(B=2, Nq=5, Nk=7, H=64, heads=4, max_q=3, max_k=4, score=0, q_ptr=P16, k_ptr=P16, q=P16, k=P16, v=P16, stat=P16, rterm=P16,
               dout=P16, dk=P16, dv=P16):
        return L.dn_seg_attn_bwd_kv_f32(B, Nq, Nk, H, heads, max_q, max_k, score, q_ptr, k_ptr, None, None, q, k, v, 0.25, stat, rterm,
                                        dout, dk, dv, None)
    return {"fwd": (fwd, ("q_ptr", "k_ptr", "q", "k", "v", "out", "stat")),
            "bwd_q": (bwd_q, ("q_ptr", "k_ptr", "q", "k", "v", "stat", "dout", "dq", "rterm")),
            "bwd_kv": (bwd_kv, ("q_ptr", "k_ptr", "q", "k", "v", "stat", "rterm", "dout", "dk", "dv"))}


@pytest.mark.parametrize("which", ["fwd", "bwd_q", "bwd_kv"])
def test_attention_checks_its_arguments(L, which):
    call, pointers = _attn_calls(L)[which]
    for kw in (dict(B=0), dict(Nq=0), dict(Nk=0), dict(Nq=-3), dict(B=1 << 31)):
        _err(L, call(**kw), b"bad sizes")
    for heads in (0, 3, 16):
        _err(L, call(heads=heads), b"heads must be 1, 2, 4 or 8")
    _err(L, call(H=0), b"hidden % heads == 0")
    _err(L, call(H=257, heads=1), b"1 <= hidden <= 256")
    _err(L, call(H=66, heads=4), b"hidden % heads == 0")
    _err(L, call(H=48, heads=4), b"the head width hidden / heads must be a power of two")
    _err(L, call(max_k=0), b"key count over the class limit")
    _err(L, call(max_k=1025), b"key count over the class limit")
    _err(L, call(max_q=0), b"bad max_q")
    _err(L, call(score=2), b"bad score function")
    for name in pointers:
        _err(L, call(**{name: None}), b"NULL pointer")


def test_window_pool_checks_its_arguments(L):
    def fwd(B=2, N=9, D=8, mem_len=4, mode=0, ptr=P16, rows=P16, mem=P16, mask=P16, arg=None, span=P16):
        return L.dn_seg_window_pool_fwd_f32(B, N, D, mem_len, mode, ptr, None, rows, mem, mask, arg, span, None)

    def bwd(B=2, N=9, D=8, mem_len=4, mode=0, ptr=P16, span=P16, arg=None, dmem=P16, drows=P16):
        return L.dn_seg_window_pool_bwd_f32(B, N, D, mem_len, mode, ptr, None, span, arg, dmem, drows, None)

    for call, pointers in ((fwd, ("ptr", "rows", "mem", "mask", "span")), (bwd, ("ptr", "span", "dmem", "drows"))):
        for kw in (dict(B=0), dict(N=0), dict(D=0), dict(N=1 << 40)):
            _err(L, call(**kw), b"bad sizes")
        _err(L, call(mem_len=0), b"1 <= mem_len <= 64")
        _err(L, call(mem_len=65), b"1 <= mem_len <= 64")
        _err(L, call(mode=3), b"bad mode")
        _err(L, call(mode=-1), b"bad mode")
        _err(L, call(mode=2), b"max needs the arg buffer")
        for name in pointers:
            _err(L, call(**{name: None}), b"NULL pointer")
