"""Every dn_eseq_* entry point refuses bad arguments on the host, before any launch, with a message in dn_last_error() (CPU only):
NULL pointers, non-positive sizes, C not a multiple of 16 or above 128, k outside 2 .. 5, padding above k // 2."""
import ctypes
import os

import pytest

P16 = ctypes.c_void_p(16)


@pytest.fixture(scope="module")
def L():
    from dummynode4graphlearning_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.lib()


def _fwd(L, B=2, Ln=8, C=16, k=3, p=1, act=1, res=0, ptrs=None):
    ptrs = [P16] * 8 if ptrs is None else ptrs
    return L.dn_eseq_conv_pool_fwd_f32(B, Ln, C, k, p, act, 0.2, res, *ptrs, None)


def _dconv(L, B=2, Ln=8, C=16, k=3, p=1, act=1, ptrs=None):
    return L.dn_eseq_dconv_f32(B, Ln, C, k, p, act, 0.2, *([P16] * 4 if ptrs is None else ptrs), None)


def _dgrad(L, B=2, Ln=8, C=16, k=3, p=1, res=0, ptrs=None):
    return L.dn_eseq_dgrad_f32(B, Ln, C, k, p, res, *([P16] * 6 if ptrs is None else ptrs), None)


def _wgrad(L, B=2, Ln=8, C=16, k=3, p=1, G=4, ptrs=None):
    ptrs = [P16] * 6 if ptrs is None else ptrs
    return L.dn_eseq_wgrad_f32(B, Ln, C, k, p, *ptrs[:4], G, *ptrs[4:], None)


SHAPED = [_fwd, _dconv, _dgrad, _wgrad]
BAD_SHAPES = [(dict(B=0), b"bad sizes"), (dict(B=-3), b"bad sizes"), (dict(Ln=0), b"bad sizes"), (dict(B=70000), b"bad sizes"),
              (dict(C=24), b"multiple of 16"), (dict(C=0), b"multiple of 16"), (dict(C=144), b"multiple of 16"),
              (dict(k=1), b"k must be in 2 .. 5"), (dict(k=6), b"k must be in 2 .. 5"), (dict(k=3, p=2), b"padding must be in"),
              (dict(k=2, p=-1), b"padding must be in"), (dict(k=5, p=0, Ln=8), b"too short")]


@pytest.mark.parametrize("call", SHAPED, ids=["fwd", "dconv", "dgrad", "wgrad"])
def test_shapes_are_checked_before_any_launch(L, call):
    for kw, msg in BAD_SHAPES:
        assert call(L, **kw) == -1 and msg in L.dn_last_error(), (kw, L.dn_last_error())


def test_null_pointers_and_flags(L):
    for call, n in ((_fwd, 8), (_dconv, 4), (_wgrad, 6)):
        for i in range(n):
            ptrs = [P16] * n
            ptrs[i] = None
            assert call(L, ptrs=ptrs) == -1 and b"NULL pointer" in L.dn_last_error(), (call.__name__, i)
    for i in (0, 2, 3, 4, 5):                                                # (dy may be NULL without the residual)
        ptrs = [P16] * 6
        ptrs[i] = None
        assert _dgrad(L, ptrs=ptrs) == -1 and b"NULL pointer" in L.dn_last_error(), i
    assert _dgrad(L, res=1, ptrs=[P16, None, P16, P16, P16, P16]) == -1 and b"NULL pointer" in L.dn_last_error()
    assert _fwd(L, act=3) == -1 and b"act must be" in L.dn_last_error()
    assert _dconv(L, act=-1) == -1 and b"act must be" in L.dn_last_error()
    assert _fwd(L, k=2, p=1, res=1) == -1 and b"keeps the length" in L.dn_last_error()
    assert _dgrad(L, k=2, p=1, res=1) == -1 and b"keeps the length" in L.dn_last_error()
    assert _wgrad(L, G=0) == -1 and b"num_slices" in L.dn_last_error()


def test_combine_and_filter_check_their_arguments(L):
    comb = L.dn_eseq_wgrad_combine_f32
    assert comb(24, 3, 4, P16, P16, P16, P16, None) == -1 and b"multiple of 16" in L.dn_last_error()
    assert comb(256, 3, 4, P16, P16, P16, P16, None) == -1 and b"multiple of 16" in L.dn_last_error()
    assert comb(16, 6, 4, P16, P16, P16, P16, None) == -1 and b"k must be in 2 .. 5" in L.dn_last_error()
    assert comb(16, 3, 0, P16, P16, P16, P16, None) == -1 and b"num_slices" in L.dn_last_error()
    for i in range(4):
        ptrs = [P16] * 4
        ptrs[i] = None
        assert comb(16, 3, 4, *ptrs, None) == -1 and b"NULL pointer" in L.dn_last_error()
    filt = L.dn_eseq_filter_gate_i64
    assert L.dn_eseq_filter_max_labels() == 4096
    for B, Lp, Lg in ((0, 4, 4), (2, 0, 4), (2, 4, 0), (-1, 4, 4), (70000, 4, 4)):
        assert filt(B, Lp, Lg, *([P16] * 7), None) == -1 and b"bad sizes" in L.dn_last_error()
    for i in range(7):
        ptrs = [P16] * 7
        ptrs[i] = None
        assert filt(2, 4, 4, *ptrs, None) == -1 and b"NULL pointer" in L.dn_last_error()
