"""The dn_eseq_rnn_* entry points refuse bad arguments on the host, before any launch, with a message in dn_last_error() (CPU only):
NULL pointers, non-positive sizes, a hidden width outside {16, 32, 48, 64}, a direction count other than 1 or 2, an unknown cell, a
batch beyond the 32-bit bound; the buffers a cell does not need may be NULL."""
import ctypes
import os

import pytest

P16 = ctypes.c_void_p(16)
FWD = ("P", "whh", "bhn", "x0", "gate", "lo", "y", "h", "saved")
BWD = ("dy", "gate", "lo", "whh", "h", "saved", "dP", "dhn")


@pytest.fixture(scope="module")
def L():
    from dummynode4graphlearning_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.lib()


def _fwd(L, B=2, Ln=8, Hd=16, D=1, cell=0, res=0, **null):
    return L.dn_eseq_rnn_fwd_f32(B, Ln, Hd, D, cell, res, *[None if null.get(n) else P16 for n in FWD], None)


def _bwd(L, B=2, Ln=8, Hd=16, D=1, cell=0, **null):
    return L.dn_eseq_rnn_bwd_f32(B, Ln, Hd, D, cell, *[None if null.get(n) else P16 for n in BWD], None)


BAD_SHAPES = [(dict(B=0), b"bad sizes"), (dict(B=-3), b"bad sizes"), (dict(Ln=0), b"bad sizes"), (dict(B=70000), b"bad sizes"),
              (dict(Hd=8), b"16, 32, 48 or 64"), (dict(Hd=24), b"16, 32, 48 or 64"), (dict(Hd=128), b"16, 32, 48 or 64"),
              (dict(Hd=0), b"16, 32, 48 or 64"), (dict(D=0), b"1 or 2 directions"), (dict(D=3), b"1 or 2 directions"),
              (dict(cell=-1), b"cell must be"), (dict(cell=3), b"cell must be"),
              (dict(B=65535, Ln=4096, Hd=64, D=2), b"below 2^31")]


@pytest.mark.parametrize("call", [_fwd, _bwd], ids=["fwd", "bwd"])
def test_shapes_are_checked_before_any_launch(L, call):
    for kw, msg in BAD_SHAPES:
        assert call(L, **kw) == -1 and msg in L.dn_last_error(), (kw, L.dn_last_error())


def test_null_pointers(L):
    for cell in (0, 1, 2):
        for n in ("P", "whh", "gate", "lo", "y", "h"):
            assert _fwd(L, cell=cell, **{n: True}) == -1 and b"NULL pointer" in L.dn_last_error(), (cell, n)
        for n in ("dy", "gate", "lo", "whh", "h", "dP"):
            assert _bwd(L, cell=cell, **{n: True}) == -1 and b"NULL pointer" in L.dn_last_error(), (cell, n)
    assert _fwd(L, cell=1, bhn=True) == -1 and b"b_hn" in L.dn_last_error()
    assert _fwd(L, cell=0, saved=True) == -1 and b"saved buffer" in L.dn_last_error()
    assert _fwd(L, cell=1, saved=True) == -1 and b"saved buffer" in L.dn_last_error()
    assert _bwd(L, cell=0, saved=True) == -1 and b"saved buffer" in L.dn_last_error()
    assert _bwd(L, cell=1, dhn=True) == -1 and b"dhn" in L.dn_last_error()
    assert _fwd(L, res=1, x0=True) == -1 and b"residual needs x0" in L.dn_last_error()


def test_saved_values_per_unit(L):
    assert [L.dn_eseq_rnn_saved_per_unit(c) for c in (0, 1, 2)] == [5, 4, 0]
    assert L.dn_eseq_rnn_saved_per_unit(3) == -1 and L.dn_eseq_rnn_saved_per_unit(-1) == -1
