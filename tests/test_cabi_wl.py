"""The dn_wl_* entry points (dn_wl.hip) check their arguments on the host before any launch: NULL pointers, non-positive sizes and
sizes past int32 are refused with -1 and a message (CPU only: nothing here reaches a launch)."""
import ctypes
import os

import pytest

P16 = ctypes.c_void_p(16)
P32 = ctypes.c_void_p(32)
BIG = 1 << 31


@pytest.fixture(scope="module")
def L():
    from dummynode4graphlearning_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.lib()


def _refused(L, rc, msg):
    assert rc == -1 and msg in L.dn_last_error(), L.dn_last_error()


def test_entry_points_are_the_wl_ones():
    from dummynode4graphlearning_amd import _lib
    assert [s for s in _lib.exported_symbols() if s.startswith("dn_wl_")] == [
        "dn_wl_fold_u64", "dn_wl_gram_i64", "dn_wl_gram_tile", "dn_wl_max_entries", "dn_wl_max_steps", "dn_wl_refine_u64"]


def test_limits(L):
    cap = L.dn_wl_max_entries()
    assert cap >= 64 and cap & (cap - 1) == 0 and 8 * cap <= 65536
    assert L.dn_wl_gram_tile() ** 2 == 256 and L.dn_wl_max_steps() >= 6 and 2048 * L.dn_wl_max_steps() <= 65536


def test_refine_checks_its_arguments(L):
    def call(N=10, n=10, nodes=P16, group=8, lds=0, ptr=P16, nbr=P16, el=None, cin=P16, cout=P32):
        return L.dn_wl_refine_u64(N, n, nodes, group, lds, ptr, nbr, el, cin, cout, None)

    for kw in (dict(N=0), dict(N=-3), dict(n=0), dict(n=-1), dict(N=BIG, n=1), dict(N=BIG, n=BIG), dict(n=11)):
        _refused(L, call(**kw), b"bad sizes")
    for kw in (dict(ptr=None), dict(nbr=None), dict(cin=None), dict(cout=None), dict(nodes=None, n=5)):
        _refused(L, call(**kw), b"NULL pointer")
    _refused(L, call(group=16), b"group must be 8, 64 or 0")
    _refused(L, call(cout=P16), b"must not alias")
    cap = L.dn_wl_max_entries()
    for lds in (0, -8, 96, 2 * cap):
        _refused(L, call(group=0, lds=lds), b"lds_entries must be a power of two")


def test_fold_checks_its_arguments(L):
    def call(N=10, n=10, nodes=P16, seg=P16, ent=P16, cin=P16, cout=P32):
        return L.dn_wl_fold_u64(N, n, nodes, seg, ent, cin, cout, None)

    for kw in (dict(N=0), dict(n=0), dict(n=-1), dict(N=BIG, n=1), dict(n=11)):
        _refused(L, call(**kw), b"bad sizes")
    for kw in (dict(seg=None), dict(cin=None), dict(cout=None), dict(nodes=None, n=5)):
        _refused(L, call(**kw), b"NULL pointer")
    _refused(L, call(cout=P16), b"must not alias")


def test_gram_checks_its_arguments(L):
    def call(B=5, S=3, use_min=0, fptr=P16, col=P16, cnt=P16, step=P16, out=P16):
        return L.dn_wl_gram_i64(B, S, use_min, fptr, col, cnt, step, out, None)

    for kw in (dict(B=0), dict(B=-1), dict(B=BIG), dict(B=65536 * L.dn_wl_gram_tile())):
        _refused(L, call(**kw), b"bad sizes")
    for S in (0, -1, L.dn_wl_max_steps() + 1):
        _refused(L, call(S=S), b"steps")
    for kw in (dict(fptr=None), dict(col=None), dict(cnt=None), dict(step=None), dict(out=None)):
        _refused(L, call(**kw), b"NULL pointer")
