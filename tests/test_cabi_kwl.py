"""The dn_kwl_* entry points (dn_kwl.hip) check their arguments on the host before any launch: NULL pointers, non-positive sizes and
sizes past int32 are refused with -1 and a message (CPU only: nothing here reaches a launch)."""
import ctypes
import os

import pytest

P16 = ctypes.c_void_p(16)
P32 = ctypes.c_void_p(32)
P48 = ctypes.c_void_p(48)
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


def test_entry_points_are_the_kwl_ones():
    from dummynode4graphlearning_amd import _lib
    assert [s for s in _lib.exported_symbols() if s.startswith("dn_kwl_")] == [
        "dn_kwl_global_u64", "dn_kwl_init_u64", "dn_kwl_local_u64", "dn_kwl_max_entries", "dn_kwl_max_nodes"]


def test_limits(L):
    n, cap = L.dn_kwl_max_nodes(), L.dn_kwl_max_entries()
    assert n >= 64 and n & (n - 1) == 0 and n <= 255                       # (a source index is one byte, 255 the padding)
    assert 9 * n * n + 16 * n <= 160 * 1024                                # keys, sources and adjacency rows within the CU's LDS
    assert cap >= 64 and cap & (cap - 1) == 0 and 2 * 8 * cap <= 65536


def test_init_checks_its_arguments(L):
    def call(N=10, T=100, tv=P16, tw=P16, ptr=P16, nbr=P16, nl=None, el=None, out=P32):
        return L.dn_kwl_init_u64(N, T, tv, tw, ptr, nbr, nl, el, out, None)

    for kw in (dict(N=0), dict(N=-3), dict(T=0), dict(T=-1), dict(N=BIG), dict(T=BIG)):
        _refused(L, call(**kw), b"bad sizes")
    for kw in (dict(tv=None), dict(tw=None), dict(ptr=None), dict(nbr=None), dict(out=None)):
        _refused(L, call(**kw), b"NULL pointer")


def test_local_checks_its_arguments(L):
    def call(N=10, T=100, n=100, tuples=P16, group=8, lds=0, conn=0, tv=P16, tw=P16, row=P16, first=P16, ptr=P16, nbr=P16, cin=P16, cout=P32):
        return L.dn_kwl_local_u64(N, T, n, tuples, group, lds, conn, tv, tw, row, first, ptr, nbr, cin, cout, None)

    for kw in (dict(N=0), dict(N=-3), dict(T=0), dict(n=0), dict(n=-1), dict(N=BIG), dict(T=BIG, n=1), dict(T=BIG, n=BIG), dict(n=101)):
        _refused(L, call(**kw), b"bad sizes")
    for kw in (dict(tv=None), dict(tw=None), dict(row=None), dict(first=None), dict(ptr=None), dict(nbr=None), dict(cin=None),
               dict(cout=None), dict(tuples=None, n=5)):
        _refused(L, call(**kw), b"NULL pointer")
    _refused(L, call(group=16), b"group must be 8, 64 or 0")
    _refused(L, call(cout=P16), b"must not alias")
    cap = L.dn_kwl_max_entries()
    for lds in (0, -8, 96, 2 * cap):
        _refused(L, call(group=0, lds=lds), b"lds_entries must be a power of two")


def test_global_checks_its_arguments(L):
    def call(B=10, T=100, n=10, graphs=P16, lds=8, malkin=0, node_ptr=P16, tuple_ptr=P16, ptr=P16, nbr=P16, cin=P16, cout=P32, work=P48):
        return L.dn_kwl_global_u64(B, T, n, graphs, lds, malkin, node_ptr, tuple_ptr, ptr, nbr, cin, cout, work, None)

    for kw in (dict(B=0), dict(B=-1), dict(T=0), dict(n=0), dict(n=-1), dict(B=BIG), dict(T=BIG), dict(B=BIG, n=BIG), dict(n=11)):
        _refused(L, call(**kw), b"bad sizes")
    for lds in (0, -8, 96, 2 * L.dn_kwl_max_nodes()):
        _refused(L, call(lds=lds), b"lds_nodes must be a power of two")
    for kw in (dict(graphs=None), dict(node_ptr=None), dict(tuple_ptr=None), dict(ptr=None), dict(nbr=None), dict(cin=None), dict(cout=None),
               dict(work=None)):
        _refused(L, call(**kw), b"NULL pointer")
    for kw in (dict(cout=P16), dict(work=P16), dict(work=P32)):
        _refused(L, call(**kw), b"must not alias")
