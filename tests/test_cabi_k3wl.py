"""The dn_k3wl_* entry points (dn_k3wl.hip) check their arguments on the host before any launch: NULL pointers, non-positive sizes
and sizes past int32 are refused with -1 and a message (CPU only: nothing here reaches a launch)."""
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


def test_entry_points_are_the_k3wl_ones():
    from dummynode4graphlearning_amd import _lib
    assert [s for s in _lib.exported_symbols() if s.startswith("dn_k3wl_")] == [
        "dn_k3wl_close_u64", "dn_k3wl_global_u64", "dn_k3wl_init_u64", "dn_k3wl_local_u64", "dn_k3wl_max_entries", "dn_k3wl_max_nodes"]
    assert sorted(s for s in _lib._SIGS if s.startswith("dn_k3wl_")) == sorted(s for s in _lib.exported_symbols() if s.startswith("dn_k3wl_"))


def test_limits(L):
    n, cap = L.dn_k3wl_max_nodes(), L.dn_k3wl_max_entries()
    assert n == 64                                                          # a fibre in one wavefront, an adjacency row in 64 bits
    assert cap >= 64 and cap & (cap - 1) == 0 and 3 * 8 * 2 * cap <= 65536  # three lists of up to 2 cap entries in LDS
    d = cap + 1                                                             # a hub of cap + 1 neighbours passes the item bound at H = 1
    assert 2 * ((d + 1) + 2 * d + 3 * d * (d - 1)) < 1000000


def test_init_checks_its_arguments(L):
    def call(N=10, T=100, conn=0, tv=P16, tw=P16, tu=P16, ptr=P16, nbr=P16, nl=None, out=P32):
        return L.dn_k3wl_init_u64(N, T, conn, tv, tw, tu, ptr, nbr, nl, out, None)

    for kw in (dict(N=0), dict(N=-3), dict(T=0), dict(T=-1), dict(N=BIG), dict(T=BIG)):
        _refused(L, call(**kw), b"bad sizes")
    for kw in (dict(tv=None), dict(tw=None), dict(tu=None), dict(ptr=None), dict(nbr=None), dict(out=None)):
        _refused(L, call(**kw), b"NULL pointer")


def test_local_checks_its_arguments(L):
    def call(N=10, T=100, n=100, items=P16, group=8, lds=0, conn=0, tv=P16, tw=P16, tu=P16, ng=P16, node_ptr=P16, tuple_ptr=P16, ptr=P16,
             nbr=P16, key=P16, slot=P16, cin=P16, cout=P32):
        return L.dn_k3wl_local_u64(N, T, n, items, group, lds, conn, tv, tw, tu, ng, node_ptr, tuple_ptr, ptr, nbr, key, slot, cin, cout, None)

    for kw in (dict(N=0), dict(N=-3), dict(T=0), dict(n=0), dict(n=-1), dict(N=BIG), dict(T=BIG, n=1), dict(T=BIG, n=BIG), dict(n=101)):
        _refused(L, call(**kw), b"bad sizes")
    for kw in (dict(tv=None), dict(tw=None), dict(tu=None), dict(ng=None), dict(node_ptr=None), dict(tuple_ptr=None), dict(ptr=None),
               dict(nbr=None), dict(cin=None), dict(cout=None), dict(items=None, n=5), dict(conn=1, key=None), dict(conn=1, slot=None)):
        _refused(L, call(**kw), b"NULL pointer")
    _refused(L, call(group=16), b"group must be 8, 64 or 0")
    _refused(L, call(cout=P16), b"must not alias")
    cap = L.dn_k3wl_max_entries()
    for lds in (0, -8, 96, 4 * cap):
        _refused(L, call(group=0, lds=lds), b"lds_entries must be a power of two")


def test_global_checks_its_arguments(L):
    def call(B=10, T=100, n=10, graphs=P16, fib=P16, fibres=300, group=8, malkin=0, node_ptr=P16, tuple_ptr=P16, bits=P16, cin=P16, work=P48):
        return L.dn_k3wl_global_u64(B, T, n, graphs, fib, fibres, group, malkin, node_ptr, tuple_ptr, bits, cin, work, None)

    for kw in (dict(B=0), dict(B=-1), dict(T=0), dict(n=0), dict(n=-1), dict(B=BIG), dict(T=BIG), dict(B=BIG, n=BIG), dict(n=11),
               dict(fibres=0), dict(fibres=-1), dict(fibres=BIG)):
        _refused(L, call(**kw), b"bad sizes")
    for group in (0, -8, 4, 24, 128):
        _refused(L, call(group=group), b"group must be 8, 16, 32 or 64")
    for kw in (dict(graphs=None), dict(fib=None), dict(node_ptr=None), dict(tuple_ptr=None), dict(cin=None), dict(work=None),
               dict(malkin=1, bits=None)):
        _refused(L, call(**kw), b"NULL pointer")
    _refused(L, call(work=P16), b"must not alias")


def test_close_checks_its_arguments(L):
    def call(N=10, T=100, malkin=0, tv=P16, tw=P16, tu=P16, ng=P16, node_ptr=P16, ptr=P16, cin=P16, work=P48, cout=P32):
        return L.dn_k3wl_close_u64(N, T, malkin, tv, tw, tu, ng, node_ptr, ptr, cin, work, cout, None)

    for kw in (dict(N=0), dict(N=-3), dict(T=0), dict(T=-1), dict(N=BIG), dict(T=BIG)):
        _refused(L, call(**kw), b"bad sizes")
    for kw in (dict(tv=None), dict(tw=None), dict(tu=None), dict(ng=None), dict(node_ptr=None), dict(ptr=None), dict(cin=None),
               dict(work=None), dict(cout=None)):
        _refused(L, call(**kw), b"NULL pointer")
    for kw in (dict(cout=P16), dict(work=P16), dict(work=P32)):
        _refused(L, call(**kw), b"must not alias")
