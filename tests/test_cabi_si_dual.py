"""Argument checks of the dual message-passing entry points (dn_dual.hip): every call below is refused on the host, before any
launch, with nothing but NULL / dummy pointers (CPU only)."""
import ctypes
import os

import pytest

P16 = ctypes.c_void_p(16)
SUFFIXES = ("f32", "bf16")
NAMES = ("dn_dual_agg", "dn_dual_agg_bwd_edge", "dn_dual_agg_bwd_node", "dn_dual_edge_update", "dn_dual_edge_update_bwd",
         "dn_sie_pool_sum")


@pytest.fixture(scope="module")
def L():
    from dummynode4graphlearning_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.lib()


def _err(L, rc, text):
    assert rc == -1 and text in L.dn_last_error(), (rc, L.dn_last_error())


def test_the_new_exports_keep_out_of_the_si_namespace():
    from dummynode4graphlearning_amd import _lib
    syms = _lib.exported_symbols()
    for n in NAMES:
        for s in SUFFIXES:
            assert "%s_%s" % (n, s) in syms
    assert len([s for s in syms if s.startswith("dn_si_")]) == 16
    assert len([s for s in syms if s.startswith(("dn_dual_", "dn_sie_"))]) == 12


@pytest.mark.parametrize("sfx", SUFFIXES)
def test_dual_agg_checks_its_arguments(L, sfx):
    fn = getattr(L, "dn_dual_agg_" + sfx)
    call = lambda mode=0, N=10, E=20, H=64, U=10, units=P16, perm=P16, src=P16, ef=P16, x=P16, out=P16, part=None, P=0: fn(  # noqa: E731
        mode, N, E, H, U, units, perm, src, None, None, ef, x, out, 0, part, P, None)
    _err(L, call(mode=3), b"bad mode")
    _err(L, call(H=0), b"1 <= H <= 256")
    _err(L, call(H=257), b"1 <= H <= 256")
    _err(L, call(N=1 << 30), b"N < 2^30")
    _err(L, call(units=None), b"NULL unit table")
    _err(L, call(perm=None), b"NULL pointer")
    _err(L, call(ef=None), b"NULL pointer")
    _err(L, call(out=None), b"NULL pointer")
    _err(L, call(mode=1, x=None), b"sub / mult need src and x")
    _err(L, call(mode=2, src=None), b"sub / mult need src and x")
    _err(L, call(P=3), b"partial slots without a partial buffer")
    _err(L, call(P=11, part=P16), b"bad unit counts")
    assert call(U=0) == 0                                                   # nothing to do


@pytest.mark.parametrize("sfx", SUFFIXES)
def test_dual_agg_backward_checks_its_arguments(L, sfx):
    fe = getattr(L, "dn_dual_agg_bwd_edge_" + sfx)
    edge = lambda mode=0, N=10, E=20, H=64, src=P16, dst=P16, g=P16, x=P16, d=P16: fe(mode, N, E, H, src, dst, None, None, g, x, d, None)  # noqa: E731
    _err(L, edge(mode=-1), b"bad mode")
    _err(L, edge(H=300), b"1 <= H <= 256")
    _err(L, edge(dst=None), b"NULL pointer")
    _err(L, edge(d=None), b"NULL pointer")
    _err(L, edge(mode=2, x=None), b"mult needs src and x")
    assert edge(E=0) == 0
    fn = getattr(L, "dn_dual_agg_bwd_node_" + sfx)
    node = lambda mode=1, N=10, E=20, H=64, U=10, units=P16, perm=P16, dst=P16, g=P16, ef=P16, dx=P16, part=None, P=0: fn(  # noqa: E731
        mode, N, E, H, U, units, perm, dst, None, None, g, ef, dx, part, P, None)
    _err(L, node(mode=0), b"sub or mult")
    _err(L, node(H=0), b"1 <= H <= 256")
    _err(L, node(units=None), b"NULL unit table")
    _err(L, node(g=None), b"NULL pointer")
    _err(L, node(dx=None), b"NULL pointer")
    _err(L, node(mode=2, ef=None), b"mult needs ef")
    _err(L, node(P=2), b"partial slots without a partial buffer")
    assert node(U=0) == 0


@pytest.mark.parametrize("sfx", SUFFIXES)
def test_edge_update_checks_its_arguments(L, sfx):
    fn = getattr(L, "dn_dual_edge_update_" + sfx)
    call = lambda N=10, E=20, H=64, src=P16, coef=P16, xs=P16, out=P16: fn(N, E, H, src, P16, None, coef, P16, P16, P16, xs, None, out, None)  # noqa: E731
    _err(L, call(H=512), b"1 <= H <= 256")
    _err(L, call(E=1 << 31), b"E < 2^31")
    for kw in (dict(src=None), dict(coef=None), dict(xs=None), dict(out=None)):
        _err(L, call(**kw), b"NULL pointer")
    assert call(E=0) == 0
    fb = getattr(L, "dn_dual_edge_update_bwd_" + sfx)
    _err(L, fb(10, 20, 0, P16, P16, P16, P16, None), b"1 <= H <= 256")
    _err(L, fb(10, 20, 64, None, P16, P16, P16, None), b"NULL pointer")
    _err(L, fb(10, 20, 64, P16, P16, P16, None, None), b"NULL pointer")
    assert fb(10, 0, 64, None, None, None, None, None) == 0


@pytest.mark.parametrize("sfx", SUFFIXES)
def test_edge_pool_sum_checks_its_arguments(L, sfx):
    fn = getattr(L, "dn_sie_pool_sum_" + sfx)

    def call(B=4, eptr=P16, src=P16, dst=P16, N=30, id_=P16, enc_v=P16, Kv=8, vl=P16, el=P16, enc_el=P16, Kel=4, od=P16, idg=P16,
             rep=P16, H=64, pooled=P16, count=P16):
        return fn(B, eptr, None, src, dst, N, id_, enc_v, 16, Kv, vl, P16, 8, 6, el, enc_el, 4, Kel, od, idg, rep, H, pooled, count, None)

    _err(L, call(B=0), b"bad sizes")
    _err(L, call(H=0), b"bad sizes")
    _err(L, call(eptr=None), b"NULL pointer")
    _err(L, call(count=None), b"NULL pointer")
    _err(L, call(vl=None), b"all three encoders or none")
    _err(L, call(enc_el=None), b"all three encoders or none")
    _err(L, call(Kv=0), b"encoder sizes must be >= 1")
    _err(L, call(od=None), b"both degrees or neither")
    _err(L, call(src=None), b"need src and dst")
