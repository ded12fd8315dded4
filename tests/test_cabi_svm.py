"""The dn_svm_* entry points (dn_svm.hip) check their arguments on the host before any launch: NULL pointers, non-positive sizes,
eps <= 0, iters_per_launch < 1 and a row list beyond the LDS limit are refused with -1 and a message (CPU only: nothing here
reaches a launch)."""
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


def _refused(L, rc, msg):
    assert rc == -1 and msg in L.dn_last_error(), L.dn_last_error()


def test_entry_points_are_the_svm_ones():
    from dummynode4graphlearning_amd import _lib
    assert [s for s in _lib.exported_symbols() if s.startswith("dn_svm_")] == ["dn_svm_max_rows", "dn_svm_smo_f64"]


def test_limit(L):
    cap = L.dn_svm_max_rows()
    assert cap >= 3288 and 28 * cap + 1024 <= 160 * 1024                     # the benchmark's solves fit; the state fits the CU's LDS


def test_smo_checks_its_arguments(L):
    def call(M=2, n=50, K=P16, S=6, table=P16, n_list=6, lst=None, R=200, rows=P16, max_len=40, eps=1e-3, ipl=100, alpha=P16, grad=P16,
             rho=P16, iters=P16, status=P16):
        return L.dn_svm_smo_f64(M, n, K, S, table, n_list, lst, R, rows, max_len, eps, ipl, alpha, grad, rho, iters, status, None)

    for kw in (dict(M=0), dict(M=-1), dict(n=0), dict(n=1 << 31), dict(S=0), dict(S=-2), dict(n_list=0, lst=P16), dict(n_list=7, lst=P16),
               dict(R=0), dict(R=-5)):
        _refused(L, call(**kw), b"bad sizes")
    for kw in (dict(K=None), dict(table=None), dict(rows=None), dict(alpha=None), dict(grad=None), dict(rho=None), dict(iters=None),
               dict(status=None), dict(n_list=3)):
        _refused(L, call(**kw), b"NULL pointer")
    for eps in (0.0, -1e-3, float("nan")):
        _refused(L, call(eps=eps), b"eps must be > 0")
    for ipl in (0, -1):
        _refused(L, call(ipl=ipl), b"iters_per_launch must be >= 1")
    for max_len in (0, -1, L.dn_svm_max_rows() + 1, 201):
        _refused(L, call(max_len=max_len, R=200 if max_len == 201 else 1 << 20), b"the LDS limit")
