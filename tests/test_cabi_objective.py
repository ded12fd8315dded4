"""The dn_objective_* entry points (dn_objective.hip): exactly the declared symbols in the header, the binding and the library, and
their host-side argument checks -- NULL pointers, non-positive sizes, unknown criterion or dtype codes and more than four
representations are refused with -1 and a message before any launch (CPU only: nothing here reaches one)."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P16 = ctypes.c_void_p(16)
SYMBOLS = ["dn_objective_bwd", "dn_objective_eval", "dn_objective_fwd", "dn_objective_workspace_bytes"]


@pytest.fixture(scope="module")
def L():
    from dummynode4graphlearning_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.lib()


def _refused(L, rc, msg):
    assert rc == -1 and msg in L.dn_last_error(), (rc, L.dn_last_error())


def test_entry_points_are_the_declared_ones(L):
    from dummynode4graphlearning_amd import _lib
    assert [s for s in _lib.exported_symbols() if s.startswith("dn_objective_")] == SYMBOLS
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dn_hip.h")).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(dn_objective_[a-z0-9_]+)\s*\(", text))) == SYMBOLS
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    assert sorted(set(re.findall(r" T (dn_objective_[a-z0-9_]+)", out))) == SYMBOLS


def _reps(n, numel=64, denom=8, dt=0, ptr=16):
    k = max(n, 1)
    return ((ctypes.c_void_p * k)(*([ptr] * n)), (ctypes.c_int64 * k)(*([numel] * n)), (ctypes.c_int64 * k)(*([denom] * n)),
            (ctypes.c_int32 * k)(*([dt] * n)))


def test_workspace_bytes(L):
    _, numel, _, _ = _reps(2, numel=4097)
    assert L.dn_objective_workspace_bytes(5, 2, numel) == (2 + 2 * 2) * 6 * 8                   # 2 workgroups of pairs, 2 chunks a representation
    assert L.dn_objective_workspace_bytes(1, 0, None) == 6 * 8
    for B, n, arr in ((0, 0, None), (-3, 0, None), (4, 5, numel), (4, -1, numel), (4, 2, None)):
        assert L.dn_objective_workspace_bytes(B, n, arr) == 0
    _, zero, _, _ = _reps(1, numel=0)
    assert L.dn_objective_workspace_bytes(4, 1, zero) == 0 and b"bad sizes" in L.dn_last_error()


def _fwd(L, B=4, pc=P16, pc_dt=0, c=P16, c_dt=0, v=(8, P16, 0, P16, P16, 0), e=(16, P16, 1, P16, P16, 1), reps=None, n=2, bp=1, ev=1,
         terms=P16, loss=P16, ws=P16, ws_bytes=1 << 20):
    ptrs, numel, denom, dts = reps or _reps(n)
    return L.dn_objective_fwd(B, pc, pc_dt, c, c_dt, *v, *e, n, ptrs, numel, denom, dts, bp, ev, 0.25, 0.5, 0.25, 0.125, terms, loss, ws,
                              ws_bytes, None)


def _bwd(L, B=4, g=P16, pc=P16, pc_dt=0, c=P16, c_dt=0, v=(8, P16, 0, P16, P16, 0), e=(16, P16, 1, P16, P16, 1), reps=None, n=2, bp=1,
         dpc=P16, dpv=P16, dpe=P16, dreps=True):
    ptrs, numel, denom, dts = reps or _reps(n)
    out = (ctypes.c_void_p * max(n, 1))(*([16] * n)) if dreps else None
    return L.dn_objective_bwd(B, g, pc, pc_dt, c, c_dt, *v, *e, n, ptrs, numel, denom, dts, bp, 0.25, 0.5, 0.25, 0.125, dpc, dpv, dpe, out,
                              None)


def _eval(L, B=4, pc=P16, pc_dt=0, c=P16, c_dt=0, v=(8, P16, 0, P16, 0), e=(16, P16, 1, P16, 1), offset=0, cap=4, bufs=(P16,) * 5):
    return L.dn_objective_eval(B, pc, pc_dt, c, c_dt, *v, *e, offset, cap, *bufs, None)


ABSENT = (0, None, 0, None, None, 0)


@pytest.mark.parametrize("call", [_fwd, _bwd])
def test_fwd_and_bwd_check_their_arguments(L, call):
    for kw in (dict(B=0), dict(B=-1), dict(B=1 << 31), dict(v=(0, P16, 0, P16, P16, 0)), dict(e=(-2, P16, 0, P16, P16, 0)),
               dict(reps=_reps(2, numel=0)), dict(reps=_reps(2, denom=0))):
        _refused(L, call(L, **kw), b"bad sizes")
    for kw in (dict(pc=None), dict(c=None), dict(v=(8, None, 0, P16, P16, 0)), dict(v=(8, P16, 0, None, P16, 0)), dict(e=(16, P16, 0, P16, None, 0)),
               dict(reps=_reps(2, ptr=None)), dict(reps=(None,) + _reps(2)[1:]), dict(reps=_reps(2)[:1] + (None,) + _reps(2)[2:]),
               dict(reps=_reps(2)[:2] + (None, None))):
        _refused(L, call(L, **kw), b"NULL pointer")
    for kw in (dict(pc_dt=2), dict(c_dt=-1), dict(v=(8, P16, 7, P16, P16, 0)), dict(e=(16, P16, 0, P16, P16, 3)), dict(reps=_reps(2, dt=2))):
        _refused(L, call(L, **kw), b"unknown dtype code")
    for bp in (-1, 3, 99):
        _refused(L, call(L, bp=bp), b"unknown criterion")
    for n in (5, 9, -1):
        _refused(L, call(L, n=n, reps=_reps(5)), b"at most 4 representations")


def test_fwd_checks_its_outputs(L):
    _refused(L, _fwd(L, ev=3), b"unknown criterion")
    for kw in (dict(terms=None), dict(loss=None), dict(ws=None)):
        _refused(L, _fwd(L, **kw), b"NULL pointer")
    _refused(L, _fwd(L, ws_bytes=8), b"workspace too small")
    _refused(L, _fwd(L, ws=ctypes.c_void_p(20)), b"workspace too small or not 8-byte aligned")
    _refused(L, _fwd(L, v=ABSENT, e=ABSENT, n=0, ws_bytes=0), b"workspace too small")


def test_bwd_checks_its_outputs(L):
    _refused(L, _bwd(L, g=None), b"NULL pointer")
    _refused(L, _bwd(L, dreps=False), b"NULL pointer")
    _refused(L, _bwd(L, v=ABSENT), b"a side that is absent")
    _refused(L, _bwd(L, e=ABSENT, dpv=None), b"a side that is absent")


def test_eval_checks_its_arguments(L):
    for kw in (dict(B=0), dict(B=-4), dict(v=(0, P16, 0, P16, 0)), dict(offset=-1), dict(offset=1), dict(cap=0), dict(cap=3)):
        _refused(L, _eval(L, **kw), b"bad sizes")
    for kw in (dict(pc=None), dict(c=None), dict(v=(8, None, 0, P16, 0)), dict(e=(16, P16, 0, None, 0)), dict(bufs=(P16, None, P16, P16, P16)),
               dict(bufs=(P16,) * 4 + (None,))):
        _refused(L, _eval(L, **kw), b"NULL pointer")
    for kw in (dict(pc_dt=5), dict(v=(8, P16, 0, P16, 2))):
        _refused(L, _eval(L, **kw), b"unknown dtype code")
