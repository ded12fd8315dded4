"""The dn_gk_* entry points (dn_gk.hip) check their arguments on the host before any launch: NULL pointers, non-positive sizes, sizes
past int32 and unknown classes are refused with -1 and a message (CPU only: nothing here reaches a launch)."""
import ctypes
import os
import re

import pytest

P16 = ctypes.c_void_p(16)
BIG = 1 << 31
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def L():
    from dummynode4graphlearning_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.lib()


def _refused(L, rc, msg):
    assert rc == -1 and msg in L.dn_last_error(), L.dn_last_error()


def test_entry_points_are_the_gk_ones():
    from dummynode4graphlearning_amd import _lib
    names = ["dn_gk_gr_keys_u64", "dn_gk_sp_lds_max_nodes", "dn_gk_sp_u64"]
    assert [s for s in _lib.exported_symbols() if s.startswith("dn_gk_")] == names
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dn_hip.h")).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(dn_gk_[a-z0-9_]+)\s*\(", header))) == names
    source = open(os.path.join(ROOT, "dummynode4graphlearning_amd", "csrc", "dn_gk.hip")).read()
    assert sorted(set(re.findall(r"^int(?:32_t)? (dn_[a-z0-9_]+)\(", source, flags=re.M))) == names
    from dummynode4graphlearning_amd.csrc import build
    assert "dn_gk.hip" in build.SOURCES


def test_limits(L):
    cap = L.dn_gk_sp_lds_max_nodes()
    words = (cap + 63) // 64
    assert cap > 64 and (cap * words + 4 * 3 * words) * 8 + 4 * cap * 4 <= 65536      # bit matrix, per-wave sets and histograms


def test_sp_checks_its_arguments(L):
    def call(B=10, n=10, graphs=P16, group=64, lds=0, node_ptr=P16, ptr=P16, nbr=P16, base=P16, lcls=P16, cptr=P16, crank=P16, counts=P16,
             offsets=None, entries=0, key=None, cnt=None):
        return L.dn_gk_sp_u64(B, n, graphs, group, lds, node_ptr, ptr, nbr, base, lcls, cptr, crank, counts, offsets, entries, key, cnt, None)

    for kw in (dict(B=0), dict(B=-3), dict(n=0), dict(n=-1), dict(B=BIG, n=1), dict(n=11)):
        _refused(L, call(**kw), b"bad sizes")
    for name in ("graphs", "node_ptr", "ptr", "nbr", "base", "lcls", "cptr", "crank", "counts"):
        _refused(L, call(**{name: None}), b"NULL pointer")
    for kw in (dict(key=P16, cnt=P16), dict(entries=5, cnt=P16), dict(entries=5, key=P16), dict(entries=-1, key=P16, cnt=P16)):
        _refused(L, call(offsets=P16, **kw), b"NULL pointer")
    for group in (8, 1, -1, 256):
        _refused(L, call(group=group), b"group must be 64")
    cap = L.dn_gk_sp_lds_max_nodes()
    for lds in (0, -8, cap + 1):
        _refused(L, call(group=0, lds=lds), b"lds_nodes must be 1 ..")


def test_gr_checks_its_arguments(L):
    def call(N=10, n=4, group=8, node=P16, r0=P16, r1=P16, off=P16, ptr=P16, nbr=P16, nl=P16, el=P16, graph=P16, cap=100, key=P16, gid=P16):
        return L.dn_gk_gr_keys_u64(N, n, group, node, r0, r1, off, ptr, nbr, nl, el, graph, cap, key, gid, None)

    for kw in (dict(N=0), dict(N=-3), dict(n=0), dict(n=-1), dict(N=BIG), dict(n=BIG), dict(cap=0), dict(cap=-5)):
        _refused(L, call(**kw), b"bad sizes")
    for name in ("node", "r0", "r1", "off", "ptr", "nbr", "graph", "key", "gid"):
        _refused(L, call(**{name: None}), b"NULL pointer")
    for group in (16, 1, -1, 256):
        _refused(L, call(group=group), b"group must be 8, 64 or 0")
    _refused(L, call(nl=None), b"edge labels need node labels")
