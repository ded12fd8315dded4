"""The SI model entry points of include/dn_hip.h (dn_si_*) check their arguments before anything reaches the GPU (CPU only:
every call below fails in its argument checks, which run on the host)."""
import os

import pytest


@pytest.fixture(scope="module")
def lib():
    from dummynode4graphlearning_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib


def _err(L, rc, text):
    assert rc == -1, rc
    msg = L.dn_last_error()
    assert text.encode() in msg, msg


def test_si_entry_points_are_bound(lib):
    names = [n for n in lib.exported_symbols() if n.startswith("dn_si_")]
    assert len(names) == 16
    L = lib.lib()
    for n in names:
        assert hasattr(L, n)


def test_filter_meta_checks_its_arguments(lib):
    L = lib.lib()
    for fn in (L.dn_si_filter_meta_f32, L.dn_si_filter_meta_bf16):
        _err(L, fn(0, None, None, None, 0, None, None, None, 0, 1, 1, 1, 1, None, None, None), "1 <= B")
        _err(L, fn(4, None, None, None, 0, None, None, None, 0, 1, 1, 1, 1, None, None, None), "NULL pointer")
        _err(L, fn(4, 8, None, None, 5, 8, None, None, 0, 1, 1, 1, 1, None, 8, None), "NULL label / id")
        _err(L, fn(4, 8, 8, 8, 5, 8, 8, 8, 5, 0, 1, 1, 1, None, 8, None), "table sizes")
        _err(L, fn(4, 8, 8, 8, 1 << 40, 8, 8, 8, 5, 1, 1, 1, 1, None, 8, None), "fit int32")


def test_embed_checks_its_arguments(lib):
    L = lib.lib()
    for fn in (L.dn_si_embed_fwd_f32, L.dn_si_embed_fwd_bf16):
        _err(L, fn(10, 0, 8, 8, 4, 4, 8, None, None, 0, 0, None, 8, None), "bad sizes")
        _err(L, fn(10, 16, None, 8, 4, 4, 8, None, None, 0, 0, None, 8, None), "NULL pointer")
        _err(L, fn(10, 16, 8, 8, 4, 4, 8, 8, None, 4, 4, None, 8, None), "second table incomplete")
        _err(L, fn(10, 256, 8, 8, 4, 64, 8, 8, 8, 4, 64, 8, 8, None), "(K1 + K2) * H must be <= 16384")
        _err(L, fn(10, 512, 8, 8, 4, 4, 8, None, None, 0, 0, None, 8, None), "H <= 256 and K <= 64")
    assert L.dn_si_embed_wgrad_workspace_bytes(-1, 4, 4) == 0
    assert L.dn_si_embed_wgrad_workspace_bytes(1000, 4, 16) == 32 * 4 * 16 * 4           # 32 chunks of 32 rows
    for fn in (L.dn_si_embed_wgrad_f32, L.dn_si_embed_wgrad_bf16):
        _err(L, fn(10, 16, 8, 8, 4, 0, 8, 8, 8, 1 << 20, None), "bad sizes")
        _err(L, fn(10, 16, None, 8, 4, 4, 8, 8, 8, 1 << 20, None), "NULL pointer")
        _err(L, fn(1000, 16, 8, 8, 4, 4, 8, 8, 8, 16, None), "workspace too small")
        _err(L, fn(10, 512, 8, 8, 4, 4, 8, 8, 8, 1 << 20, None), "H <= 256 and K <= 64")


def test_pooling_and_mask_check_their_arguments(lib):
    L = lib.lib()
    for fn in (L.dn_si_pool_sum_f32, L.dn_si_pool_sum_bf16):
        _err(L, fn(0, 8, None, None, None, 0, 0, None, None, 0, 0, None, None, 8, 16, 8, 8, None), "bad sizes")
        _err(L, fn(4, None, None, None, None, 0, 0, None, None, 0, 0, None, None, 8, 16, 8, 8, None), "NULL pointer")
        _err(L, fn(4, 8, None, 8, None, 0, 0, None, None, 0, 0, None, None, 8, 16, 8, 8, None), "enc_v incomplete")
        _err(L, fn(4, 8, None, None, None, 0, 0, 8, None, 0, 0, None, None, 8, 16, 8, 8, None), "enc_vl incomplete")
        _err(L, fn(4, 8, None, None, None, 0, 0, None, None, 0, 0, 8, None, 8, 16, 8, 8, None), "both degrees or neither")
    for fn in (L.dn_si_pool_sum_bwd_f32, L.dn_si_pool_sum_bwd_bf16):
        _err(L, fn(4, 8, None, 8, 16, 8, 16, 8, None), "bad sizes")                   # col0 + H > D
        _err(L, fn(4, None, None, 8, 16, 0, 16, 8, None), "NULL pointer")
    for fn in (L.dn_si_pool_max_f32, L.dn_si_pool_max_bf16):
        _err(L, fn(4, 8, None, 8, 16, 8, 0, 8, 8, None), "bad sizes")                 # L == 0
        _err(L, fn(4, 8, None, 8, 16, None, 3, 8, 8, None), "NULL pointer")
    for fn in (L.dn_si_pool_max_bwd_f32, L.dn_si_pool_max_bwd_bf16):
        _err(L, fn(0, 16, 8, 8, 8, None), "bad sizes")
        _err(L, fn(4, 16, None, 8, 8, None), "NULL pointer")
    _err(L, L.dn_si_len_mask_u8(4, 0, 8, None, 8, None), "bad sizes")
    _err(L, L.dn_si_len_mask_u8(4, 5, None, None, 8, None), "NULL pointer")
    with pytest.raises(lib.DnHipError):
        lib.check(L.dn_si_len_mask_u8(4, 5, None, None, 8, None), "dn_si_len_mask_u8")
