"""Host side of the batch loader (no GPU): the batch plan, the error cases, BatchLoader's ordering, and the argument checks of
dn_batch_assemble (reported before anything is launched)."""
import ctypes
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch


def _items(sizes, edges, F=3):
    g = torch.Generator().manual_seed(0)
    out = []
    for n, e in zip(sizes, edges):
        out.append(SimpleNamespace(x=torch.randn(n, F, generator=g),
                                   edge_index=torch.randint(0, max(n, 1), (2, e), generator=g) if e else torch.zeros((2, 0), dtype=torch.long),
                                   edge_attr=None, y=torch.tensor([n % 2]), is_dummy_node=None, is_dummy_edge=None))
    return out


def test_plan_matches_numpy_on_random_sizes():
    from dummynode4graphlearning_amd.loader import plan_batch
    rng = np.random.default_rng(0)
    for _ in range(50):
        G = int(rng.integers(1, 40))
        nn = rng.integers(0, 50, size=G) * (rng.random(G) > 0.3)             # empty graphs included
        ne = rng.integers(0, 200, size=G) * (nn > 0)
        ids = rng.integers(0, G, size=int(rng.integers(1, 60)))              # duplicates, any order
        got_ids, onp, oep = plan_batch(nn.astype(np.int64), ne.astype(np.int64), ids.tolist())
        assert got_ids.dtype == onp.dtype == oep.dtype == np.int64
        assert np.array_equal(got_ids, ids)
        assert np.array_equal(onp, np.concatenate([[0], np.cumsum(nn[ids])]))
        assert np.array_equal(oep, np.concatenate([[0], np.cumsum(ne[ids])]))
    # ids as a CPU tensor / numpy array give the same plan
    a = plan_batch(np.array([3, 0, 2]), np.array([5, 0, 1]), torch.tensor([2, 2, 1]))
    b = plan_batch(np.array([3, 0, 2]), np.array([5, 0, 1]), np.array([2, 2, 1], dtype=np.int32))
    assert all(np.array_equal(x, y) for x, y in zip(a, b)) and a[1].tolist() == [0, 2, 4, 4] and a[2].tolist() == [0, 1, 2, 2]


def test_error_cases():
    from dummynode4graphlearning_amd import PackedGraphs, _lib
    packed = PackedGraphs.from_items(_items([0, 4, 2], [0, 6, 1]))
    assert len(packed) == 3 and packed.num_nodes == 6 and packed.num_edges == 7
    assert packed.node_ptr.dtype == torch.int32 and packed.node_ptr.tolist() == [0, 0, 4, 6] and packed.edge_ptr.tolist() == [0, 0, 6, 7]
    assert isinstance(packed.node_sizes, np.ndarray) and packed.node_ptr_host.tolist() == [0, 0, 4, 6]
    with pytest.raises(IndexError):
        packed.assemble([0, 3])
    with pytest.raises(IndexError):
        packed.assemble([-1])
    with pytest.raises(ValueError):
        packed.assemble([])
    with pytest.raises(ValueError):
        packed.assemble(torch.zeros(0, dtype=torch.long))
    with pytest.raises(_lib.DnHipError):                                   # CPU tensors: no fallback, the product path is the GPU's
        packed.assemble([1])
    with pytest.raises(ValueError):                                          # an optional field given by some graphs only
        it = _items([2, 2], [1, 1])
        it[0].edge_attr = torch.zeros(1, 2)
        PackedGraphs.from_items(it)


def test_int32_guard_fires_on_fake_sizes_without_allocating():
    from dummynode4graphlearning_amd.loader import check_totals, plan_batch
    big = np.broadcast_to(np.int64(1 << 20), (1 << 11,))                     # 2^31 in total, 8 bytes of memory
    small = np.broadcast_to(np.int64(1), (1 << 11,))
    with pytest.raises(ValueError):
        check_totals(big, small)
    with pytest.raises(ValueError):
        check_totals(small, big)
    assert check_totals(big[:-1], small) == ((1 << 31) - (1 << 20), 1 << 11)
    with pytest.raises(ValueError):                                          # a batch of duplicates can pass 2^31 on its own
        plan_batch(np.array([1 << 30], dtype=np.int64), np.array([1], dtype=np.int64), [0, 0])
    assert plan_batch(np.array([(1 << 30) - 1], dtype=np.int64), np.array([1], dtype=np.int64), [0, 0])[1][-1] == (1 << 31) - 2


class _Fake:
    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n

    def assemble(self, ids):
        return [int(i) for i in ids]


def test_batch_loader_order_len_and_reiteration():
    from dummynode4graphlearning_amd import BatchLoader
    ds = _Fake(23)
    plain = BatchLoader(ds, batch_size=5)
    assert len(plain) == 5 and list(plain) == [list(range(a, min(a + 5, 23))) for a in range(0, 23, 5)]
    assert list(plain) == list(plain)                                        # re-iterable
    dl = BatchLoader(ds, batch_size=5, drop_last=True)
    assert len(dl) == 4 and list(dl) == [list(range(a, a + 5)) for a in range(0, 20, 5)]
    assert len(BatchLoader(_Fake(20), batch_size=5)) == len(BatchLoader(_Fake(20), batch_size=5, drop_last=True)) == 4
    # shuffle: an epoch's order is torch.randperm(len, generator=generator) on the CPU; the next epoch draws the next permutation
    gen, ref = torch.Generator().manual_seed(7), torch.Generator().manual_seed(7)
    sh = BatchLoader(ds, batch_size=4, shuffle=True, generator=gen)
    for _ in range(2):
        want = torch.randperm(23, generator=ref).tolist()
        got = list(sh)
        assert len(got) == len(sh) == 6 and sum(got, []) == want and [len(b) for b in got] == [4, 4, 4, 4, 4, 3]
    e1, e2 = sum(list(sh), []), sum(list(sh), [])
    assert e1 != e2 and sorted(e1) == sorted(e2) == list(range(23))
    shd = BatchLoader(ds, batch_size=4, shuffle=True, drop_last=True, generator=torch.Generator().manual_seed(7))
    assert sum(list(shd), []) == torch.randperm(23, generator=torch.Generator().manual_seed(7)).tolist()[:20]


def test_batch_loader_sampler_and_fetch_pass_through():
    from dummynode4graphlearning_amd import BatchLoader
    sampler = [[3, 1], [0], [2, 2, 2]]
    seen = []
    bl = BatchLoader(_Fake(4), batch_sampler=sampler, fetch=lambda ids: seen.append(ids) or ("batch", tuple(ids)))
    assert len(bl) == 3 and list(bl) == [("batch", (3, 1)), ("batch", (0,)), ("batch", (2, 2, 2))]
    assert seen[0] is sampler[0]                                             # the sampler's lists arrive as they are
    assert list(BatchLoader(_Fake(4), batch_sampler=iter_twice(sampler))) == sampler
    for kw in (dict(batch_size=2), dict(shuffle=True), dict(drop_last=True)):
        with pytest.raises(ValueError):
            BatchLoader(_Fake(4), batch_sampler=sampler, **kw)
    with pytest.raises(ValueError):
        BatchLoader(_Fake(4), batch_size=0)


class iter_twice:
    """An iterable (not a list) of index lists, as a bucket sampler object is."""

    def __init__(self, lists):
        self.lists = lists

    def __iter__(self):
        return iter(self.lists)

    def __len__(self):
        return len(self.lists)


@pytest.fixture(scope="module")
def lib():
    from dummynode4graphlearning_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib


def test_batch_assemble_checks_its_arguments_without_a_gpu(lib):
    L = lib.lib()
    P16, P4 = ctypes.c_void_p(16), ctypes.c_void_p(4)

    def col(**kw):
        arr = (lib.BatchCol * 1)()
        c = dict(src=P16, dst=P16, row_bytes=4, level=0, rebase=0, int_width=0, src_global=0, ptr_tail=0)
        c.update(kw)
        for k, v in c.items():
            setattr(arr[0], k, v)
        return arr

    def call(B=2, table=P16, dn=P16, de=P16, G=5, N=3, E=1, cols=None, n=1, bvec=None):
        return L.dn_batch_assemble(B, table, dn, de, G, N, E, col() if cols is None else cols, n, bvec, None)

    assert L.dn_batch_assemble(0, None, None, None, 0, 0, 0, None, 0, None, None) == 0           # B == 0: nothing to do
    assert call(B=0, table=None) == 0
    assert call(N=0, E=0, n=0) == 0                                                            # no rows at all: no launch
    assert call(N=0, E=0, cols=col(level=0), bvec=P16) == 0
    for kw, msg in ((dict(B=-1), b"bad sizes"), (dict(N=-1), b"bad sizes"), (dict(E=1 << 31), b"bad sizes"), (dict(n=-1), b"bad sizes"),
                    (dict(n=33), b"too many columns"), (dict(table=None), b"NULL pointer"), (dict(dn=None), b"NULL pointer"),
                    (dict(de=None), b"NULL pointer"), (dict(cols=col(src=None)), b"NULL pointer"),
                    (dict(cols=col(dst=None)), b"NULL pointer"), (dict(cols=col(row_bytes=0)), b"bad sizes"),
                    (dict(cols=col(level=3)), b"bad sizes"), (dict(cols=col(rebase=3)), b"bad sizes"),
                    (dict(cols=col(rebase=1, int_width=2)), b"bad sizes"), (dict(cols=col(rebase=1, int_width=8, row_bytes=12)), b"bad sizes"),
                    (dict(cols=col(rebase=1, int_width=4, level=2)), b"bad sizes"), (dict(cols=col(ptr_tail=1)), b"bad sizes"),
                    (dict(cols=col(rebase=2, int_width=8, row_bytes=8, dst=P4)), b"not aligned"),
                    (dict(N=0, E=0, cols=col(rebase=2, int_width=4, ptr_tail=1, dst=None)), b"NULL pointer")):
        assert call(**kw) == -1 and msg in L.dn_last_error(), (kw, L.dn_last_error())
    rc = call(cols=None, n=1, table=None)
    with pytest.raises(lib.DnHipError):
        lib.check(rc, "dn_batch_assemble")
