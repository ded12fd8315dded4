"""GPU tests of the 2-WL graph kernels (graph_kernels_kwl.py on dn_kwl.hip) against the plain-Python restatement tests/kwl_ref.py,
which tests/test_graph_kernels_kwl_host.py holds against the reference binary's own output.  Everything is exact integer arithmetic,
so every comparison is equality, over ALL tuples.

* colours of every iteration: the six golden datasets x four kernels, on both paths (fused and composed);
* graphs at the boundaries of the kernels' classes (kwl_cases): 1, 2, 8 / 9, 16 / 17 nodes, hubs of degree 7 / 8 / 9 and 63 / 64 / 65
  (64 / 65 / 66 nodes), the composed path in chunks of a few entries;
* the upper limits: graphs of kwl_max_nodes() and one more node in one dataset (WL / DWL fused against composed, the restatement being
  O(n^3) per step; LWL / LWLC against the restatement), hubs of degree kwl_max_entries() - 1, + 0, + 1 (LWLC);
* integer gram matrices, the command line end to end against the golden texts, determinism, and no read-back.
"""
import functools

import pytest
import torch

import kwl_cases as C
import wl_cases
import wl_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H, GOLD = C.golden()
M64 = (1 << 64) - 1


def _kk():
    from dummynode4graphlearning_amd import graph_kernels_kwl
    return graph_kernels_kwl


@functools.lru_cache(maxsize=None)
def _limits():
    from dummynode4graphlearning_amd import ops
    return ops.kwl_max_nodes(), ops.kwl_max_entries()


_DATA = {}


def _data(ds):
    if ds["name"] not in _DATA:
        _DATA[ds["name"]] = _kk().GraphKernelData.from_arrays(ds["graph_indicator"], ds["A"], ds["node_labels"], ds["edge_labels"],
                                                              ds["graph_labels"], device=DEV)
    return _DATA[ds["name"]]


def _u(t):
    return [x & M64 for x in t.cpu().tolist()]


def _both(ds, h, kernel, use_nl=True, use_el=True, workspace_keys=None):
    from dummynode4graphlearning_amd import ops
    kk, d = _kk(), _data(ds)
    kw = {} if workspace_keys is None else {"workspace_keys": workspace_keys}
    with ops.kwl_fused(True):
        fused, tp = kk.kwl_colors(d, h, kernel, use_nl, use_el, **kw)
    with ops.kwl_fused(False):
        composed, tp2 = kk.kwl_colors(d, h, kernel, use_nl, use_el, **kw)
    assert torch.equal(tp, tp2) and tp.dtype == torch.int32
    return fused, composed, tp


def _assert_colors(ds, h, kernel, use_nl=True, use_el=True, workspace_keys=None):
    fused, composed, tp = _both(ds, h, kernel, use_nl, use_el, workspace_keys)
    _, cols = C.ref(ds, h, kernel, use_nl, use_el)
    sizes = [len(c[0]) for c in cols]
    assert tp.tolist() == [sum(sizes[:g]) for g in range(len(sizes) + 1)]
    assert fused.shape == composed.shape == (h + 1, sum(sizes)) and fused.dtype == torch.int64
    for it in range(h + 1):
        want = C.flat(cols, it)
        assert _u(fused[it]) == want, "fused, iteration %d" % it
        assert _u(composed[it]) == want, "composed, iteration %d" % it


@pytest.mark.parametrize("kernel", C.KERNELS)
@pytest.mark.parametrize("name", sorted(GOLD))
def test_colors_golden(name, kernel):
    _assert_colors(GOLD[name], H, kernel, *C.flags(name))


@pytest.mark.parametrize("kernel", C.KERNELS)
def test_colors_small_sizes(kernel):
    """1, 2, 8, 9, 16, 17 nodes, an edgeless graph, hubs of degree 7, 8, 9; with and without labels; the composed path also in chunks
    of at most 50 entries (tuples with more take a chunk each)."""
    ds = C.small_bounds()
    p = _kk()._plan(_data(ds), kernel)
    if p.is_global:
        assert [c for c, _ in p.graph_classes] == [8, 16, 32]
    else:
        assert [g for g, _, _ in p.tuple_classes] == [8, 64]
    _assert_colors(ds, 2, kernel)
    _assert_colors(ds, 2, kernel, workspace_keys=50)
    _assert_colors(ds, 1, kernel, False, False)


@pytest.mark.parametrize("kernel", C.KERNELS)
def test_colors_around_64(kernel):
    """Hubs of degree 63, 64, 65 (64, 65, 66 nodes) and a 33-node graph: the wavefront lists and the first workgroup lists of LWL /
    LWLC, the 64-node and 128-node classes of WL / DWL."""
    ds = C.wave_bounds()
    p = _kk()._plan(_data(ds), kernel)
    if p.is_global:
        assert [c for c, _ in p.graph_classes] == [64, 128]
    else:
        assert [(g, l) for g, l, _ in p.tuple_classes] == [(8, 0), (64, 0), (0, 128)]
    _assert_colors(ds, 2, kernel)


@pytest.mark.parametrize("kernel", C.KERNELS)
def test_colors_across_the_node_limit(kernel):
    cap = _limits()[0]
    ds = C.limit_bounds(cap)
    p = _kk()._plan(_data(ds), kernel)
    if p.is_global:
        assert p.fused_graph.tolist() == [True, True, False, True]           # the hand-over is crossed inside the dataset
        fused, composed, _ = _both(ds, 2, kernel)
        assert torch.equal(fused, composed)
        small = wl_cases.take(ds, 1)                                          # (and the first graph against the restatement)
        assert _u(fused[2][:25]) == C.flat(C.ref(small, 2, kernel)[1], 2)
    else:
        assert p.fused_graph.all()
        _assert_colors(ds, 2, kernel)


def test_colors_across_the_list_limit():
    cap = _limits()[1]
    ds = C.hub_bounds(cap)
    p = _kk()._plan(_data(ds), "LWLC")
    assert p.fused_graph.tolist() == [True, True, False, True] and [(g, l) for g, l, _ in p.tuple_classes] == [(8, 0), (0, cap)]
    _assert_colors(ds, 1, "LWLC")                                       # (one step: the restatement walks the hub lists in Python)


@pytest.mark.parametrize("kernel", C.KERNELS)
@pytest.mark.parametrize("name", ["DUMMY_BIG", "TWOS", "REDDIT-BINARY"])
def test_gram(name, kernel):
    kk, ds = _kk(), GOLD[name]
    d, fl = _data(ds), C.flags(name)
    _, cols = C.ref(ds, H, kernel, *fl)
    want = wl_ref.gram([wl_ref.features(c) for c in cols], H, "WL")
    f = kk.kwl_features(d, H, kernel, *fl)
    Gs = kk.kwl_gram_matrices(d, H, kernel, *fl, features=f)
    assert len(Gs) == H + 1 and f.num_graphs == d.num_graphs and f.num_steps == H + 1
    for s in range(H + 1):
        assert Gs[s].dtype == torch.int64 and Gs[s].tolist() == want[s], (kernel, s)


def test_command_line_end_to_end(tmp_path, capsys):
    kk = _kk()
    data, out = tmp_path / "data", tmp_path / "gram"
    out.mkdir()
    for i, ds in enumerate(GOLD.values()):
        wl_cases.write_tu(ds, str(data), raw=bool(i % 2))
    for kernel in C.KERNELS:
        assert kk.main(["--dataset_dir", str(data), "--gram_dir", str(out), "--k", "2", "--kernel", kernel, "--n_iters", str(H),
                        "--device", DEV, "--datasets"] + list(GOLD)) == 0
        for name, ds in GOLD.items():
            for h in range(H + 1):
                with open(out / ("%s__%s2_%d.gram" % (name, kernel, h)), "rb") as f:
                    assert f.read() == ds["grams"]["%s2_%d" % (kernel, h)].encode(), (name, kernel, h)
    said = capsys.readouterr().out
    assert "Warning: TWOS is not a valid dataset." in said and "Warning: NCI1" not in said and "LWLC-%d\tQUIRKS\t" % H in said


def test_two_runs_are_equal():
    kk, ds = _kk(), GOLD["DUMMY_BIG"]
    d = _data(ds)
    for kernel in C.KERNELS:
        a, b = _both(ds, H, kernel), _both(ds, H, kernel)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        x, y = kk.kwl_gram_matrices(d, H, kernel), kk.kwl_gram_matrices(d, H, kernel)
        assert all(torch.equal(p, q) for p, q in zip(x, y))


def test_refinement_and_gram_read_nothing_back():
    """kwl_colors (both paths; KWL_LIMIT also takes the composed path for its graph above the limit) and the gram launch under torch's
    sync debug mode "error" -- after checking that this build honours the mode at all.  Plans, chunks and the composed path's index
    arrays were built by the first use, and the feature build read its two sizes before."""
    from dummynode4graphlearning_amd import ops
    kk = _kk()
    d, s = _data(GOLD["DUMMY_BIG"]), _data(C.limit_bounds(_limits()[0]))
    feats = {}
    for kernel in C.KERNELS:                                           # (first use: library load, plans, allocator)
        feats[kernel] = kk.kwl_features(d, H, kernel)
        for on in (True, False):
            with ops.kwl_fused(on):
                kk.kwl_colors(d, 1, kernel)
                kk.kwl_colors(s, 1, kernel)
    probe = torch.ones(1, device=DEV)
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            probe.item()                                               # the mode is honoured: a plain read-back raises
        got = {}
        for kernel in C.KERNELS:
            with ops.kwl_fused(True):
                a = kk.kwl_colors(d, H, kernel)[0]
                kk.kwl_colors(s, 1, kernel)
            with ops.kwl_fused(False):
                b = kk.kwl_colors(d, H, kernel)[0]
            got[kernel] = (a, b, kk.kwl_gram_matrices(d, H, kernel, features=feats[kernel]))
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    for a, b, Gs in got.values():
        assert torch.equal(a, b) and len(Gs) == H + 1
