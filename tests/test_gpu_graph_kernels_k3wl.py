"""GPU tests of the 3-WL graph kernels (graph_kernels_k3wl.py on dn_k3wl.hip) against the plain-Python restatement tests/k3wl_ref.py,
which tests/test_graph_kernels_k3wl_host.py holds against the reference binary's own output, and against that output itself.
Everything is exact integer arithmetic, so every comparison is equality, over ALL items.

* colours of every iteration: the six small golden datasets x four kernels, on both paths (fused and composed);
* graphs at the boundaries of the kernels' classes (k3wl_cases) against the restatement: 1, 2, 8 / 9, 16 / 17 nodes, an edgeless graph,
  hubs of degree 7 / 8 / 9, the composed path also in chunks of a few entries;
* where the restatement's n^4 work would take Python minutes, fused against composed at H = 1: hubs of degree 63 / 64 / 65 and a
  33-node graph, graphs of k3wl_max_nodes() and one more node in one dataset, LWLC hubs of degree k3wl_max_entries() - 1, + 0, + 1;
* the command line end to end against the binary's texts (DUMMY_BIG, TWOS, REDDIT-BINARY), integer gram matrices, determinism, and no
  read-back.
"""
import functools

import pytest
import torch

import k3wl_cases as C
import wl_cases
import wl_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H, GOLD = C.golden()
M64 = (1 << 64) - 1


def _kk():
    from dummynode4graphlearning_amd import graph_kernels_k3wl
    return graph_kernels_k3wl


@functools.lru_cache(maxsize=None)
def _limits():
    from dummynode4graphlearning_amd import ops
    return ops.k3wl_max_nodes(), ops.k3wl_max_entries()


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
    with ops.k3wl_fused(True):
        fused, tp = kk.k3wl_colors(d, h, kernel, use_nl, use_el, **kw)
    with ops.k3wl_fused(False):
        composed, tp2 = kk.k3wl_colors(d, h, kernel, use_nl, use_el, **kw)
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


def _assert_fused_is_composed(ds, h, kernel):
    fused, composed, _ = _both(ds, h, kernel)
    assert fused.shape[0] == h + 1 and torch.equal(fused, composed)
    assert not torch.equal(fused[h], fused[0])                              # (a step happened)
    return fused


@pytest.mark.parametrize("kernel", C.KERNELS)
@pytest.mark.parametrize("name", C.SMALL_GOLDENS)
def test_colors_golden(name, kernel):
    _assert_colors(GOLD[name], H, kernel, *C.flags(name))


@pytest.mark.parametrize("kernel", C.KERNELS)
def test_colors_small_sizes(kernel):
    """1, 2, 8, 9 nodes, an edgeless graph, hubs of degree 7, 8, 9 (8, 9 and 10 nodes); with and without labels; the composed path
    also in chunks of at most 300 entries (items with more take a chunk each)."""
    ds = C.small_bounds()
    p = _kk()._plan(_data(ds), kernel)
    if p.is_global:
        assert [c[0] for c in p.graph_classes] == [8, 16]
    else:
        assert [g for g, _, _ in p.tuple_classes] == [8, 64]
    _assert_colors(ds, 2, kernel)
    _assert_colors(ds, 1, kernel, workspace_keys=300)
    _assert_colors(ds, 1, kernel, False, False)


@pytest.mark.parametrize("kernel", C.KERNELS)
def test_colors_16_and_17_nodes(kernel):
    ds = C.mid_bounds()
    p = _kk()._plan(_data(ds), kernel)
    if p.is_global:
        assert [c[0] for c in p.graph_classes] == [16, 32]
    _assert_colors(ds, 1, kernel)


@pytest.mark.parametrize("kernel", C.KERNELS)
def test_colors_around_64(kernel):
    """Hubs of degree 63, 64, 65 (64, 65, 66 nodes) and a 33-node graph: the wavefront lists and the first workgroup lists of LWL /
    LWLC; the 64-lane fibres of WL / DWL and the first two graphs above them.  Fused against composed, one step."""
    ds = C.wave_bounds()
    p = _kk()._plan(_data(ds), kernel)
    if p.is_global:
        assert [c[0] for c in p.graph_classes] == [64] and p.fused_graph.tolist() == [True, False, False, True]
    elif kernel == "LWL":
        assert [(g, l) for g, l, _ in p.tuple_classes] == [(8, 0), (64, 0), (0, 128)] and p.fused_graph.all()
    else:
        assert [(g, l) for g, l, _ in p.tuple_classes] == [(8, 0), (64, 0), (0, 256)] and p.fused_graph.all()
    _assert_fused_is_composed(ds, 1, kernel)


@pytest.mark.parametrize("kernel", C.KERNELS)
def test_colors_across_the_node_limit(kernel):
    cap = _limits()[0]
    ds = C.limit_bounds(cap)
    p = _kk()._plan(_data(ds), kernel)
    if p.is_global:
        assert p.fused_graph.tolist() == [True, True, False, True]           # the hand-over is crossed inside the dataset
    else:
        assert p.fused_graph.all()
    fused = _assert_fused_is_composed(ds, 1, kernel)
    small = wl_cases.take(ds, 1)                                              # (and the first graph against the restatement)
    want = C.flat(C.ref(small, 1, kernel)[1], 1)
    assert _u(fused[1][:len(want)]) == want


def test_colors_across_the_list_limit():
    cap = _limits()[1]
    ds = C.hub_bounds(cap)
    p = _kk()._plan(_data(ds), "LWLC")
    assert p.fused_graph.tolist() == [True, True, False, True]
    classes = [(g, l) for g, l, _ in p.tuple_classes]                     # (a hub item's merged list holds up to 2 cap entries)
    assert classes[0] == (8, 0) and classes[-1] == (0, 2 * cap)
    _assert_fused_is_composed(ds, 1, "LWLC")


@pytest.mark.parametrize("kernel", C.KERNELS)
@pytest.mark.parametrize("name", C.SMALL_GOLDENS)
def test_gram(name, kernel):
    kk, ds = _kk(), GOLD[name]
    d, fl = _data(ds), C.flags(name)
    _, cols = C.ref(ds, H, kernel, *fl)
    want = wl_ref.gram([wl_ref.features(c) for c in cols], H, "WL")
    f = kk.k3wl_features(d, H, kernel, *fl)
    Gs = kk.k3wl_gram_matrices(d, H, kernel, *fl, features=f)
    assert len(Gs) == H + 1 and f.num_graphs == d.num_graphs and f.num_steps == H + 1
    for s in range(H + 1):
        assert Gs[s].dtype == torch.int64 and Gs[s].tolist() == want[s], (kernel, s)


@pytest.mark.parametrize("kernel", C.KERNELS)
def test_command_line_end_to_end(kernel, tmp_path, capsys):
    """The files `main` writes equal the text the reference's binary wrote (flags (true, true), (true, true) and (false, false))."""
    kk = _kk()
    names = ["DUMMY_BIG", "TWOS", "REDDIT-BINARY"]
    data, out = tmp_path / "data", tmp_path / "gram"
    out.mkdir()
    for i, name in enumerate(names):
        wl_cases.write_tu(GOLD[name], str(data), raw=bool(i % 2))
    assert kk.main(["--dataset_dir", str(data), "--gram_dir", str(out), "--k", "3", "--kernel", kernel, "--n_iters", str(H),
                    "--device", DEV, "--datasets"] + names) == 0
    for name in names:
        for h in range(H + 1):
            with open(out / ("%s__%s3_%d.gram" % (name, kernel, h)), "rb") as f:
                assert f.read() == GOLD[name]["grams"]["%s3_%d" % (kernel, h)].encode(), (name, kernel, h)
    said = capsys.readouterr().out
    assert "Warning: TWOS is not a valid dataset." in said and "Warning: REDDIT" not in said and "%s-%d\tDUMMY_BIG\t" % (kernel, H) in said


def test_two_runs_are_equal():
    from dummynode4graphlearning_amd import ops
    kk = _kk()
    big, mid = _data(GOLD["DUMMY_BIG"]), C.mid_bounds()
    for kernel in C.KERNELS:
        with ops.k3wl_fused(True):
            a, b = kk.k3wl_colors(big, H, kernel)[0], kk.k3wl_colors(big, H, kernel)[0]
        assert torch.equal(a, b)
        x, y = _both(mid, H, kernel), _both(mid, H, kernel)
        assert torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]) and torch.equal(x[0], x[1])
        p, q = kk.k3wl_gram_matrices(big, H, kernel), kk.k3wl_gram_matrices(big, H, kernel)
        assert all(torch.equal(s, t) for s, t in zip(p, q))


def test_refinement_and_gram_read_nothing_back():
    """k3wl_colors (both paths; K3WL_LIMIT also takes the composed path for its graph above the limit) and the gram launch under
    torch's sync debug mode "error" -- after checking that this build honours the mode at all.  Plans, chunks and the composed path's
    index arrays were built by the first use, and the feature build read its two sizes before."""
    from dummynode4graphlearning_amd import ops
    kk = _kk()
    d, m, s = _data(GOLD["DUMMY_BIG"]), _data(C.mid_bounds()), _data(C.limit_bounds(_limits()[0]))
    feats = {}
    for kernel in C.KERNELS:                                           # (first use: library load, plans, allocator)
        feats[kernel] = kk.k3wl_features(d, H, kernel)
        for on in (True, False):
            with ops.k3wl_fused(on):
                kk.k3wl_colors(m, 1, kernel)
                kk.k3wl_colors(s, 1, kernel)
    probe = torch.ones(1, device=DEV)
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            probe.item()                                               # the mode is honoured: a plain read-back raises
        got = {}
        for kernel in C.KERNELS:
            with ops.k3wl_fused(True):
                a = kk.k3wl_colors(m, H, kernel)[0]
                kk.k3wl_colors(d, H, kernel)
                kk.k3wl_colors(s, 1, kernel)
            with ops.k3wl_fused(False):
                b = kk.k3wl_colors(m, H, kernel)[0]
            got[kernel] = (a, b, kk.k3wl_gram_matrices(d, H, kernel, features=feats[kernel]))
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    for a, b, Gs in got.values():
        assert torch.equal(a, b) and len(Gs) == H + 1
