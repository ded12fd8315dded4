"""GPU tests of the WL / WLOA graph kernels (graph_kernels.py on dn_wl.hip) against the plain-Python restatement tests/wl_ref.py,
which tests/test_graph_kernels_host.py holds against the reference binary's own output.  Everything is exact integer arithmetic, so
every comparison is equality.

* colours: every golden dataset under its flags, and STARS (wl_cases.stars: centre entry counts at every boundary of the three
  refinement launches and of their cap, with and without edge labels, labels near 2^63 and 2^64 - 1), fused and composed;
* features: colours, counts and steps;
* gram: WL and WLOA, every h, B in {1, tile - 1, tile, tile + 1, 2 tile + 3}, two graphs without a common colour, feature rows of
  about 3000 entries next to rows of a few dozen (at the kernel's largest number of steps), symmetry;
* the command line end to end against the golden texts, determinism, and no read-back in refinement and gram.
"""
import functools

import pytest
import torch

import wl_cases as C
import wl_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H, GOLD = C.golden()
M64 = (1 << 64) - 1


def _gk():
    from dummynode4graphlearning_amd import graph_kernels
    return graph_kernels


@functools.lru_cache(maxsize=None)
def _limits():
    from dummynode4graphlearning_amd import ops
    return ops.wl_max_entries(), ops.wl_gram_tile(), ops.wl_max_steps()


_DATA = {}


def _data(ds):
    if ds["name"] not in _DATA:
        _DATA[ds["name"]] = _gk().GraphKernelData.from_arrays(ds["graph_indicator"], ds["A"], ds["node_labels"], ds["edge_labels"],
                                                              ds["graph_labels"], device=DEV)
    return _DATA[ds["name"]]


def _u(t):
    return [x & M64 for x in t.cpu().tolist()]


def _colors_both_paths(ds, h, use_nl, use_el):
    from dummynode4graphlearning_amd import ops
    gk, d = _gk(), _data(ds)
    with ops.wl_fused(True):
        fused = gk.wl_colors(d, h, use_nl, use_el)
    with ops.wl_fused(False):
        composed = gk.wl_colors(d, h, use_nl, use_el)
    return fused, composed


def _assert_colors(ds, h, use_nl, use_el):
    fused, composed = _colors_both_paths(ds, h, use_nl, use_el)
    _, cols, _ = C.ref(ds, h, use_nl, use_el)
    assert fused.shape == composed.shape == (h + 1, len(ds["graph_indicator"])) and fused.dtype == torch.int64
    for it in range(h + 1):
        want = [x for c in cols for x in c[it]]
        assert _u(fused[it]) == want, "fused, iteration %d" % it
        assert _u(composed[it]) == want, "composed, iteration %d" % it
    assert torch.equal(fused, composed)


@pytest.mark.parametrize("name", sorted(GOLD))
def test_colors_golden(name):
    _assert_colors(GOLD[name], H, *_gk().dataset_flags(name))


@pytest.mark.parametrize("use_el", [False, True])
def test_colors_at_the_sorts_boundaries(use_el):
    cap = _limits()[0]
    ds = C.stars(cap)
    d = _data(ds)
    p = d.plan(use_el)
    counts = sorted(set(((d.ptr[1:] - d.ptr[:-1]) * (2 if use_el else 1)).tolist()))
    want = [0, 2, 62, 64, 66, 126, 128, 130, cap - 2, cap, cap + 2] if use_el else [0, 1, 63, 64, 65, 127, 128, 129, cap - 1, cap, cap + 1]
    assert set(want) <= set(counts)
    assert all(x.numel() for x in (p.small, p.wave, p.block, p.huge)) and p.block_lds == cap        # every launch and the cap's overflow
    _assert_colors(ds, 2, True, use_el)
    _assert_colors(ds, 1, False, use_el)


@pytest.mark.parametrize("name", ["DUMMY_BIG", "QUIRKS", "REDDIT-BINARY"])
def test_features(name):
    gk, ds = _gk(), GOLD[name]
    flags = gk.dataset_flags(name)
    f = gk.wl_features(_data(ds), H, *flags)
    _, _, feats = C.ref(ds, H, *flags)
    ptr = f.ptr.tolist()
    assert f.num_graphs == len(feats) and f.num_steps == H + 1 and f.max_row == max(len(v) for v, _, _ in feats)
    assert ptr == [sum(len(v) for v, _, _ in feats[:g]) for g in range(len(feats) + 1)]
    assert _u(f.color) == [x for v, _, _ in feats for x in v]
    assert f.count.tolist() == [x for _, c, _ in feats for x in c]
    assert f.step.tolist() == [x for _, _, s in feats for x in s]


def _assert_gram(ds, h, use_nl, use_el):
    gk, d = _gk(), _data(ds)
    _, _, feats = C.ref(ds, h, use_nl, use_el)
    f = gk.wl_features(d, h, use_nl, use_el)
    out = {}
    for kernel in ("WL", "WLOA"):
        Gs = gk.wl_gram_matrices(d, h, kernel, use_nl, use_el, features=f)
        want = wl_ref.gram(feats, h, kernel)
        assert len(Gs) == h + 1
        for s in range(h + 1):
            assert Gs[s].dtype == torch.int64 and Gs[s].shape == (d.num_graphs, d.num_graphs)
            assert Gs[s].tolist() == want[s], (kernel, s)
            assert torch.equal(Gs[s], Gs[s].t())
        out[kernel] = (Gs, want)
    return out


@pytest.mark.parametrize("name", sorted(GOLD))
def test_gram_golden(name):
    _assert_gram(GOLD[name], H, *_gk().dataset_flags(name))


@pytest.mark.parametrize("which", ["1", "tile-1", "tile", "tile+1", "2tile+3"])
def test_gram_tile_boundaries(which):
    tile = _limits()[1]
    B = {"1": 1, "tile-1": tile - 1, "tile": tile, "tile+1": tile + 1, "2tile+3": 2 * tile + 3}[which]
    _assert_gram(C.take(C.mixed(2 * tile + 3), B), 3, True, True)


def test_gram_of_graphs_without_a_common_colour():
    rng = C.random.Random(3)
    ds = C.assemble("DISJOINT", [C.random_graph(rng, 6, 0.5, [1, 2], [1]), C.random_graph(rng, 7, 0.5, [1 << 40, (1 << 40) + 1], [1]),
                                 C.random_graph(rng, 5, 0.5, [1, 2], [1])])
    for kernel, (Gs, want) in _assert_gram(ds, 3, True, True).items():
        assert all(want[s][0][1] == 0 and want[s][1][2] == 0 for s in range(4)) and want[3][0][2] > 0


def test_gram_with_rows_far_longer_than_their_neighbours():
    """Two 200-node graphs among graphs of a few nodes, at the kernel's largest number of steps: rows of about 3000 entries joined with
    rows of a few dozen, with each other and with themselves.  The gram kernel keeps no rows in LDS (a stage was measured slower,
    docs/LAB_NOTES.md), so no row length takes another path; what a workgroup holds at once is its buckets, and this case fills all
    of them."""
    S = _limits()[2]
    rng = C.random.Random(11)
    ds = C.assemble("LONGROW", [C.random_graph(rng, n, p, [1, 2, 3], [1, 2]) for n, p in ((5, 0.5), (200, 0.04), (6, 0.5), (200, 0.04), (4, 0.6))])
    _, _, feats = C.ref(ds, S - 1, True, True)
    assert max(len(v) for v, _, _ in feats) > 2500 and max(max(s) for _, _, s in feats) == S - 1
    _assert_gram(ds, S - 1, True, True)


def test_command_line_end_to_end(tmp_path, capsys):
    gk = _gk()
    data, out = tmp_path / "data", tmp_path / "gram"
    out.mkdir()
    for i, ds in enumerate(GOLD.values()):
        C.write_tu(ds, str(data), raw=bool(i % 2))
    for kernel, stem in (("WL", "WL1"), ("WLOA", "WLOA")):
        assert gk.main(["--dataset_dir", str(data), "--gram_dir", str(out), "--k", "1", "--kernel", kernel, "--n_iters", str(H),
                        "--device", DEV, "--datasets"] + list(GOLD)) == 0
        for name, ds in GOLD.items():
            for h in range(H + 1):
                with open(out / ("%s__%s_%d.gram" % (name, stem, h)), "rb") as f:
                    assert f.read() == ds["grams"]["%s_%d" % (stem, h)].encode(), (name, kernel, h)
    said = capsys.readouterr().out
    assert "Warning: TOYA is not a valid dataset." in said and "Warning: NCI1" not in said and "WLOA-%d\tQUIRKS\t" % H in said


def test_two_runs_are_equal():
    gk = _gk()
    ds = GOLD["DUMMY_BIG"]
    a, b = _colors_both_paths(ds, H, True, True), _colors_both_paths(ds, H, True, True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    d = _data(ds)
    f = gk.wl_features(d, H)
    for kernel in ("WL", "WLOA"):
        x, y = gk.wl_gram_matrices(d, H, kernel, features=f), gk.wl_gram_matrices(d, H, kernel, features=gk.wl_features(d, H))
        assert all(torch.equal(p, q) for p, q in zip(x, y))


def test_refinement_and_gram_read_nothing_back():
    """wl_colors (both paths; STARS also takes the composed path for its lists above the cap) and the gram launch under torch's sync
    debug mode "error" -- after checking that this build honours the mode at all.  The node classes were built with the dataset and
    the feature build read its two sizes (entries, longest row) before."""
    from dummynode4graphlearning_amd import ops
    gk = _gk()
    d, s = _data(GOLD["DUMMY_BIG"]), _data(C.stars(_limits()[0]))
    f = gk.wl_features(d, H)                                       # (first use: library load, plans, allocator)
    gk.wl_colors(s, 1, True, True)
    probe = torch.ones(1, device=DEV)
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            probe.item()                                           # the mode is honoured: a plain read-back raises
        with ops.wl_fused(True):
            a = gk.wl_colors(d, H)
            gk.wl_colors(s, 1, True, True)
        with ops.wl_fused(False):
            b = gk.wl_colors(d, H)
        Gs = gk.wl_gram_matrices(d, H, "WL", features=f) + gk.wl_gram_matrices(d, H, "WLOA", features=f)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    assert torch.equal(a, b) and len(Gs) == 2 * (H + 1)
