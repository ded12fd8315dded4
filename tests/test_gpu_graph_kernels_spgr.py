"""GPU tests of the SP / GR graph kernels (graph_kernels_spgr.py on dn_gk.hip) against the plain-Python restatement
tests/spgr_ref.py, which tests/test_graph_kernels_spgr_host.py holds against the reference binary's own output.  Everything is exact
integer arithmetic, so every comparison is equality.

* every golden dataset under its flags: fused and composed features equal the restatement's per-graph dictionaries (SP keys decoded
  from their ranks), the matrices equal its matrices, the command line's files equal the golden text;
* SP: graphs of 63 / 64 / 65 nodes, a graph one node below, at and above the workgroup class's cap (the kernel's own and a lowered
  one), the 300-node path, unreachable pairs, isolated and single nodes, the label filter;
* GR: centre degrees at the boundaries of the three launches and of the hub's work items, the 69-degree hub, K4 with edge labels, the
  unlabelled keys, several chunks of a small key workspace;
* determinism, and no read-back in the gram step once the features exist.
"""
import pytest
import torch

import spgr_cases as S
import wl_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLD = S.golden()
INT_MAX = 2147483647


def _m():
    from dummynode4graphlearning_amd import graph_kernels_spgr
    return graph_kernels_spgr


def _ops():
    from dummynode4graphlearning_amd import ops
    return ops


_DATA = {}


def _data(ds):
    if ds["name"] not in _DATA:
        _DATA[ds["name"]] = _m().GraphKernelData.from_arrays(ds["graph_indicator"], ds["A"], ds["node_labels"], ds["edge_labels"],
                                                             ds["graph_labels"], device=DEV)
    return _DATA[ds["name"]]


def _same(f, g):
    return all(torch.equal(getattr(f, a), getattr(g, a)) for a in ("ptr", "color", "count", "step")) and f.max_row == g.max_row


def _assert_sp(ds, use_nl, **kw):
    m, ops, d = _m(), _ops(), _data(ds)
    feats, G = S.ref_sp(ds, use_nl)
    with ops.gk_fused(True):
        fused = m.sp_features(d, use_nl, **kw)
    with ops.gk_fused(False):
        composed = m.sp_features(d, use_nl)
    assert S.sp_decode(ds, use_nl, fused) == feats, "fused"
    assert S.sp_decode(ds, use_nl, composed) == feats, "composed"
    assert _same(fused, composed)
    got = m.sp_gram_matrix(d, use_nl, features=fused)
    assert got.dtype == torch.int64 and got.is_cuda and got.cpu().tolist() == G
    return fused


def _assert_gr(ds, use_nl, use_el, **kw):
    m, ops, d = _m(), _ops(), _data(ds)
    feats, G = S.ref_gr(ds, use_nl, use_el)
    with ops.gk_fused(True):
        fused = m.gr_features(d, use_nl, use_el, **kw)
    with ops.gk_fused(False):
        composed = m.gr_features(d, use_nl, use_el, **kw)
    assert [dict(r) for r in S.rows(fused)] == feats, "fused"
    assert [dict(r) for r in S.rows(composed)] == feats, "composed"
    assert _same(fused, composed)
    got = m.gr_gram_matrix(d, use_nl, use_el, features=fused)
    assert got.dtype == torch.int64 and got.is_cuda and got.cpu().tolist() == G
    return fused


@pytest.mark.parametrize("name", sorted(S.FLAGS))
def test_sp_golden(name):
    _assert_sp(GOLD[name], S.FLAGS[name][0])


@pytest.mark.parametrize("name", sorted(S.FLAGS))
def test_gr_golden(name):
    _assert_gr(GOLD[name], *S.FLAGS[name])


def test_sp_edges_graph_by_graph():
    """EDGES holds the wavefront class's boundary (63 / 64 / 65 nodes), the 300-node path, and the graphs whose pairs are unreachable."""
    m, ds = _m(), GOLD["EDGES"]
    plan = m._sp_plan(_data(ds), True, _ops().gk_sp_lds_max_nodes())
    assert [int(plan.sizes[g]) for g in plan.wave] == [2, 1, 3, 63, 64, 4] and [int(plan.sizes[g]) for g in plan.block] == [300, 65, 65, 128, 70]
    got = S.sp_decode(ds, True, _assert_sp(ds, True))
    assert max(d for (_, _, d) in got[S.EDGES_PATH] if d != INT_MAX) == 299 and got[S.EDGES_PATH][(1, 3, 299)] == 1
    assert got[S.EDGES_SINGLE] == {(2, 2, INT_MAX): 2}
    assert got[S.EDGES_PAIR] == {(1, 2, 1): 1, (2, 1, 1): 1, (1, 1, 2): 2, (2, 2, 2): 2}
    assert got[S.EDGES_EDGELESS] == {(1, 1, INT_MAX): 6, (1, 3, INT_MAX): 2, (3, 1, INT_MAX): 2, (3, 3, INT_MAX): 2}
    _assert_sp(ds, False)                                        # without node labels: one class, nothing filtered


def test_sp_label_filter():
    """lo32(l_a) of 0 (labels 0, 2^32, 2^63) and of INT_MAX never start a triple; 2^32 + 1 starts the triples of label 1."""
    got = S.sp_decode(GOLD["LABELS"], True, _assert_sp(GOLD["LABELS"], True))
    assert set(la for f in got for (la, _, _) in f) == {1, (1 << 32) - 1}
    assert {0, 2147483647, 1 << 32, (1 << 32) + 1, 1 << 63, (1 << 64) - 1} <= set(lb for f in got for (_, lb, _) in f)
    _assert_sp(GOLD["QUIRKS"], True)                             # an isolated node beside a component, a single node


@pytest.mark.parametrize("cap", [None, 100])
def test_sp_at_the_workgroup_class_cap(cap):
    """Graphs one node below, at and above the cap of the workgroup class: the kernel's own (None) and a lowered one.  The graph above
    it takes the composed path inside the fused build."""
    m = _m()
    top = _ops().gk_sp_lds_max_nodes() if cap is None else cap
    ds = S.sp_sizes([top - 1, top, top + 1, 64, 65], "CAP%d" % top)
    plan = m._sp_plan(_data(ds), True, top)
    assert plan.wave.tolist() == [3] and plan.block.tolist() == [0, 1, 4] and plan.large.tolist() == [2] and plan.block_nodes == top
    feats = S.ref_sp(ds, True)[0]
    assert all(any(d == INT_MAX for (_, _, d) in f) and max(d for (_, _, d) in f if d != INT_MAX) >= 5 for f in feats[:3])
    _assert_sp(ds, True, **({} if cap is None else {"lds_max_nodes": cap}))
    with pytest.raises(ValueError, match="lds_max_nodes must be 64 .."):
        m.sp_features(_data(ds), True, lds_max_nodes=_ops().gk_sp_lds_max_nodes() + 1)


@pytest.mark.parametrize("use_nl,use_el", [(True, True), (True, False), (False, False)])
def test_gr_at_the_launch_boundaries(use_nl, use_el):
    """DEGREES: centres of 4 / 5 neighbours (8 pairs), 11 / 12 (64 pairs), and hubs of 64 / 65 / 100 (one, two, three work items)."""
    m, ds = _m(), S.gr_degrees()
    plan = m._gr_plan(_data(ds), m.GR_WORKSPACE_KEYS)
    assert len(plan.chunks) == 1 and [g for g, *_ in plan.chunks[0]["lists"]] == [8, 64, 0]
    hub_items = plan.chunks[0]["lists"][2][1].tolist()
    assert sorted(hub_items.count(v) for v in set(hub_items)) == [1, 1, 1, 2, 3]        # degrees 12, 13, 64 | 65 | 100
    f = _assert_gr(ds, use_nl, use_el)
    if not use_nl:
        assert set(k for r in S.rows(f) for k, _ in r) == {2, 3}


def test_gr_hub_k4_and_unlabelled_keys():
    ds = GOLD["EDGES"]
    got = [dict(r) for r in S.rows(_assert_gr(ds, True, True))]
    want = S.ref_gr(ds, True, True)[0]
    assert got[S.EDGES_STAR] == want[S.EDGES_STAR] and sum(want[S.EDGES_STAR].values()) >= 69 * 68 // 2
    assert got[S.EDGES_K4] == want[S.EDGES_K4] and sum(got[S.EDGES_K4].values()) == 4 and len(got[S.EDGES_K4]) >= 2
    _assert_gr(ds, True, False)
    plain = [dict(r) for r in S.rows(_assert_gr(GOLD["REDDIT-BINARY"], False, False))]
    assert set(k for f in plain for k in f) == {2, 3}
    assert [dict(r) for r in S.rows(_assert_gr(ds, False, True))][S.EDGES_K4] == {3: 4}


def test_gr_in_several_chunks():
    m, ds = _m(), GOLD["DUMMY_BIG"]
    one = _assert_gr(ds, True, True)
    for cap in (4096, 1000):
        assert len(m._gr_plan(_data(ds), cap).chunks) >= 3
        assert _same(one, _assert_gr(ds, True, True, workspace_keys=cap))
    deg = S.gr_degrees()
    assert len(m._gr_plan(_data(deg), 3000).chunks) > 3          # the 100-degree hub's three items fall into different chunks
    assert _same(_assert_gr(deg, True, True), _assert_gr(deg, True, True, workspace_keys=3000))


def test_command_line_end_to_end(tmp_path, capsys):
    m = _m()
    data, out = tmp_path / "data", tmp_path / "gram"
    out.mkdir()
    for i, ds in enumerate(GOLD.values()):
        C.write_tu(ds, str(data), raw=bool(i % 2))
    for kernel in ("SP", "GR"):
        assert m.main(["--dataset_dir", str(data), "--gram_dir", str(out), "--k", "1", "--kernel", kernel, "--n_iters", "2",
                       "--device", DEV, "--datasets"] + list(GOLD)) == 0
        for name, ds in GOLD.items():
            with open(out / ("%s__%s_0.gram" % (name, kernel)), "rb") as f:
                assert f.read() == ds["grams"][kernel + "_0"].encode(), (name, kernel)
    said = capsys.readouterr().out
    assert "Warning: LABELS is not a valid dataset." in said and "Warning: NCI1" not in said and "SP-2\tEDGES\t" in said
    assert m.main(["--dataset_dir", str(data), "--gram_dir", str(out), "--kernel", "WL", "--n_iters", str(C.golden()[0]), "--device", DEV,
                   "--datasets", "NCI1"]) == 0
    with open(out / "NCI1__WL1_1.gram", "rb") as f:                 # WL is handed to graph_kernels.main
        assert f.read() == C.golden()[1]["NCI1"]["grams"]["WL1_1"].encode()


def test_two_runs_are_equal():
    m, ops = _m(), _ops()
    for ds in (GOLD["EDGES"], GOLD["DUMMY_BIG"]):
        d = _data(ds)
        with ops.gk_fused(True):
            a, b = m.sp_features(d, True), m.sp_features(d, True)
            x, y = m.gr_features(d, True, True, workspace_keys=5000), m.gr_features(d, True, True, workspace_keys=5000)
        assert _same(a, b) and _same(x, y)
        assert torch.equal(m.sp_gram_matrix(d, True, features=a), m.sp_gram_matrix(d, True, features=b))
        assert torch.equal(m.gr_gram_matrix(d, True, True, features=x), m.gr_gram_matrix(d, True, True, features=y))


def test_the_gram_step_reads_nothing_back():
    """With the features built, sp_gram_matrix / gr_gram_matrix are one launch each: run under torch's sync debug mode "error", after
    checking that this build honours the mode at all."""
    m = _m()
    d = _data(GOLD["DUMMY_BIG"])
    fs, fg = m.sp_features(d, True), m.gr_features(d, True, True)
    want = (m.sp_gram_matrix(d, True, features=fs), m.gr_gram_matrix(d, True, True, features=fg))
    probe = torch.ones(1, device=DEV)
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            probe.item()                                           # the mode is honoured: a plain read-back raises
        got = (m.sp_gram_matrix(d, True, features=fs), m.gr_gram_matrix(d, True, True, features=fg))
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
