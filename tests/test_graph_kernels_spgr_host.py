"""Host tests of the SP / GR graph kernels (dummynode4graphlearning_amd/graph_kernels_spgr.py): no GPU.

* tests/spgr_ref.py, the plain-Python restatement the GPU tests use as their reference, reproduces through write_libsvm every
  .gram file the reference's own binary wrote (tests/golden/graph_kernels_spgr.json), byte for byte;
* the composed path on CPU tensors gives the restatement's integer matrices and features on every golden dataset;
* GR in several chunks of a small key workspace gives the features of one chunk;
* every refusal; the new command line writes the golden files and hands WL / WLOA on; the old one still refuses SP / GR.
"""
import numpy as np
import pytest
import torch

import spgr_cases as S
import wl_cases as C

GOLD = S.golden()
INT_MAX = 2147483647


def _m():
    from dummynode4graphlearning_amd import graph_kernels_spgr
    return graph_kernels_spgr


_CPU = {}


def _cpu(ds):
    if ds["name"] not in _CPU:
        _CPU[ds["name"]] = _m().GraphKernelData.from_arrays(ds["graph_indicator"], ds["A"], ds["node_labels"], ds["edge_labels"],
                                                            ds["graph_labels"], device="cpu")
    return _CPU[ds["name"]]


def test_the_goldens_are_the_issues_cases():
    m = _m()
    assert sorted(GOLD) == sorted(S.FLAGS)
    for name, flags in S.FLAGS.items():
        assert m.dataset_flags(name) == flags, name
        assert sorted(GOLD[name]["grams"]) == ["GR_0", "SP_0"]
    ds = GOLD["EDGES"]
    sizes = np.bincount(np.array(ds["graph_indicator"]) - 1).tolist()
    assert sizes == S.EDGES_SIZES
    deg = np.bincount(np.array(ds["A"])[:, 0] - 1, minlength=len(ds["graph_indicator"]))
    star0 = sum(sizes[:S.EDGES_STAR])
    assert deg[star0] == 69 and deg[:300].max() == 2 and deg[302:306].sum() == 0
    for g in (7, 8):                                             # the dummy node: label 0, joined to every node by edges labelled 0
        last = sum(sizes[:g + 1]) - 1
        assert ds["node_labels"][last] == 0 and deg[last] == sizes[g] - 1
        assert all(el == 0 for (v, w), el in zip(ds["A"], ds["edge_labels"]) if v - 1 == last)
    assert set(GOLD["LABELS"]["node_labels"]) == {0, 1, 2147483647, 1 << 32, (1 << 32) + 1, 1 << 63, (1 << 64) - 1}


@pytest.mark.parametrize("name", sorted(S.FLAGS))
def test_restatement_and_writer_reproduce_the_binary(name, tmp_path):
    m = _m()
    ds = GOLD[name]
    use_nl, use_el = S.FLAGS[name]
    for kernel, G in (("SP", S.ref_sp(ds, use_nl)[1]), ("GR", S.ref_gr(ds, use_nl, use_el)[1])):
        path = str(tmp_path / (kernel + ".gram"))
        m.write_libsvm(G, ds["graph_labels"], path)
        with open(path, "rb") as f:
            assert f.read() == ds["grams"][kernel + "_0"].encode(), kernel
        assert m.gram_file("G", name, kernel) == "G/%s__%s_0.gram" % (name, kernel)


def test_the_restatements_quirks():
    """What the goldens pin, spelled out on EDGES and LABELS."""
    ds = GOLD["EDGES"]
    sp = S.ref_sp(ds, True)[0]
    assert max(d for (_, _, d) in sp[S.EDGES_PATH] if d != INT_MAX) == 299
    assert sp[S.EDGES_SINGLE] == {(2, 2, INT_MAX): 2}                                     # a single node: its diagonal, at INT_MAX
    assert sp[S.EDGES_PAIR] == {(1, 2, 1): 1, (2, 1, 1): 1, (1, 1, 2): 2, (2, 2, 2): 2}   # the diagonal of a node with a neighbour: 2
    assert sp[S.EDGES_EDGELESS] == {(1, 1, INT_MAX): 6, (1, 3, INT_MAX): 2, (3, 1, INT_MAX): 2, (3, 3, INT_MAX): 2}
    assert all(la != 0 for f in sp for (la, _, _) in f) and any(lb == 0 for (_, lb, _) in sp[7])    # the dummy: as b, never as a
    lab = S.ref_sp(GOLD["LABELS"], True)[0]
    firsts = set(la for f in lab for (la, _, _) in f)
    assert firsts == {1, (1 << 32) - 1} and {1 << 32, (1 << 32) + 1, 1 << 63, (1 << 64) - 1, 0, 2147483647} <= set(lb for f in lab for (_, lb, _) in f)
    gr = S.ref_gr(GOLD["REDDIT-BINARY"], False, False)[0]
    assert set(k for f in gr for k in f) == {2, 3}
    assert sum(S.ref_gr(ds, True, True)[0][S.EDGES_K4].values()) == 4                      # K4: four triangles, no wedge


@pytest.mark.parametrize("name", sorted(S.FLAGS))
def test_composed_path_on_cpu_tensors(name):
    m = _m()
    ds, d = GOLD[name], _cpu(GOLD[name])
    use_nl, use_el = S.FLAGS[name]
    feats, G = S.ref_sp(ds, use_nl)
    f = m.sp_features(d, use_nl)
    assert S.sp_decode(ds, use_nl, f) == feats
    got = m.sp_gram_matrix(d, use_nl, features=f)
    assert got.dtype == torch.int64 and got.tolist() == G
    feats, G = S.ref_gr(ds, use_nl, use_el)
    f = m.gr_features(d, use_nl, use_el)
    assert [dict(r) for r in S.rows(f)] == feats
    got = m.gr_gram_matrix(d, use_nl, use_el)
    assert got.dtype == torch.int64 and got.tolist() == G


def test_gr_in_several_chunks():
    m = _m()
    d = _cpu(GOLD["DUMMY_BIG"])
    one = m.gr_features(d, True, True)
    assert len(m._gr_plan(d, m.GR_WORKSPACE_KEYS).chunks) == 1
    for cap in (4096, 1000):
        plan = m._gr_plan(d, cap)
        assert len(plan.chunks) >= 3 and all(0 < ch["used"] <= cap for ch in plan.chunks)
        assert sum(ch["used"] for ch in plan.chunks) == plan.pairs
        many = m.gr_features(d, True, True, workspace_keys=cap)
        for a in ("ptr", "color", "count", "step"):
            assert torch.equal(getattr(one, a), getattr(many, a)), (cap, a)
        assert many.max_row == one.max_row


def test_gr_work_items_cover_every_pair_once():
    """The hub rows of DEGREES are cut into items of about 2048 pairs; items and chunks partition the pairs of every centre."""
    m = _m()
    ds = S.gr_degrees()
    d = _cpu(ds)
    deg = np.diff(d._ptr_h)
    plan = m._gr_plan(d, 3000)
    seen = np.zeros(deg.size, dtype=np.int64)
    for ch in plan.chunks:
        used = 0
        for grp, node, r0, r1, off in ch["lists"]:
            for v, a, b, o in zip(node.tolist(), r0.tolist(), r1.tolist(), off.tolist()):
                size = sum(deg[v] - 1 - i for i in range(a, min(b, deg[v])))
                pairs = deg[v] * (deg[v] - 1) // 2
                assert grp == (8 if pairs <= 8 else 64 if pairs <= 64 else 0) and 0 <= o and o + size <= ch["used"]
                seen[v] += size
                used += size
        assert used == ch["used"] <= 3000
    assert (seen == deg * (deg - 1) // 2).all() and len(plan.chunks) > 3
    feats, _ = S.ref_gr(ds, True, True)
    assert [dict(r) for r in S.rows(m.gr_features(d, True, True, workspace_keys=3000))] == feats


def test_refusals(tmp_path):
    m = _m()
    ds = GOLD["REDDIT-BINARY"]
    C.write_tu(ds, str(tmp_path))
    d = m.GraphKernelData.from_dir(str(tmp_path), "REDDIT-BINARY", device="cpu")
    for fn in (m.sp_features, m.sp_gram_matrix, m.gr_features, m.gr_gram_matrix):
        with pytest.raises(ValueError, match=r"REDDIT-BINARY_node_labels\.txt: use_node_labels without"):
            fn(d, True)
    nci = dict(GOLD["NCI1"], name="NCI1")
    C.write_tu(nci, str(tmp_path))
    d = m.GraphKernelData.from_dir(str(tmp_path), "NCI1", device="cpu")
    with pytest.raises(ValueError, match=r"NCI1_edge_labels\.txt: use_edge_labels without"):
        m.gr_features(d, True, True)
    m.gr_features(d, False, True)                                # without node labels the edge labels are never read
    # SP: 2 n^2 must fit an int32 count
    n = 32768
    big = dict(name="WIDE", graph_indicator=[1] * n + [2], A=[[1, 2], [2, 1]], node_labels=None, edge_labels=None, graph_labels=[0, 1])
    C.write_tu(big, str(tmp_path))
    d = m.GraphKernelData.from_dir(str(tmp_path), "WIDE", device="cpu")
    with pytest.raises(ValueError, match=r"WIDE: graph 1 has 32768 nodes, more than 32767"):
        m.sp_features(d, False)
    m.gr_features(d, False, False)                               # GR has no such limit
    # SP: 65537 distinct labels, all with distinct low halves: 65537^2 > 2^32
    n = 65537
    many = dict(name="RANKS", graph_indicator=[1 + i // 8 for i in range(n)], A=[[1, 2], [2, 1]], node_labels=list(range(1, n + 1)),
                edge_labels=None, graph_labels=[0] * (1 + (n - 1) // 8))
    C.write_tu(many, str(tmp_path))
    d = m.GraphKernelData.from_dir(str(tmp_path), "RANKS", device="cpu")
    with pytest.raises(ValueError, match=r"RANKS: 65537 distinct 32-bit source labels x 65537 distinct labels .*rank overflow"):
        m.sp_features(d, True)
    m.sp_features(d, False)
    # GR: a workspace smaller than one work item
    with pytest.raises(ValueError, match=r"workspace_keys = 100 is smaller than one work item"):
        m.gr_features(_cpu(GOLD["DUMMY_BIG"]), True, True, workspace_keys=100)
    with pytest.raises(ValueError, match="workspace_keys must be positive"):
        m.gr_features(_cpu(GOLD["DUMMY_BIG"]), True, True, workspace_keys=0)


def test_command_line_on_cpu_tensors(tmp_path, capsys, monkeypatch):
    m = _m()
    data, out = tmp_path / "data", tmp_path / "gram"
    out.mkdir()
    for i, ds in enumerate(GOLD.values()):
        C.write_tu(ds, str(data), raw=bool(i % 2))
    for kernel in ("SP", "GR"):
        assert m.main(["--dataset_dir", str(data), "--gram_dir", str(out), "--k", "1", "--kernel", kernel, "--n_iters", "7",
                       "--device", "cpu", "--datasets"] + list(GOLD)) == 0
        for name, ds in GOLD.items():
            with open(out / ("%s__%s_0.gram" % (name, kernel)), "rb") as f:
                assert f.read() == ds["grams"][kernel + "_0"].encode(), (name, kernel)
    said = capsys.readouterr().out
    assert "Warning: EDGES is not a valid dataset." in said and "Warning: NCI1" not in said and "GR-7\tLABELS\t" in said
    assert sorted(p.name for p in out.iterdir()) == sorted("%s__%s_0.gram" % (n, k) for n in GOLD for k in ("SP", "GR"))
    # WL / WLOA are handed to graph_kernels.main with the same arguments
    calls = []
    monkeypatch.setattr(m.gk, "main", lambda argv=None: calls.append(list(argv)) or 0)
    for kernel in ("WL", "WLOA"):
        argv = ["--kernel", kernel, "--n_iters", "3", "--datasets", "NCI1"]
        assert m.main(argv) == 0 and calls[-1] == argv
    for argv in (["--k", "2", "--kernel", "SP"], ["--kernel", "LWL"], ["--k", "3", "--kernel", "GR"]):
        with pytest.raises(SystemExit) as e:
            m.main(argv + ["--datasets", "NCI1"])
        assert e.value.code == 2 and "not built" in capsys.readouterr().err


@pytest.mark.parametrize("kernel", ["SP", "GR"])
def test_the_old_command_line_still_refuses(kernel, capsys):
    from dummynode4graphlearning_amd import graph_kernels
    with pytest.raises(SystemExit) as e:
        graph_kernels.main(["--kernel", kernel, "--datasets", "NCI1"])
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert "not built" in err and "--kernel WL" in err and "WLOA" in err and "graph_kernels_spgr" in err
    with pytest.raises(ValueError, match="not built"):
        graph_kernels.wl_gram_matrices(None, 1, kernel)


def test_package_exports_and_toggle():
    import dummynode4graphlearning_amd as pkg
    from dummynode4graphlearning_amd import ops
    m = _m()
    for name in ("sp_features", "gr_features", "sp_gram_matrix", "gr_gram_matrix"):
        assert getattr(pkg, name) is getattr(m, name)
    assert pkg.graph_kernels_spgr is m and callable(m.main)
    for kernel in ("SP", "GR"):
        default = ops.gk_fused_enabled(kernel)
        assert default == ops.GK_FUSED_DEFAULT[kernel]
        with ops.gk_fused(False):
            assert not ops.gk_fused_enabled(kernel)
            with ops.gk_fused(True):
                assert ops.gk_fused_enabled(kernel)
            assert not ops.gk_fused_enabled(kernel)
        assert ops.gk_fused_enabled(kernel) == default
