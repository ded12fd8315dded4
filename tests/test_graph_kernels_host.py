"""Host tests of the WL / WLOA graph kernels (dummynode4graphlearning_amd/graph_kernels.py): no GPU.

* tests/wl_ref.py, the plain-Python restatement the GPU tests use as their reference, reproduces every entry of every .gram file the
  reference's own binary wrote (tests/golden/graph_kernels.json), as text;
* write_libsvm on the restatement's integer matrices reproduces those files byte for byte;
* the reader: the quirks of the QUIRKS dataset, the directory layouts, and every refusal;
* dataset_flags restates the binary's table; the command line rejects what is not built.
"""
import numpy as np
import pytest

import wl_cases as C
import wl_ref

H, GOLD = C.golden()
STEMS = (("WL", "WL1"), ("WLOA", "WLOA"))
# what the binary's table says about the goldens' names (gram.cpp:17-36; names outside it get (true, true))
FLAGS = {"TOYA": (True, True), "DUMMY_BIG": (True, True), "NCI1": (True, False), "REDDIT-BINARY": (False, False), "QUIRKS": (True, True)}


def _gk():
    from dummynode4graphlearning_amd import graph_kernels
    return graph_kernels


def _cpu(ds):
    return _gk().GraphKernelData.from_arrays(ds["graph_indicator"], ds["A"], ds["node_labels"], ds["edge_labels"], ds["graph_labels"],
                                             device="cpu")


def test_dataset_flags_match_the_goldens_names():
    gk = _gk()
    assert sorted(FLAGS) == sorted(GOLD)
    for name, flags in FLAGS.items():
        assert gk.dataset_flags(name) == flags, name
        assert (name in gk.DATASET_FLAGS) == (name in ("NCI1", "REDDIT-BINARY"))
    assert gk.dataset_flags("MUTAG") == (True, True) and gk.dataset_flags("ENZYMES") == (True, False)
    assert len(gk.DATASET_FLAGS) == 17


@pytest.mark.parametrize("name", sorted(FLAGS))
def test_restatement_and_writer_reproduce_the_binary(name, tmp_path):
    gk = _gk()
    ds = GOLD[name]
    use_nl, use_el = gk.dataset_flags(name)
    graphs, _, feats = C.ref(ds, H, use_nl, use_el)
    for kernel, stem in STEMS:
        Gs = wl_ref.gram(feats, H, kernel)
        for h in range(H + 1):
            want = ds["grams"]["%s_%d" % (stem, h)]
            assert wl_ref.libsvm_text(Gs[h], ds["graph_labels"]) == want, (kernel, h)
            path = str(tmp_path / ("%s_%d.gram" % (stem, h)))
            gk.write_libsvm(Gs[h], ds["graph_labels"], path)
            with open(path, "rb") as f:
                assert f.read() == want.encode(), (kernel, h)
            assert gk.gram_file("G", name, kernel, h) == "G/%s__%s_%d.gram" % (name, stem, h)


def test_the_big_golden_wraps_and_reorders():
    """DUMMY_BIG is only a test of the ordering quirk if some colour's step differs from the iteration that made it."""
    _, cols, feats = C.ref(GOLD["DUMMY_BIG"], H, True, True)
    moved = 0
    for c, (vals, _, steps) in zip(cols, feats):
        made = {}
        for h, row in enumerate(c):
            for x in row:
                made.setdefault(x, h)
        moved += sum(made[v] != s for v, s in zip(vals, steps))
    assert moved > 0


def test_normalize_gram_is_the_references_expression():
    import torch
    gk = _gk()
    G = torch.tensor([[4, 2, 0], [2, 9, 0], [0, 0, 0]])
    n = gk.normalize_gram(G)
    assert n.dtype == torch.float64
    assert n.tolist() == [[1.0, 2 / (2.0 * 3.0), 0.0], [2 / (3.0 * 2.0), 1.0, 0.0], [0.0, 0.0, 0.0]]


def test_reader_quirks():
    ds = GOLD["QUIRKS"]
    d = _cpu(ds)
    ptr, nbr, el = d.ptr.tolist(), d.nbr.tolist(), d.edge_label.tolist()
    assert d.num_graphs == 4 and d.node_ptr.tolist() == [0, 4, 5, 8, 10]
    adj = [nbr[ptr[v]:ptr[v + 1]] for v in range(d.num_nodes)]
    lab = [el[ptr[v]:ptr[v + 1]] for v in range(d.num_nodes)]
    assert adj[0] == [1] and adj[1] == [0, 2] and adj[2] == [1]          # the repeated line 1,2 adds nothing
    assert adj[3] == [] and adj[4] == []                                 # an isolated node, a one-node graph
    assert adj[5] == [6] and adj[6] == [5, 7] and adj[7] == [6]          # a path given in one direction only is undirected
    assert lab[0] == [1] and lab[1] == [1, 2] and lab[2] == [2]          # the FIRST line that names a pair labels both directions
    assert adj[8] == [9] and adj[9] == [8] and lab[8] == [2] and lab[9] == [2]
    # ... and all of it as the restatement reads it
    for G, n0 in zip(wl_ref.read_graphs(ds["graph_indicator"], ds["A"], ds["node_labels"], ds["edge_labels"]), d.node_ptr.tolist()):
        for v in range(G["n"]):
            assert sorted(G["nbrs"][v]) == [w - n0 for w in adj[n0 + v]]
            assert [G["elabel"][(v, w - n0)] for w in adj[n0 + v]] == lab[n0 + v]


@pytest.mark.parametrize("raw", [False, True])
def test_from_dir_reads_both_layouts(tmp_path, raw):
    gk = _gk()
    for name in ("QUIRKS", "REDDIT-BINARY"):
        C.write_tu(GOLD[name], str(tmp_path), raw=raw)
        a, b = gk.GraphKernelData.from_dir(str(tmp_path), name, device="cpu"), _cpu(GOLD[name])
        assert a.classes == GOLD[name]["graph_labels"]
        for k in ("node_ptr", "ptr", "nbr", "edge_label", "node_label"):
            x, y = getattr(a, k), getattr(b, k)
            assert (x is None and y is None) or x.tolist() == y.tolist(), k
    assert a.node_label is None and a.edge_label is None


def test_from_arrays_takes_a_batch():
    """batch = the tensors of a tu_io.TUBatch (0-based global endpoints, node_ptr) instead of the raw arrays"""
    import torch
    ds = GOLD["TOYA"]
    gi, A = np.array(ds["graph_indicator"]), np.array(ds["A"])
    batch = dict(node_ptr=torch.tensor(np.concatenate([[0], np.cumsum(np.bincount(gi - 1))]), dtype=torch.int32),
                 src=torch.tensor(A[:, 0] - 1, dtype=torch.int32), dst=torch.tensor(A[:, 1] - 1, dtype=torch.int32),
                 node_label=torch.tensor(ds["node_labels"], dtype=torch.int32), edge_label=torch.tensor(ds["edge_labels"], dtype=torch.int32))
    a, b = _gk().GraphKernelData.from_arrays(batch=batch, graph_labels=ds["graph_labels"], device="cpu"), _cpu(ds)
    for k in ("node_ptr", "ptr", "nbr", "edge_label", "node_label"):
        assert getattr(a, k).tolist() == getattr(b, k).tolist(), k


def test_unsigned_64_bit_node_labels(tmp_path):
    gk = _gk()
    ds = dict(name="U64", graph_indicator=[1, 1], A=[[1, 2], [2, 1]], node_labels=[(1 << 64) - 1, 1 << 63], edge_labels=[7, 7],
              graph_labels=[3])
    C.write_tu(ds, str(tmp_path))
    d = gk.GraphKernelData.from_dir(str(tmp_path), "U64", device="cpu")
    assert d.node_label.tolist() == [-1, -(1 << 63)]                     # the unsigned bit patterns


def test_refusals(tmp_path):
    gk = _gk()
    base = dict(name="BAD", graph_indicator=[1, 1, 1, 2, 2], A=[[1, 2], [2, 1], [3, 3], [4, 5]], node_labels=[1, 1, 1, 1, 1],
                edge_labels=[1, 1, 1, 1], graph_labels=[0, 1])
    C.write_tu(base, str(tmp_path))
    with pytest.raises(ValueError, match=r"BAD_A\.txt:3: self loop"):
        gk.GraphKernelData.from_dir(str(tmp_path), "BAD", device="cpu")
    with pytest.raises(ValueError, match="self loop"):
        _cpu(base)
    with pytest.raises(ValueError, match=r"BAD_A\.txt:3: .*different graphs"):
        C.write_tu(dict(base, A=[[1, 2], [2, 1], [3, 4], [4, 5]]), str(tmp_path))
        gk.GraphKernelData.from_dir(str(tmp_path), "BAD", device="cpu")
    with pytest.raises(ValueError, match=r"BAD_edge_labels\.txt:2: .*32-bit"):
        C.write_tu(dict(base, A=[[1, 2], [2, 1], [2, 3], [4, 5]], edge_labels=[1, 1 << 32, 1, 1]), str(tmp_path))
        gk.GraphKernelData.from_dir(str(tmp_path), "BAD", device="cpu")
    # labels wanted, no label file
    C.write_tu(GOLD["REDDIT-BINARY"], str(tmp_path))
    d = gk.GraphKernelData.from_dir(str(tmp_path), "REDDIT-BINARY", device="cpu")
    for fn in (gk.wl_colors, gk.wl_features, gk.wl_gram_matrices):
        with pytest.raises(ValueError, match=r"REDDIT-BINARY_node_labels\.txt: use_node_labels without"):
            fn(d, 2, use_node_labels=True, use_edge_labels=False)
        with pytest.raises(ValueError, match=r"REDDIT-BINARY_edge_labels\.txt: use_edge_labels without"):
            fn(d, 2, use_node_labels=False, use_edge_labels=True)
    # MAXNUMCOLOR's early stop is not built: more than 1,000,000 / (H + 1) nodes in one graph
    big = _cpu(dict(name="BIGG", graph_indicator=[1] * 11 + [2], A=[[1, 2], [2, 1]], node_labels=None, edge_labels=None,
                    graph_labels=[0, 1]))
    with pytest.raises(ValueError, match=r"graph 1 has 11 nodes, more than 1000000 / \(H \+ 1\) = 10"):
        gk.wl_colors(big, 99999, use_node_labels=False, use_edge_labels=False)
    with pytest.raises(ValueError, match="not built"):
        gk.wl_gram_matrices(big, 1, "SP", False, False)
    with pytest.raises(ValueError, match="graph labels"):
        _cpu(dict(base, A=[[1, 2]], edge_labels=[1], graph_labels=[0]))
    with pytest.raises(ValueError, match=r"\[node_labels\]:5: 4 labels for 5 nodes"):
        _cpu(dict(base, A=[[1, 2]], edge_labels=[1], node_labels=[1, 1, 1, 1]))


@pytest.mark.parametrize("argv", [["--k", "2"], ["--k", "3", "--kernel", "WL"], ["--kernel", "SP"], ["--kernel", "GR"],
                                  ["--k", "2", "--kernel", "LWL"]])
def test_command_line_rejects_what_is_not_built(argv, capsys):
    with pytest.raises(SystemExit) as e:
        _gk().main(argv + ["--datasets", "NCI1"])
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert "not built" in err and "--kernel WL" in err and "WLOA" in err


def test_package_exports():
    import dummynode4graphlearning_amd as pkg
    from dummynode4graphlearning_amd import ops
    for name in ("GraphKernelData", "wl_colors", "wl_features", "wl_gram_matrices", "normalize_gram", "write_libsvm", "dataset_flags"):
        assert getattr(pkg, name) is getattr(pkg.graph_kernels, name)
    assert ops.wl_fused_enabled() == ops.WL_FUSED_DEFAULT
    with ops.wl_fused(False):
        assert not ops.wl_fused_enabled()
        with ops.wl_fused(True):
            assert ops.wl_fused_enabled()
        assert not ops.wl_fused_enabled()
    assert ops.wl_fused_enabled() == ops.WL_FUSED_DEFAULT
    assert np.int64(ops._WL_SIGN) == np.iinfo(np.int64).min
