"""Host tests of the 2-WL graph kernels (graph_kernels_kwl.py): no GPU.

* the plain-Python restatement tests/kwl_ref.py and the writer reproduce, byte for byte, every file the reference's own binary wrote
  for `--k 2 --kernel WL | DWL | LWL | LWLC --n_iters 2` (tests/golden/graph_kernels_kwl.json);
* the composed path's torch part on CPU tensors: it runs there except for the one kernel it ends in (dn_wl_fold_u64), which is
  restated here over the same host arrays -- so the entry construction, the segmented sort, the removal of the maxima and the final
  combination are held to the restatement, in one chunk and in chunks of a few entries;
* refusals, command-line routing, package exports and the switch.
"""
import ctypes

import pytest
import torch

import kwl_cases as C
import wl_cases
import wl_ref

H, GOLD = C.golden()
M64 = (1 << 64) - 1


def _m():
    from dummynode4graphlearning_amd import graph_kernels_kwl
    return graph_kernels_kwl


@pytest.fixture(scope="module", autouse=True)
def _library():
    """The plans ask the library for its limits (host calls)."""
    import os
    from dummynode4graphlearning_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()


def _cpu(ds):
    return _m().GraphKernelData.from_arrays(ds["graph_indicator"], ds["A"], ds["node_labels"], ds["edge_labels"], ds["graph_labels"],
                                            device="cpu")


@pytest.mark.parametrize("kernel", C.KERNELS)
@pytest.mark.parametrize("name", sorted(GOLD))
def test_restatement_reproduces_the_reference_binary(name, kernel):
    ds = GOLD[name]
    _, cols = C.ref(ds, H, kernel, *C.flags(name))                          # (cached: DUMMY_BIG / WL takes seconds)
    Gs = wl_ref.gram([wl_ref.features(c) for c in cols], H, "WL")
    assert sorted(k for k in ds["grams"] if k.startswith(kernel + "2_")) == ["%s2_%d" % (kernel, h) for h in range(H + 1)]
    for h in range(H + 1):
        assert wl_ref.libsvm_text(Gs[h], ds["graph_labels"]) == ds["grams"]["%s2_%d" % (kernel, h)], (name, kernel, h)


def test_the_goldens_cover_what_they_should():
    assert sorted(GOLD) == ["DUMMY_BIG", "NCI1", "QUIRKS", "REDDIT-BINARY", "TOYA", "TWOS"] and H == 2
    sizes = [GOLD["TWOS"]["graph_indicator"].count(g) for g in range(1, 6)]
    assert sizes == [1, 2, 2, 5, 6]
    _, cols = C.ref(GOLD["DUMMY_BIG"], H, "LWL")
    assert sum(x >= (1 << 62) for c in cols for row in c for x in row) > 1000       # the next pairing of such a colour wraps
    below = 0
    for c in cols:
        for h in range(1, H + 1):
            old = set(x for row in c[:h] for x in row)
            below += any(x not in old and x < max(old) for x in c[h])
    assert below > 0                                                          # the ordering quirk is exercised at k = 2


@pytest.fixture
def host_fold(monkeypatch):
    """dn_wl_fold_u64 restated over host arrays, so that the composed path runs on CPU tensors."""
    from dummynode4graphlearning_amd import ops
    real = ops.lib()

    class Lib:
        def __getattr__(self, name):                                          # (the limit getters)
            return getattr(real, name)

        def dn_wl_fold_u64(self, N, n, nodes, seg_ptr, entries, cin, cout, stream):
            assert nodes is None and N == n
            sp = (ctypes.c_int64 * (n + 1)).from_address(seg_ptr.value)
            ent = (ctypes.c_uint64 * max(sp[n], 1)).from_address(entries.value)
            a, b = (ctypes.c_uint64 * n).from_address(cin.value), (ctypes.c_uint64 * n).from_address(cout.value)
            for s in range(n):
                c = a[s]
                for i in range(sp[s], sp[s + 1]):
                    c = wl_ref.pairing(c, ent[i])
                b[s] = c
            return 0

    fake = Lib()
    monkeypatch.setattr(ops, "lib", lambda: fake)
    monkeypatch.setattr(ops, "require_gpu", lambda *t: None)
    monkeypatch.setattr(ops, "stream_ptr", lambda: None)
    return ops


@pytest.mark.parametrize("kernel", C.KERNELS)
@pytest.mark.parametrize("name", ["TOYA", "NCI1", "REDDIT-BINARY", "QUIRKS", "TWOS", "KWL_SMALL"])
def test_composed_path_on_cpu_tensors(host_fold, name, kernel):
    m = _m()
    ds = C.small_bounds() if name == "KWL_SMALL" else GOLD[name]
    fl = C.flags(name)
    d = _cpu(ds)
    _, cols = C.ref(ds, H, kernel, *fl)
    for ws in (m.KWL_WORKSPACE_KEYS, 50):
        with host_fold.kwl_fused(False):
            c, tp = m.kwl_colors(d, H, kernel, *fl, workspace_keys=ws)
        assert tp.tolist()[-1] == c.shape[1] and c.dtype == torch.int64
        for h in range(H + 1):
            assert [x & M64 for x in c[h].tolist()] == C.flat(cols, h), (name, kernel, ws, h)


def test_the_kernels_refuse_cpu_tensors():
    from dummynode4graphlearning_amd import _lib, ops
    m = _m()
    for on in (True, False):
        with ops.kwl_fused(on), pytest.raises(_lib.DnHipError, match="need GPU tensors"):
            m.kwl_colors(_cpu(GOLD["TWOS"]), 1, "LWL")


def test_refusals(tmp_path):
    m = _m()
    d = _cpu(GOLD["TOYA"])
    for kernel in ("LWLP", "LWLPC", "WLOA", "SP"):
        with pytest.raises(ValueError, match="not built"):
            m.kwl_colors(d, 1, kernel)
    with pytest.raises(ValueError, match="num_iterations must be >= 0"):
        m.kwl_colors(d, -1, "WL")
    with pytest.raises(ValueError, match="workspace_keys must be positive"):
        m.kwl_colors(d, 1, "WL", workspace_keys=0)
    with pytest.raises(ValueError, match=r"exceeds the gram kernel's \d+ steps"):
        m.kwl_gram_matrices(d, 16, "LWLC")
    # labels wanted without a file: the message names the file
    wl_cases.write_tu(GOLD["NCI1"], str(tmp_path))
    nci = m.GraphKernelData.from_dir(str(tmp_path), "NCI1", device="cpu")
    with pytest.raises(ValueError, match=r"NCI1_edge_labels\.txt: use_edge_labels without"):
        m.kwl_colors(nci, 1, "WL", True, True)
    wl_cases.write_tu(GOLD["REDDIT-BINARY"], str(tmp_path))
    red = m.GraphKernelData.from_dir(str(tmp_path), "REDDIT-BINARY", device="cpu")
    with pytest.raises(ValueError, match=r"REDDIT-BINARY_node_labels\.txt: use_node_labels without"):
        m.kwl_features(red, 1, "LWL", True, False)
    # MAXNUMCOLOR on tuples: 1000 nodes are 10^6 pairs (H = 0 only); 1001 are too many for any H; LWLC counts n + 2 m
    for n, h, ok in ((1000, 0, True), (1000, 1, False), (1001, 0, False)):
        big = dict(name="WIDE%d" % n, graph_indicator=[1] * n + [2], A=[[1, 2], [2, 1]], node_labels=None, edge_labels=None, graph_labels=[0, 1])
        w = _cpu(big)
        for kernel in ("WL", "DWL", "LWL"):
            if ok:
                assert m._check(w, h, kernel, False, False)[1].num_tuples == n * n + 1
            else:
                with pytest.raises(ValueError, match=r"graph 1 has %d tuples, more than 1000000 / \(H \+ 1\) = %d: .*MAXNUMCOLOR" % (n * n, 1000000 // (h + 1))):
                    m.kwl_colors(w, h, kernel, False, False)
        assert m._check(w, 5, "LWLC", False, False)[1].num_tuples == n + 2 + 1
    # T above int32: 2200 graphs of 1000 nodes are 2.2 10^9 pairs
    n, b = 1000, 2200
    huge = dict(name="MANY", graph_indicator=[1 + i // n for i in range(n * b)], A=[[1, 2], [2, 1]], node_labels=None, edge_labels=None,
                graph_labels=[0] * b)
    with pytest.raises(ValueError, match=r"2200000000 tuples, more than 2\^31 - 2"):
        m.kwl_colors(_cpu(huge), 0, "LWL", False, False)


def test_command_line_routing(capsys, monkeypatch):
    m = _m()
    from dummynode4graphlearning_amd import graph_kernels, graph_kernels_spgr
    calls = []
    monkeypatch.setattr(graph_kernels_spgr, "main", lambda argv=None: calls.append(list(argv)) or 0)
    for kernel in ("WL", "WLOA", "SP", "GR"):
        argv = ["--k", "1", "--kernel", kernel, "--n_iters", "3", "--datasets", "NCI1"]
        assert m.main(argv) == 0 and calls[-1] == argv
    assert m.main(["--kernel", "SP"]) == 0 and calls[-1] == ["--kernel", "SP"]      # (--k defaults to 1)
    for argv in (["--k", "2", "--kernel", "LWLP"], ["--k", "2", "--kernel", "LWLPC"], ["--k", "3", "--kernel", "WL"],
                 ["--k", "2", "--kernel", "WLOA"], ["--k", "2", "--kernel", "SP"], ["--k", "0", "--kernel", "WL"]):
        with pytest.raises(SystemExit) as e:
            m.main(argv + ["--datasets", "NCI1"])
        err = capsys.readouterr().err
        assert e.value.code == 2 and "not built" in err and "WL, DWL, LWL or LWLC" in err and "LWLP" in err and "behind the end" in err
    monkeypatch.undo()
    for main in (graph_kernels.main, graph_kernels_spgr.main):                      # the k = 1 command lines keep refusing --k 2
        with pytest.raises(SystemExit) as e:
            main(["--k", "2", "--kernel", "WL", "--datasets", "NCI1"])
        assert e.value.code == 2 and "not built" in capsys.readouterr().err
    assert m.gram_file("/x", "NCI1", "DWL", 2) == "/x/NCI1__DWL2_2.gram"


def test_package_exports_and_switch():
    import dummynode4graphlearning_amd as pkg
    from dummynode4graphlearning_amd import graph_kernels, ops
    m = _m()
    for name in ("kwl_colors", "kwl_features", "kwl_gram_matrices"):
        assert getattr(pkg, name) is getattr(m, name)
    assert pkg.graph_kernels_kwl is m and callable(m.main) and m.KERNELS == ("WL", "DWL", "LWL", "LWLC")
    assert callable(graph_kernels.features_of_colors)
    default = ops.kwl_fused_enabled()
    assert default == ops.KWL_FUSED_DEFAULT
    with ops.kwl_fused(False):
        assert not ops.kwl_fused_enabled()
        with ops.kwl_fused(True):
            assert ops.kwl_fused_enabled()
            with ops.kwl_fused(False):
                assert not ops.kwl_fused_enabled()
            assert ops.kwl_fused_enabled()
        assert not ops.kwl_fused_enabled()
    assert ops.kwl_fused_enabled() == default
