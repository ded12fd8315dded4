"""Host tests of the 3-WL graph kernels (graph_kernels_k3wl.py): no GPU.

* the plain-Python restatement tests/k3wl_ref.py and the writer reproduce, byte for byte, every file the reference's own binary wrote
  for `--k 3 --kernel WL | DWL | LWL | LWLC --n_iters 2` (tests/golden/graph_kernels_k3wl.json; DUMMY_BIG for LWLC only: its n^3
  kernels would take the restatement minutes -- the GPU tests hold the device against those texts);
* the composed path's torch part on CPU tensors: it runs there except for the one kernel it ends in (dn_wl_fold_u64), which is
  restated here over the same host arrays -- so the entry construction, the segmented sort, the removal of the maxima and the final
  combination are held to the restatement, in one chunk and in chunks of a few entries;
* the plan's offsets and LWLC item lists, refusals, command-line routing, package exports and the switch.
"""
import ctypes

import pytest
import torch

import k3wl_cases as C
import k3wl_ref
import wl_cases
import wl_ref

H, GOLD = C.golden()
M64 = (1 << 64) - 1


def _m():
    from dummynode4graphlearning_amd import graph_kernels_k3wl
    return graph_kernels_k3wl


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


def _named(name):
    return C.small_bounds() if name == "K3WL_SMALL" else GOLD[name]


@pytest.mark.parametrize("kernel", C.KERNELS)
@pytest.mark.parametrize("name", C.SMALL_GOLDENS + ["DUMMY_BIG"])
def test_restatement_reproduces_the_reference_binary(name, kernel):
    ds = GOLD[name]
    assert sorted(k for k in ds["grams"] if k.startswith(kernel + "3_")) == ["%s3_%d" % (kernel, h) for h in range(H + 1)]
    if name == "DUMMY_BIG" and kernel != "LWLC":
        assert all(ds["grams"]["%s3_%d" % (kernel, h)].count("\n") == 24 for h in range(H + 1))
        return                                                                # (585,410 triples: held on the device, not here)
    _, cols = C.ref(ds, H, kernel, *C.flags(name))
    Gs = wl_ref.gram([wl_ref.features(c) for c in cols], H, "WL")
    for h in range(H + 1):
        assert wl_ref.libsvm_text(Gs[h], ds["graph_labels"]) == ds["grams"]["%s3_%d" % (kernel, h)], (name, kernel, h)


def test_the_goldens_cover_what_they_should():
    assert sorted(GOLD) == ["DUMMY_BIG", "NCI1", "QUIRKS", "REDDIT-BINARY", "THREES", "TOYA", "TWOS"] and H == 2
    ds = GOLD["THREES"]
    sizes = [ds["graph_indicator"].count(g) for g in range(1, 6)]
    assert sizes == [1, 3, 4, 11, 6] and max(sizes) <= 12
    graphs = C.graphs_of(ds)
    assert not graphs[1]["nbrs"][0] and not graphs[1]["nbrs"][1] and not graphs[1]["nbrs"][2]       # the edgeless graph
    assert len(graphs[3]["nbrs"][0]) == 10                                                            # the hub
    assert {(1 << 63) - 1, 1 << 63, (1 << 63) + 1, M64 - 1, M64} <= set(ds["node_labels"])
    for kernel in C.KERNELS:
        _, cols = C.ref(ds, H, kernel)
        assert sum(x >= (1 << 62) for c in cols for row in c for x in row) > 100     # the next pairing of such a colour wraps
        below = 0
        for c in cols:
            for h in range(1, H + 1):
                old = set(x for row in c[:h] for x in row)
                below += any(x not in old and x < max(old) for x in c[h])
        assert below > 0                                                      # the ordering quirk is exercised at k = 3


def test_edge_labels_enter_nowhere():
    ds = GOLD["TWOS"]
    for kernel in C.KERNELS:
        assert C.ref(ds, 1, kernel, True, True)[1] == C.ref(ds, 1, kernel, True, False)[1]
    d = _cpu(ds)
    stripped = dict(ds, edge_labels=[7] * len(ds["edge_labels"]), name="TWOS_EL7")
    a, b = _m()._plan(d, "LWLC"), _m()._plan(_cpu(stripped), "LWLC")
    assert torch.equal(a.tup_u, b.tup_u) and torch.equal(a.item_key, b.item_key)


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
@pytest.mark.parametrize("name", C.SMALL_GOLDENS + ["K3WL_SMALL"])
def test_composed_path_on_cpu_tensors(host_fold, name, kernel):
    """The small goldens with their own flags; K3WL_SMALL (1, 2, 8, 9 nodes, an edgeless graph, hubs of degree 7, 8, 9) with labels
    and without; H = 1 keeps the Python fold of the n^4 entries short."""
    m = _m()
    ds = _named(name)
    d = _cpu(ds)
    for fl in ([C.flags(name)] if name != "K3WL_SMALL" else [(True, True), (False, False)]):
        _, cols = C.ref(ds, 1, kernel, *fl)
        for ws in (m.K3WL_WORKSPACE_KEYS, 300):
            with host_fold.k3wl_fused(False):
                c, tp = m.k3wl_colors(d, 1, kernel, *fl, workspace_keys=ws)
            assert tp.tolist()[-1] == c.shape[1] and c.dtype == torch.int64
            for h in range(2):
                assert [x & M64 for x in c[h].tolist()] == C.flat(cols, h), (name, kernel, fl, ws, h)


@pytest.mark.parametrize("name", C.SMALL_GOLDENS + ["K3WL_SMALL", "DUMMY_BIG"])
def test_plan_offsets_and_item_lists(name):
    m = _m()
    ds = _named(name)
    d, graphs = _cpu(ds), C.graphs_of(ds)
    first = d.node_ptr.tolist()
    for kernel in ("LWL", "LWLC"):
        p = m._plan(d, kernel)
        items = [k3wl_ref.triples(G, kernel) for G in graphs]
        ptr = [sum(len(t) for t in items[:g]) for g in range(len(items) + 1)]
        assert p.tuple_ptr.tolist() == ptr and p.num_tuples == ptr[-1]
        want = [(first[g] + i, first[g] + j, first[g] + k) for g, t in enumerate(items) for i, j, k in t]
        assert list(zip(p.tup_v.tolist(), p.tup_w.tolist(), p.tup_u.tolist())) == want
        assert p.tuple_graph.tolist() == [g for g, t in enumerate(items) for _ in t]
    keys, slots = p.item_key.tolist(), p.item_slot.tolist()                  # LWLC: per graph ascending keys and the item behind each
    for g, (G, t) in enumerate(zip(graphs, items)):
        n = G["n"]
        by_key = sorted(((i * n + j) * n + k, ptr[g] + s) for s, (i, j, k) in enumerate(t))
        assert list(zip(keys[ptr[g]:ptr[g + 1]], slots[ptr[g]:ptr[g + 1]])) == by_key


def test_the_kernels_refuse_cpu_tensors():
    from dummynode4graphlearning_amd import _lib, ops
    m = _m()
    for on in (True, False):
        with ops.k3wl_fused(on), pytest.raises(_lib.DnHipError, match="need GPU tensors"):
            m.k3wl_colors(_cpu(GOLD["TWOS"]), 1, "LWL")


def test_refusals(tmp_path):
    m = _m()
    d = _cpu(GOLD["TOYA"])
    for kernel in ("LWLP", "LWLPC", "WLOA", "SP"):
        with pytest.raises(ValueError, match="not built at k = 3.*behind the end"):
            m.k3wl_colors(d, 1, kernel)
    with pytest.raises(ValueError, match="num_iterations must be >= 0"):
        m.k3wl_colors(d, -1, "WL")
    with pytest.raises(ValueError, match="workspace_keys must be positive"):
        m.k3wl_colors(d, 1, "WL", workspace_keys=0)
    with pytest.raises(ValueError, match=r"exceeds the gram kernel's \d+ steps"):
        m.k3wl_gram_matrices(d, 16, "LWLC")
    # labels wanted without a file: the message names the file (what the k = 1 reader refuses is refused by the reader itself)
    wl_cases.write_tu(GOLD["NCI1"], str(tmp_path))
    nci = m.GraphKernelData.from_dir(str(tmp_path), "NCI1", device="cpu")
    with pytest.raises(ValueError, match=r"NCI1_edge_labels\.txt: use_edge_labels without"):
        m.k3wl_colors(nci, 1, "WL", True, True)
    wl_cases.write_tu(GOLD["REDDIT-BINARY"], str(tmp_path))
    red = m.GraphKernelData.from_dir(str(tmp_path), "REDDIT-BINARY", device="cpu")
    with pytest.raises(ValueError, match=r"REDDIT-BINARY_node_labels\.txt: use_node_labels without"):
        m.k3wl_features(red, 1, "LWL", True, False)
    # MAXNUMCOLOR on items, with the reference's `<`: n^3 (H + 1) must stay below 10^6 -- 62 nodes at H = 3, 69 at H = 2, 79 at H = 1
    for n, h, ok in ((62, 3, True), (63, 3, False), (69, 2, True), (70, 2, False), (79, 1, True), (80, 1, False), (99, 0, True), (100, 0, False)):
        big = dict(name="WIDE%d" % n, graph_indicator=[1] * n + [2], A=[[1, 2], [2, 1]], node_labels=None, edge_labels=None, graph_labels=[0, 1])
        w = _cpu(big)
        for kernel in ("WL", "DWL", "LWL"):
            if ok:
                assert m._check(w, h, kernel, False, False)[1].num_tuples == n ** 3 + 1
            else:
                with pytest.raises(ValueError, match=r"graph 1 has %d items, times \(H \+ 1\) = %d that reaches 1000000: .*MAXNUMCOLOR"
                                   % (n ** 3, h + 1)):
                    m.k3wl_colors(w, h, kernel, False, False)
        assert m._check(w, 5, "LWLC", False, False)[1].num_tuples == n + 2 + 1
    # LWLC counts n + 2 m + the two-edge triples: a hub of degree 600 has 601 + 1200 + 3 * 600 * 599 items; one of degree 2000 is
    # refused from a lower bound (a third of its 2000 * 1999 centred pairs) before any item is built
    for deg, said in ((600, "1080001"), (2000, "at least 1338668")):
        star = dict(name="STAR", graph_indicator=[1] * (deg + 1), A=[[1, v] for v in range(2, deg + 2)] + [[v, 1] for v in range(2, deg + 2)],
                    node_labels=None, edge_labels=None, graph_labels=[0])
        with pytest.raises(ValueError, match=r"graph 1 has %s items.*MAXNUMCOLOR" % said):
            m.k3wl_colors(_cpu(star), 0, "LWLC", False, False)
    # T above int32: 2220 graphs of 99 nodes are 2.15 10^9 triples
    n, b = 99, 2220
    huge = dict(name="MANY", graph_indicator=[1 + i // n for i in range(n * b)], A=[[1, 2], [2, 1]], node_labels=None, edge_labels=None,
                graph_labels=[0] * b)
    with pytest.raises(ValueError, match=r"2154063780 items, more than 2\^31 - 2"):
        m.k3wl_colors(_cpu(huge), 0, "LWL", False, False)


def test_command_line_routing(capsys, monkeypatch):
    m = _m()
    from dummynode4graphlearning_amd import graph_kernels, graph_kernels_kwl, graph_kernels_spgr
    calls = []
    monkeypatch.setattr(graph_kernels_kwl, "main", lambda argv=None: calls.append(list(argv)) or 0)
    for k, kernel in (("1", "WL"), ("1", "WLOA"), ("1", "SP"), ("1", "GR"), ("2", "WL"), ("2", "DWL"), ("2", "LWL"), ("2", "LWLC"),
                      ("2", "LWLP")):
        argv = ["--k", k, "--kernel", kernel, "--n_iters", "3", "--datasets", "NCI1"]
        assert m.main(argv) == 0 and calls[-1] == argv
    assert m.main(["--kernel", "SP"]) == 0 and calls[-1] == ["--kernel", "SP"]      # (--k defaults to 1)
    n = len(calls)
    for argv in (["--k", "3", "--kernel", "LWLP"], ["--k", "3", "--kernel", "LWLPC"], ["--k", "4", "--kernel", "WL"],
                 ["--k", "3", "--kernel", "WLOA"], ["--k", "3", "--kernel", "SP"], ["--k", "0", "--kernel", "WL"]):
        with pytest.raises(SystemExit) as e:
            m.main(argv + ["--datasets", "NCI1"])
        err = capsys.readouterr().err
        assert e.value.code == 2 and "not built" in err and "WL, DWL, LWL or LWLC" in err and "LWLP" in err and "behind the end" in err
    assert len(calls) == n
    monkeypatch.undo()
    for main in (graph_kernels.main, graph_kernels_spgr.main, graph_kernels_kwl.main):      # the other command lines keep refusing --k 3
        with pytest.raises(SystemExit) as e:
            main(["--k", "3", "--kernel", "WL", "--datasets", "NCI1"])
        assert e.value.code == 2 and "not built" in capsys.readouterr().err
    assert m.gram_file("/x", "NCI1", "DWL", 2) == "/x/NCI1__DWL3_2.gram"
    assert m.gram_file("g", "TWOS", "LWLC", 0) == "g/TWOS__LWLC3_0.gram"


def test_package_exports_and_switch():
    import dummynode4graphlearning_amd as pkg
    from dummynode4graphlearning_amd import graph_kernels, ops
    m = _m()
    for name in ("k3wl_colors", "k3wl_features", "k3wl_gram_matrices"):
        assert getattr(pkg, name) is getattr(m, name)
    assert pkg.graph_kernels_k3wl is m and callable(m.main) and m.KERNELS == ("WL", "DWL", "LWL", "LWLC")
    assert callable(graph_kernels.features_of_colors)
    assert sorted(ops.K3WL_FUSED_DEFAULT) == sorted(m.KERNELS)
    default = {k: ops.k3wl_fused_enabled(k) for k in m.KERNELS}
    assert default == ops.K3WL_FUSED_DEFAULT and ops.k3wl_fused_enabled() == all(default.values())
    with ops.k3wl_fused(False):
        assert not ops.k3wl_fused_enabled() and not ops.k3wl_fused_enabled("WL")
        with ops.k3wl_fused(True):
            assert ops.k3wl_fused_enabled() and ops.k3wl_fused_enabled("LWLC")
            with ops.k3wl_fused(False):
                assert not ops.k3wl_fused_enabled("DWL")
            assert ops.k3wl_fused_enabled("DWL")
        assert not ops.k3wl_fused_enabled("LWL")
    assert {k: ops.k3wl_fused_enabled(k) for k in m.KERNELS} == default
    with ops.kwl_fused(False):                                               # the k = 2 switch is another one
        assert {k: ops.k3wl_fused_enabled(k) for k in m.KERNELS} == default
