"""Golden vectors of the HGP-SL pooling layer: the reference's own models/hgpsl.py (and the sparse_softmax.py it imports), imported
UNMODIFIED by file path, run on the CPU under the stand-ins of _ref_standins_sparse.py (torch_geometric / torch_scatter / torch_sparse
names; parity with the real libraries unpinned, see there).  The reference hard-codes dtype=torch.float for its dense [N', N']
matrix and fails in float64, so its run is float32.

Run on the authoring box only (needs the reference checkout; DN_REFERENCE overrides its place):
    python tests/golden/make_golden_gc_hgpsl.py
Writes gc_hgpsl.npz (data only).

Per case <tag>: the batch (x, edge_index, edge_attr where the case has weights, batch, ptr), init/<key> = the parameters at
construction, out/x, out/edge_index, out/edge_attr, out/batch, perm (level by level for the stack), the seeded coefficients cx / ce of
the linear functional L = <cx, out/x> + <ce, out/edge_attr>, and grad/<input or parameter> of L.

Asserted here for every case, trying seeds until all three hold, with the float64 restatement of tests/hgpsl_ref.py:
  * every two adjacent sorted scores of a graph differ by more than 1e-3 of the larger;
  * every sparsemax support decision rho z_(rho) - (cumsum_rho - 1) is more than 1e-3 away from 0;
  * the float32 run's perm and edge list equal the float64 restatement's."""
import importlib.machinery
import importlib.util
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import _ref_standins_sparse as SS  # noqa: E402
import hgpsl_ref as R  # noqa: E402

REF = os.environ.get("DN_REFERENCE", "/root/reference")
MARGIN = 1e-3


def _reference():
    SS.install()
    base = os.path.join(REF, "graph_classification", "graph_neural_networks", "models")
    pkg = importlib.util.module_from_spec(importlib.machinery.ModuleSpec("ref_hgpsl_pkg", None, is_package=True))
    pkg.__path__ = [base]
    sys.modules["ref_hgpsl_pkg"] = pkg
    for name in ("sparse_softmax", "hgpsl"):
        spec = importlib.util.spec_from_file_location("ref_hgpsl_pkg." + name, os.path.join(base, name + ".py"))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[spec.name] = mod
        spec.loader.exec_module(mod)
    return sys.modules["ref_hgpsl_pkg.hgpsl"]


def _graph(rng, n, m, loops=0, isolated=None):
    """m distinct directed edges (no self loops) and `loops` distinct self loops on n nodes; node `isolated` touches nothing."""
    live = [v for v in range(n) if v != isolated]
    pairs = [(a, b) for a in live for b in live if a != b]
    pick = rng.choice(len(pairs), size=min(m, len(pairs)), replace=False) if pairs else []
    e = [pairs[int(i)] for i in pick]
    for v in rng.choice(live, size=min(loops, len(live)), replace=False) if loops else []:
        e.append((int(v), int(v)))
    return e


def _collate(graphs, H, rng, weights):
    ei, ptr = [], [0]
    for n, edges in graphs:
        ei += [(a + ptr[-1], b + ptr[-1]) for a, b in edges]
        ptr.append(ptr[-1] + n)
    order = rng.permutation(len(ei))                                  # (the edge order is the caller's: not sorted by graph)
    ei = np.asarray([ei[int(i)] for i in order], dtype=np.int64).reshape(-1, 2).T
    x = torch.from_numpy(rng.standard_normal((ptr[-1], H)).astype(np.float32))
    w = torch.from_numpy(rng.uniform(0.2, 2.0, size=ei.shape[1]).astype(np.float32)) if weights else None
    batch = torch.tensor([g for g, (n, _) in enumerate(graphs) for _ in range(n)], dtype=torch.long)
    return x, torch.from_numpy(np.ascontiguousarray(ei)), w, batch, ptr


def _batch_a(rng):
    # sizes 5 / 1 / 9 / 12: a one-node graph without edges, an isolated node (node 4 of the third graph), self loops
    return [(5, _graph(rng, 5, 8, loops=1)), (1, []), (9, _graph(rng, 9, 20, loops=2, isolated=4)), (12, _graph(rng, 12, 30))]


def _batch_b(rng):
    return [(n, _graph(rng, n, 2 * n, loops=1)) for n in (7, 12, 4, 10)]


def _batch_c(rng):
    return [(50, _graph(rng, 50, 120, loops=2)), (8, _graph(rng, 8, 14))]


def _batch_tu(rng):
    # dummy-augmented, TU-shaped: undirected real edges both ways, the dummy node LAST and joined both ways to every real node
    out = []
    for n in (8, 6, 11, 8):
        und = [(a, b) for a in range(n - 1) for b in range(a + 1, n - 1)]
        e = []
        for i in rng.choice(len(und), size=min(len(und), n + 2), replace=False):
            a, b = und[int(i)]
            e += [(a, b), (b, a)]
        e += [(n - 1, v) for v in range(n - 1)] + [(v, n - 1) for v in range(n - 1)]
        out.append((n, e))
    return out


CASES = [  # tag, batch, H, ratio, sparse, weights, lamb
    ("soft_w", _batch_a, 6, 0.8, False, True, 1.0),
    ("soft_n", _batch_a, 6, 0.8, False, False, 1.0),
    ("sparse_w", _batch_a, 6, 0.8, True, True, 1.0),
    ("sparse_n", _batch_a, 6, 0.8, True, False, 1.0),
    ("lamb", _batch_a, 6, 0.8, True, True, 0.5),
    ("ratio05", _batch_b, 5, 0.5, True, True, 1.0),
    ("ratio03", _batch_c, 4, 0.3, False, True, 1.0),
    ("tu", _batch_tu, 6, 0.8, True, False, 1.0),
]
STACK = dict(tag="stack", F=5, H=6, ratios=(0.8, 0.5), sparse=True, lamb=1.0)


def _same_edges(a, b):
    return a.shape == b.shape and bool((a == b).all())


def _functional(rng, xo, eo):
    cx = torch.from_numpy(rng.standard_normal(tuple(xo.shape)).astype(np.float32))
    ce = torch.from_numpy(rng.standard_normal(tuple(eo.shape)).astype(np.float32))
    return cx, ce


def _run_case(ref, tag, make_batch, H, ratio, sparse, weights, lamb, seed):
    rng = np.random.default_rng(seed)
    x, ei, w, batch, ptr = _collate(make_batch(rng), H, rng, weights)
    torch.manual_seed(seed)
    layer = ref.HGPSLPool(H, ratio=ratio, sparse=sparse, lamb=lamb)
    att0 = layer.att.detach().clone()
    x.requires_grad_(True)
    if w is not None:
        w.requires_grad_(True)
    SS.TOPK_PERMS.clear()
    xo, eio, eo, bo = layer(x, ei, w, batch)
    perm = SS.TOPK_PERMS[-1]
    cx, ce = _functional(rng, xo, eo)
    ((cx * xo).sum() + (ce * eo).sum()).backward()
    # the float64 restatement and the three margins
    got = R.pool(x.detach().double(), ei, None if w is None else w.detach().double(), ptr, att0.double(), ratio, sparse, lamb, 0.2)
    if not (got["score_gap"] > MARGIN and got["support_margin"] > MARGIN):
        return None
    if not (_same_edges(perm, got["perm"]) and _same_edges(eio, got["edge_index"]) and _same_edges(bo, got["batch"])):
        return None
    assert float((xo.detach().double() - got["x"]).abs().max()) == 0.0
    assert float((eo.detach().double() - got["edge_attr"]).abs().max()) < 1e-5
    out = {"x": x.detach().numpy(), "edge_index": ei.numpy(), "batch": batch.numpy(), "ptr": np.asarray(ptr, dtype=np.int64),
           "init/att": att0.numpy(), "out/x": xo.detach().numpy(), "out/edge_index": eio.numpy(), "out/edge_attr": eo.detach().numpy(),
           "out/batch": bo.numpy(), "perm": perm.numpy(), "cx": cx.numpy(), "ce": ce.numpy(), "grad/x": x.grad.numpy(),
           "grad/att": layer.att.grad.numpy()}
    if w is not None:
        out["edge_attr"], out["grad/edge_attr"] = w.detach().numpy(), w.grad.numpy()
    meta = dict(tag=tag, H=H, ratio=ratio, sparse=sparse, weights=weights, lamb=lamb, negative_slop=0.2, seed=seed,
                pairs=int(sum(k * k for k in np.diff(got["ptr"]))), survivors=int(eio.shape[1]))
    return meta, out


def _run_stack(ref, seed):
    cfg = STACK
    rng = np.random.default_rng(seed)
    x, ei, _, batch, ptr = _collate(_batch_b(rng), cfg["F"], rng, False)
    torch.manual_seed(seed)
    conv1, pool1 = ref.GCN(cfg["F"], cfg["H"]), ref.HGPSLPool(cfg["H"], ratio=cfg["ratios"][0], sparse=cfg["sparse"], lamb=cfg["lamb"])
    conv2, pool2 = ref.GCN(cfg["H"], cfg["H"]), ref.HGPSLPool(cfg["H"], ratio=cfg["ratios"][1], sparse=cfg["sparse"], lamb=cfg["lamb"])
    mods = dict(conv1=conv1, pool1=pool1, conv2=conv2, pool2=pool2)
    init = {m + "." + k: v.detach().clone() for m, mod in mods.items() for k, v in mod.named_parameters()}
    x.requires_grad_(True)
    SS.TOPK_PERMS.clear()
    h = F.relu(conv1(x, ei, None))
    h1, ei1, ea1, b1 = pool1(h, ei, None, batch)
    h = F.relu(conv2(h1, ei1, ea1))
    h2, ei2, ea2, b2 = pool2(h, ei1, ea1, b1)
    perm1, perm2 = SS.TOPK_PERMS[0], SS.TOPK_PERMS[1]
    cx, ce = _functional(rng, h2, ea2)
    ((cx * h2).sum() + (ce * ea2).sum()).backward()
    d = {k: v.double() for k, v in init.items()}
    g = F.relu(R.gcn(x.detach().double(), ei, None, d["conv1.weight"], d["conv1.bias"]))
    r1 = R.pool(g, ei, None, ptr, d["pool1.att"], cfg["ratios"][0], cfg["sparse"], cfg["lamb"], 0.2)
    g = F.relu(R.gcn(r1["x"], r1["edge_index"], r1["edge_attr"], d["conv2.weight"], d["conv2.bias"]))
    r2 = R.pool(g, r1["edge_index"], r1["edge_attr"], r1["ptr"], d["pool2.att"], cfg["ratios"][1], cfg["sparse"], cfg["lamb"], 0.2)
    for r in (r1, r2):
        if not (r["score_gap"] > MARGIN and r["support_margin"] > MARGIN):
            return None
    if not (_same_edges(perm1, r1["perm"]) and _same_edges(ei1, r1["edge_index"]) and _same_edges(perm2, r2["perm"])
            and _same_edges(ei2, r2["edge_index"]) and _same_edges(b2, r2["batch"])):
        return None
    assert float((h2.detach().double() - r2["x"]).abs().max()) < 1e-5 and float((ea2.detach().double() - r2["edge_attr"]).abs().max()) < 1e-5
    out = {"x": x.detach().numpy(), "edge_index": ei.numpy(), "batch": batch.numpy(), "ptr": np.asarray(ptr, dtype=np.int64),
           "out/x": h2.detach().numpy(), "out/edge_index": ei2.numpy(), "out/edge_attr": ea2.detach().numpy(), "out/batch": b2.numpy(),
           "mid/edge_index": ei1.numpy(), "mid/edge_attr": ea1.detach().numpy(), "perm1": perm1.numpy(), "perm2": perm2.numpy(),
           "cx": cx.numpy(), "ce": ce.numpy(), "grad/x": x.grad.numpy()}
    for k, v in init.items():
        out["init/" + k] = v.numpy()
    for m, mod in mods.items():
        for k, p in mod.named_parameters():
            out["grad/%s.%s" % (m, k)] = p.grad.numpy()
    meta = dict(cfg, ratios=list(cfg["ratios"]), negative_slop=0.2, seed=seed, survivors=int(ei2.shape[1]))
    return meta, out


def make():
    ref = _reference()
    store, metas = {}, []
    runs = [(c[0], lambda seed, c=c: _run_case(ref, *c, seed)) for c in CASES] + [(STACK["tag"], lambda seed: _run_stack(ref, seed))]
    for tag, run in runs:
        got = None
        for seed in range(100, 1100):
            got = run(seed)
            if got is not None:
                break
        assert got is not None, "no seed of case %s keeps the margins" % tag
        meta, out = got
        metas.append(meta)
        for k, v in out.items():
            store[tag + "/" + k] = v
        print("case %s: seed %d, %s survivors" % (tag, meta["seed"], meta["survivors"]), meta.get("pairs", ""))
    store["meta"] = np.frombuffer(json.dumps(metas).encode(), dtype=np.uint8)
    path = os.path.join(HERE, "gc_hgpsl.npz")
    np.savez_compressed(path, **store)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    make()
