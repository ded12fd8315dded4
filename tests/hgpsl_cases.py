"""What the HGP-SL host and GPU tests share: the goldens of gc_hgpsl.npz, the bounds, and one run of the package's layer or stack
against a golden case (a helper)."""
import functools
import json
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gc_hgpsl.npz")
RTOL = 1e-4            # outputs: max|a - b| / max|b|
GTOL = 5e-4            # gradients, of their range
TINY = 1e-5            # a gradient expected below this stays below it


def rel_max(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    if b.numel() == 0:
        return 0.0 if a.numel() == 0 else float("inf")
    return float((a - b).abs().max() / b.abs().max().clamp(min=1e-12))


def check_grad(got, want, what):
    want = torch.as_tensor(want)
    if want.numel() == 0 or float(want.abs().max()) < TINY:
        assert got is None or got.numel() == 0 or float(got.abs().max()) < TINY, what
        return 0.0
    err = rel_max(got, want)
    assert err < GTOL, (what, err)
    return err


@functools.lru_cache(maxsize=1)
def golden():
    z = np.load(GOLDEN)
    metas = {m["tag"]: m for m in json.loads(bytes(z["meta"]).decode())}
    return z, metas


def layer_tags():
    return [t for t in golden()[1] if t != "stack"]


def run_layer(tag, device, dtype=torch.float32):
    """The package's HGPSLPool on golden case `tag`: perm and the edge list equal, values and gradients within the bounds."""
    from dummynode4graphlearning_amd import ops
    from dummynode4graphlearning_amd.graph_classification import HGPSLPool
    z, metas = golden()
    m = metas[tag]
    t = lambda k: torch.from_numpy(z[tag + "/" + k])                                # noqa: E731
    x = t("x").to(device=device, dtype=dtype).requires_grad_(True)
    ei, batch = t("edge_index").to(device), t("batch").to(device)
    w = t("edge_attr").to(device=device, dtype=dtype).requires_grad_(True) if m["weights"] else None
    layer = HGPSLPool(m["H"], ratio=m["ratio"], sparse=m["sparse"], lamb=m["lamb"], negative_slop=m["negative_slop"]).to(device=device, dtype=dtype)
    with torch.no_grad():
        layer.att.copy_(t("init/att"))
    index = ops.HgpslIndex(ei[0], ei[1], t("ptr").to(device), x.shape[0])
    xo, eio, eo, bo, nxt = layer(x, ei, w, batch, index=index, return_index=True)
    sel = ops.hgpsl_topk(ops.hgpsl_score(x, index, w), index, index.pooled(m["ratio"]))
    assert torch.equal(sel.perm.cpu(), t("perm"))
    assert torch.equal(eio.cpu(), t("out/edge_index")) and torch.equal(bo.cpu(), t("out/batch"))
    assert nxt.sizes == np.diff(np.asarray(index.pooled(m["ratio"]).ptr_host)).tolist() and nxt.num_edges == eio.shape[1]
    errs = {"x": rel_max(xo, t("out/x")), "edge_attr": rel_max(eo, t("out/edge_attr"))}
    assert max(errs.values()) < RTOL, (tag, errs)
    ((t("cx").to(device=device, dtype=dtype) * xo).sum() + (t("ce").to(device=device, dtype=dtype) * eo).sum()).backward()
    errs["grad x"] = check_grad(x.grad, t("grad/x"), (tag, "x"))
    errs["grad att"] = check_grad(layer.att.grad, t("grad/att"), (tag, "att"))
    if w is not None:
        errs["grad edge_attr"] = check_grad(w.grad, t("grad/edge_attr"), (tag, "edge_attr"))
    return errs


def run_stack(device, dtype=torch.float32):
    """GCN -> pool -> GCN -> pool of the package against the golden stack; the second level's index comes from the first layer."""
    from dummynode4graphlearning_amd import ops
    from dummynode4graphlearning_amd.graph_classification import HGPSLPool, hgpsl
    z, metas = golden()
    m, tag = metas["stack"], "stack"
    t = lambda k: torch.from_numpy(z[tag + "/" + k])                                # noqa: E731
    x = t("x").to(device=device, dtype=dtype).requires_grad_(True)
    ei, batch = t("edge_index").to(device), t("batch").to(device)
    mods = dict(conv1=hgpsl.GCN(m["F"], m["H"]), pool1=HGPSLPool(m["H"], ratio=m["ratios"][0], sparse=m["sparse"], lamb=m["lamb"]),
                conv2=hgpsl.GCN(m["H"], m["H"]), pool2=HGPSLPool(m["H"], ratio=m["ratios"][1], sparse=m["sparse"], lamb=m["lamb"]))
    for name, mod in mods.items():
        mod.to(device=device, dtype=dtype)
        with torch.no_grad():
            for k, p in mod.named_parameters():
                p.copy_(t("init/%s.%s" % (name, k)))
    index = ops.HgpslIndex(ei[0], ei[1], t("ptr").to(device), x.shape[0])
    h = torch.relu(mods["conv1"](x, ei, None))
    h1, ei1, ea1, b1, index1 = mods["pool1"](h, ei, None, batch, index=index, return_index=True)
    assert torch.equal(ei1.cpu(), t("mid/edge_index"))
    h = torch.relu(mods["conv2"](h1, ei1, ea1))
    h2, ei2, ea2, b2 = mods["pool2"](h, ei1, ea1, b1, index=index1)
    assert torch.equal(ei2.cpu(), t("out/edge_index")) and torch.equal(b2.cpu(), t("out/batch"))
    errs = {"mid edge_attr": rel_max(ea1, t("mid/edge_attr")), "x": rel_max(h2, t("out/x")), "edge_attr": rel_max(ea2, t("out/edge_attr"))}
    assert max(errs.values()) < RTOL, errs
    ((t("cx").to(device=device, dtype=dtype) * h2).sum() + (t("ce").to(device=device, dtype=dtype) * ea2).sum()).backward()
    errs["grad x"] = check_grad(x.grad, t("grad/x"), "x")
    for name, mod in mods.items():
        for k, p in mod.named_parameters():
            errs["grad %s.%s" % (name, k)] = check_grad(p.grad, t("grad/%s.%s" % (name, k)), (name, k))
    return errs


# ---------------------------------------------------------------------------------------------- the structure batch of the GPU test
STRUCT_SIZES = [1, 78, 0, 80, 81, 1280, 1281]          # ratio 0.8: k = 1, 63, 0, 64, 65, 1024, 1025
STRUCT_SCALE = [1.0, 1.0, 1.0, 1.0, 1.0, 6.0, 6.0]      # the factor on the rows of each graph
STRUCT_SEED0 = {6: 1000, 128: 2000}                      # where the seed search for the sparsemax margin starts, per H

# The batches of the structure test: graph sizes, row factors, the first seed per H, and what the batch must come to at ratio 0.8
# (kept sizes, the graphs of the composed fallback, the largest key count of each kernel class).  The block class sorts every row of
# a launch at n2 = the launch's largest key count rounded up to a power of two (at least 128): "classes" meets n2 = 1024 with rows of
# 65, 1024 keys, "mid-512" n2 = 512 with rows of 129 and of 257 keys, "mid-256" n2 = 256.
STRUCT_BATCHES = {
    "classes": dict(sizes=STRUCT_SIZES, scale=STRUCT_SCALE, seed0=STRUCT_SEED0, ks=[1, 63, 0, 64, 65, 1024, 1025], big=[6], max_wave=64,
                    max_block=1024),
    "mid-512": dict(sizes=[161, 321], scale=[3.0, 3.0], seed0={6: 3000, 128: 3000}, ks=[129, 257], big=[], max_wave=0, max_block=257),
    "mid-256": dict(sizes=[161], scale=[3.0], seed0={6: 3000, 128: 3000}, ks=[129], big=[], max_wave=0, max_block=129),
}


def structure_batch(H, seed, sizes=STRUCT_SIZES, scale=STRUCT_SCALE):
    """x [N, H], edge_index (unique pairs, about 3 per node, some self loops, shuffled), weights [E], ptr, att [1, 2 H], distinct
    integer scores (exact in any precision, so every path selects the same nodes) -- all float32 on the CPU.  The rows of the large
    graphs are scaled up: their logits spread, which is what lets EVERY one of a thousand rows keep the 1e-3 support margin."""
    rng = np.random.default_rng(seed)
    ptr = [0] + np.cumsum(sizes).tolist()
    N = ptr[-1]
    pairs = set()
    for g, n in enumerate(sizes):
        for _ in range(3 * n):
            a, b = rng.integers(n, size=2)
            pairs.add((ptr[g] + int(a), ptr[g] + int(b)))
    pairs = sorted(pairs)
    ei = np.asarray([pairs[int(i)] for i in rng.permutation(len(pairs))], dtype=np.int64).T
    x = rng.standard_normal((N, H)).astype(np.float32)
    for g, factor in enumerate(scale):
        if factor != 1.0:
            x[ptr[g]:ptr[g + 1]] *= factor
    w = rng.uniform(0.2, 2.0, size=ei.shape[1]).astype(np.float32)
    att = (rng.standard_normal((1, 2 * H)) / np.sqrt(H)).astype(np.float32)
    score = rng.permutation(N).astype(np.float32)
    return dict(x=torch.from_numpy(x), edge_index=torch.from_numpy(np.ascontiguousarray(ei)), w=torch.from_numpy(w), ptr=ptr,
                att=torch.from_numpy(att), score=torch.from_numpy(score))


def structure_reference(b, sparse, weights, lamb=0.5, slope=0.2, ratio=0.8):
    """The float64 restatement on the batch: (perm, pooled boundaries, result dict of hgpsl_ref.structure, the float64 leaves)."""
    import hgpsl_ref as R
    perm, pptr, _ = R.select(b["score"].double(), b["ptr"], ratio)
    xp = b["x"].double()[perm].requires_grad_(True)
    att = b["att"].double().requires_grad_(True)
    w = b["w"].double().requires_grad_(True) if weights else None
    res = R.structure(xp, perm, pptr, b["x"].shape[0], b["edge_index"], w, att, sparse, lamb, slope)
    return perm, pptr, res, (xp, att, w)
