"""Restatement of the LRP ego-net permutation index (subgraph_isomorphism/dataset.py:1750-1886) in NumPy and of the pooling op
(models/lrp.py:65-75) in float64, and the loader of the goldens (tests/golden/si_lrp.npz, made by
tests/golden/make_golden_si_lrp.py from the reference's own LRPDataset / LRPLayer / LRP).

Enumeration, per graph of a batch with graph-local ids (only edges with is_reversed == 0 count):
  adj(v)   sorted, duplicate-free out-neighbours of v;  eid(u, w) = the LAST such edge in edge-id order;  m = min(L - 1, |adj(v)|)
  no node of the graph is a dummy, or v is not one and has no dummy neighbour:   (v,) + p,  p over the m-permutations of adj(v)
  v is a dummy node:                                   (v,) + c,  c over the m-combinations of adj(v) (the reference's "reversed"
                                                       second half walks an exhausted iterator and adds nothing)
  v is not a dummy and has dummy neighbours:           (v,) + q + (d,) for every dummy neighbour d in adj order, q over the
                                                       min(L - 2, n')-permutations of the n' non-dummy neighbours
A sequence of length l fills slot k (L + 1) of its L x L block with node perm[k] and slot a L + b with eid(perm[a], perm[b])
where that edge exists (a != b, a, b < l).  tests/test_lrp_host.py pins all of it against the goldens."""
import itertools
import json
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "si_lrp.npz")
LEAKY_SLOPE = 1.0 / 5.5


# ------------------------------------------------------------------------------------------------ goldens
def load_golden():
    """{case name: meta dict with "arrays" = {name: np.ndarray}} (the packing of make_golden_si_dual_models._pack)."""
    cases = {}
    z = np.load(GOLDEN)
    for m in json.loads(bytes(z["meta"]).decode()):
        arrays = {}
        for name, kind, off, shape in m["index"]:
            blob = z["%s/%s" % (m["tag"], kind)]
            n = int(np.prod(shape)) if shape else 1
            a = blob[off:off + n].reshape(shape)
            arrays[name] = a.astype(bool) if kind == "u8" else a
        m["arrays"] = arrays
        cases[m["name"]] = m
    return cases


def batch(case, side):
    a = case["arrays"]
    d = {k: a["%s/%s" % (side, k)] for k in ("sizes", "esizes", "u", "v", "id", "label", "elabel")}
    for k in ("dummy", "edummy", "rev"):
        d[k] = a.get("%s/%s" % (side, k))
    return d


def golden_lists(case, side):
    a = case["arrays"]
    return tuple(a["%s/lrp_%s" % (side, k)] for k in ("node_row", "node_col", "edge_row", "edge_col", "split"))


def state_dict(case, prefix="param"):
    a = case["arrays"]
    return {k: torch.from_numpy(np.array(a["%s/%s" % (prefix, case["alias"].get(k, k))])) for k in case["keys"]}


def make_graph(d, dev):
    from dummynode4graphlearning_amd import BatchedGraph
    t = lambda x: torch.as_tensor(np.asarray(x)).to(dev)                        # noqa: E731
    nd = {"id": t(d["id"]), "label": t(d["label"])}
    ed = {"label": t(d["elabel"])}
    if d.get("dummy") is not None:
        nd["is_dummy"] = t(d["dummy"])
    if d.get("edummy") is not None:
        ed["is_dummy"] = t(d["edummy"])
    if d.get("rev") is not None:
        ed["is_reversed"] = t(d["rev"])
    return BatchedGraph(t(d["u"]), t(d["v"]), int(np.sum(d["sizes"])), batch_num_nodes=torch.as_tensor(np.asarray(d["sizes"])),
                        batch_num_edges=torch.as_tensor(np.asarray(d["esizes"])), ndata=nd, edata=ed)


def rel_max(got, want):
    got = torch.as_tensor(np.asarray(got.detach().cpu()) if isinstance(got, torch.Tensor) else got).double()
    want = torch.as_tensor(np.asarray(want.detach().cpu()) if isinstance(want, torch.Tensor) else want).double()
    return float((got - want).abs().max() / want.abs().max().clamp(min=1e-30)) if want.numel() else 0.0


# ------------------------------------------------------------------------------------------------ enumeration
def node_sequences(adj, v, dummies, L):
    """The sequences of node v (tuples of graph-local ids), in the reference's order."""
    nb = adj[v]
    m = min(L - 1, len(nb))
    if not dummies:
        return [(v,) + p for p in itertools.permutations(nb, m)]
    if v in dummies:
        return [(v,) + c for c in itertools.combinations(nb, m)]
    dn = [n for n in nb if n in dummies]
    rest = [n for n in nb if n not in dummies]
    if not dn:
        return [(v,) + p for p in itertools.permutations(nb, m)]
    return [(v,) + q + (d,) for d in dn for q in itertools.permutations(rest, min(L - 2, len(rest)))]


def perm_index(d, L):
    """(perm_ptr [N + 1], perm_nodes [P, L], perm_edges [P, L * L]) of a batch dict (sizes, esizes, u, v, rev, dummy), global ids,
    -1 = empty; raises ValueError on a self-loop among the counted edges."""
    sizes, esizes = np.asarray(d["sizes"], np.int64), np.asarray(d["esizes"], np.int64)
    u, v = np.asarray(d["u"], np.int64), np.asarray(d["v"], np.int64)
    rev = np.zeros(len(u), bool) if d.get("rev") is None else np.asarray(d["rev"], bool)
    dummy = np.zeros(int(sizes.sum()), bool) if d.get("dummy") is None else np.asarray(d["dummy"], bool)
    ptr, nodes, edges = [0], [], []
    n0 = e0 = 0
    for gi, (n, ne) in enumerate(zip(sizes, esizes)):
        eid, adj = {}, [set() for _ in range(n)]
        for e in range(e0, e0 + ne):
            if rev[e]:
                continue
            a, b = int(u[e] - n0), int(v[e] - n0)
            if a == b:
                raise ValueError("self-loop on node %d of graph %d" % (a, gi))
            eid[(a, b)] = e
            adj[a].add(b)
        adj = [tuple(sorted(s)) for s in adj]
        dummies = set(int(i) for i in np.nonzero(dummy[n0:n0 + n])[0])
        for x in range(n):
            seqs = node_sequences(adj, x, dummies, L)
            for s in seqs:
                row_n, row_e = [-1] * L, [-1] * (L * L)
                for k, node in enumerate(s):
                    row_n[k] = node + n0
                    for k2, other in enumerate(s):
                        if k2 != k and (node, other) in eid:
                            row_e[k * L + k2] = eid[(node, other)]
                nodes.append(row_n)
                edges.append(row_e)
            ptr.append(ptr[-1] + len(seqs))
        n0 += n
        e0 += ne
    return (np.asarray(ptr, np.int64), np.asarray(nodes, np.int64).reshape(-1, L), np.asarray(edges, np.int64).reshape(-1, L * L))


def index_lists(perm_nodes, perm_edges):
    """The reference's two COO lists (node_to_perm row / col, edge_to_perm row / col) from the materialised index."""
    P, L = perm_nodes.shape
    k = np.arange(L, dtype=np.int64) * (L + 1)
    rows_n = (np.arange(P, dtype=np.int64)[:, None] * L * L + k[None, :])
    keep = perm_nodes >= 0
    rows_e = (np.arange(P, dtype=np.int64)[:, None] * L * L + np.arange(L * L, dtype=np.int64)[None, :])
    keep_e = perm_edges >= 0
    return rows_n[keep], perm_nodes[keep], rows_e[keep_e], perm_edges[keep_e]


# ------------------------------------------------------------------------------------------------ the op in float64
def act_fn(name):
    if name == "relu":
        return torch.relu
    if name == "leaky_relu":
        return lambda t: torch.nn.functional.leaky_relu(t, LEAKY_SLOPE)
    if name == "none":
        return lambda t: t
    raise ValueError(name)


def lrp_pool(x, ef, weight, bias, factor, index, act="relu", pool="mean"):
    """[N, H] = act(pool_p(act(sum_slots W_slot^T row_slot + bias)) * factor) in the dtype of x (float64 in the tests), written as
    lrp.py:65-75 writes it: the dense [P L^2, in] rows, the einsum with weight [in, hid, L^2], the pooling.  factor None: no
    scale and no second activation.  Differentiable (torch autograd)."""
    perm_ptr, perm_nodes, perm_edges = (torch.as_tensor(np.asarray(t)).long() for t in index)
    P, L = perm_nodes.shape
    rows = torch.zeros(P, L * L, x.shape[1], dtype=x.dtype)
    k = torch.arange(L) * (L + 1)
    xn = x[perm_nodes.clamp(min=0)] * (perm_nodes >= 0).unsqueeze(-1).to(x.dtype)                 # [P, L, in]
    rows = rows.index_add(1, k, xn)
    rows = rows + ef[perm_edges.clamp(min=0)] * (perm_edges >= 0).unsqueeze(-1).to(x.dtype)       # [P, L*L, in]
    z = torch.einsum("dab,bca->dc", rows, weight)
    if bias is not None:
        z = z + bias
    f = act_fn(act)
    z = f(z)
    N = perm_ptr.numel() - 1
    cnt = perm_ptr[1:] - perm_ptr[:-1]
    seg = torch.repeat_interleave(torch.arange(N), cnt)
    out = torch.zeros(N, z.shape[1], dtype=x.dtype).index_add(0, seg, z)
    if pool == "mean":
        out = out / cnt.to(x.dtype).view(-1, 1)
    if factor is not None:
        out = f(out * factor)
    return out, z


def exact_premise(*tensors):
    """Every value is an integer below 2^24 in magnitude (an fp32 sum of such terms is exact whatever its order)."""
    for t in tensors:
        t = t.detach().double()
        assert bool((t == t.round()).all()) and float(t.abs().max()) < 2 ** 24, float(t.abs().max())


# ------------------------------------------------------------------------------------------------ exact-integer test data
def exact_inputs(rng, N, E, H, L, in_dim=None):
    """Small-integer operands of the exact tests: x, edge_feat, bias, factor in {-1, 0, 1}, weight in {-1, 0, 1} on a third of
    its entries, the output gradient in {-1, 0, 1}."""
    in_dim = in_dim or H
    f = lambda *s: torch.from_numpy(rng.integers(-1, 2, size=s).astype(np.float32))     # noqa: E731
    w = f(in_dim, H, L * L) * torch.from_numpy((rng.integers(0, 3, size=(in_dim, H, L * L)) == 0).astype(np.float32))
    return dict(x=f(N, in_dim), ef=f(E, in_dim), weight=w, bias=f(H), factor=f(N, H), g=f(N, H))


def exact_graphs():
    """The batches of the exact tests of tests/test_gpu_lrp.py as (name, batch dict, L, H); see there for what each one holds."""
    from dummynode4graphlearning_amd import ops
    cases = load_golden()
    out = []
    rng = np.random.default_rng(11)
    for L, H in ((3, 16), (4, 16), (3, 64), (4, 64)):
        case = cases["lrp_no_reversed" if L == 4 else "lrp_no_reversed_l3"]      # dummy hubs, dummy neighbours, parallel edges
        out.append(("golden_L%d_H%d" % (L, H), batch(case, "g"), L, H))
    case = cases["lrp_no_dummy"]                                                  # an isolated node, plain permutations
    out.append(("isolated", batch(case, "g"), 4, 16))
    # a hub one past the LDS staging limit (and past the pair-table limit): a star with a few edges among the leaves
    H, L = 64, 3
    d = ops.lrp_stage_nodes(H, L)                                                 # ego nodes that still fit -> d neighbours = one past
    assert d + 1 > ops.LRP_PAIR_NODES
    u = [0] * d + list(range(1, d + 1)) + list(rng.integers(1, d + 1, size=40))
    v = list(range(1, d + 1)) + [0] * d + list(rng.integers(1, d + 1, size=40))
    keep = [i for i in range(len(u)) if u[i] != v[i]]
    u, v = np.array(u)[keep], np.array(v)[keep]
    out.append(("past_stage_limit", dict(sizes=[d + 1], esizes=[len(u)], u=u, v=v, dummy=None, rev=None), L, H))
    # staged, but past the pair-table limit, the hub a dummy (combinations); and exactly at the staging limit
    for name, n, H, L, dummy in (("dummy_hub_no_pair_table", ops.LRP_PAIR_NODES + 6, 16, 3, True),
                                 ("at_stage_limit", ops.lrp_stage_nodes(64, 3) - 1, 64, 3, False)):
        u = [0] * n + list(range(1, n + 1)) + list(rng.integers(1, n + 1, size=30))
        v = list(range(1, n + 1)) + [0] * n + list(rng.integers(1, n + 1, size=30))
        keep = [i for i in range(len(u)) if u[i] != v[i]]
        u, v = np.array(u)[keep], np.array(v)[keep]
        dm = np.zeros(n + 1, bool)
        dm[0] = dummy
        out.append((name, dict(sizes=[n + 1], esizes=[len(u)], u=u, v=v, dummy=dm if dummy else None, rev=None), L, H))
    return out
