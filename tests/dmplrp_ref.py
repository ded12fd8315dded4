"""Restatement of the collapsed ego-net pooling index of DMPLRP (subgraph_isomorphism/models/dmplrp.py:180-185) in NumPy, and the
loader of its goldens (tests/golden/si_dmplrp.npz, made by tests/golden/make_golden_si_dmplrp.py from the reference's own
DMPLRPPoolLayer / DMPLRP).  Builds on tests/lrp_ref.py: the enumeration, the float64 pooling op and the exact-test data are its.

Nothing non-linear stands between the contraction and the pooling of a DMPLRP layer, so the mean over a node's sequences is a
weighted sum of table rows: out[v] = bias + sum_rows (occurrences of the row in v's sequences / P_v) T[row].  Rows are numbered as
ops.LrpIndex.composed_tables numbers them: node u at position k -> u L + k, edge eid in slot (a, b) ->
N L + eid L (L - 1) + a (L - 1) + (b - 1 if b > a else b).

collapsed_by_enumeration counts the rows of the materialised index (lrp_ref.perm_index); collapsed_closed_form is the closed form
the device kernel evaluates (dn_lrp.hip), written the way the kernel walks an ego: the node rows of the ego's d + 1 nodes, then
every counted edge between two ego nodes with the number of sequences that hold its ends at positions (a, b)."""
import json
import os
from math import comb

import numpy as np

import lrp_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "si_dmplrp.npz")


def load_golden():
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


def seq_len(case):
    return case["cfg"]["lrp_seq_len"] if case["kind"] == "model" else case["kw"]["lrp_seq_len"]


def hand_made_graph():
    """One batch of two graphs (graph 0: nodes 0-9, graph 1: nodes 10-13), dummies 8, 9 and 13:
      0        isolated
      1 -> 2                          kind 0 with d = 1 < L - 1
      2 -> {1, 3, 4, 5}, twice -> 3   kind 0 with d = 4, a parallel edge; 3 -> 2 exists, 4 -> 2 only as a reversed edge
      3 -> {2, 4}
      4 -> 8                          kind 2 with n' = 0
      5 -> {6, 8}                     kind 2 with n' = 1
      6 -> {1, 2, 5, 8, 9}            kind 2 with two dummy neighbours, 2 -> ... and 5 -> 6 make pairs among the neighbours
      7 -> {8, 9}                     kind 2, n' = 0, two dummy neighbours
      8 -> {1, 2, 3, 4, 5, 6, 7}      a dummy node, combinations
      9 -> {6, 7}                     a dummy node with d = 2 < L - 1 at L = 4
      10 -> {11, 12, 13}, 11 -> 10, 12 -> {10, 11}, 13 -> {10}   a dummy node with d = 1, a kind-2 node with n' = 2"""
    edges = [(1, 2), (2, 1), (2, 3), (2, 4), (2, 5), (2, 3), (3, 2), (3, 4), (4, 8), (5, 6), (5, 8),
             (6, 1), (6, 2), (6, 5), (6, 8), (6, 9), (7, 8), (7, 9)] + [(8, i) for i in range(1, 8)] + [(9, 6), (9, 7)]
    rev = [False] * len(edges)
    edges.append((4, 2))
    rev.append(True)
    n0 = len(edges)
    edges += [(10, 11), (10, 12), (10, 13), (11, 10), (12, 10), (12, 11), (13, 10)]
    rev += [False] * (len(edges) - n0)
    dummy = np.zeros(14, bool)
    dummy[[8, 9, 13]] = True
    u, v = np.array([e[0] for e in edges]), np.array([e[1] for e in edges])
    return dict(sizes=np.array([10, 4]), esizes=np.array([n0, len(edges) - n0]), u=u, v=v, dummy=dummy, rev=np.array(rev),
                id=np.arange(14) % 10, label=np.ones(14, np.int64), elabel=np.zeros(len(edges), np.int64), edummy=None)


def dummy_star(leaves, extra=30, seed=3):
    """A dummy hub 0 with edges to and from `leaves` leaves and a few edges among the leaves."""
    rng = np.random.default_rng(seed)
    u = [0] * leaves + list(range(1, leaves + 1)) + list(rng.integers(1, leaves + 1, size=extra))
    v = list(range(1, leaves + 1)) + [0] * leaves + list(rng.integers(1, leaves + 1, size=extra))
    keep = [i for i in range(len(u)) if u[i] != v[i]]
    dm = np.zeros(leaves + 1, bool)
    dm[0] = True
    return dict(sizes=[leaves + 1], esizes=[len(keep)], u=np.array(u)[keep], v=np.array(v)[keep], dummy=dm, rev=None)


# ------------------------------------------------------------------------------------------------ the collapsed index
def off_slot(a, b, L):
    return a * (L - 1) + (b - 1 if b > a else b)


def collapsed_by_enumeration(d, L):
    """(col_ptr [N + 1], col_rows [Q], col_cnt [Q]) int64: np.unique per node over the rows of the materialised index."""
    ptr, nodes, edges = R.perm_index(d, L)
    N = len(ptr) - 1
    slot = np.arange(L * L)
    a, b = slot // L, slot % L
    off = a * (L - 1) + np.where(b > a, b - 1, b)
    rows_n = np.where(nodes >= 0, nodes * L + np.arange(L), -1)
    rows_e = np.where(edges >= 0, N * L + edges * (L * (L - 1)) + off, -1)
    rows = np.concatenate([rows_n, rows_e], 1)
    col_ptr, col_rows, col_cnt = [0], [], []
    for v in range(N):
        r = rows[ptr[v]:ptr[v + 1]].reshape(-1)
        uq, cnt = np.unique(r[r >= 0], return_counts=True)
        col_rows.append(uq)
        col_cnt.append(cnt)
        col_ptr.append(col_ptr[-1] + len(uq))
    return np.asarray(col_ptr, np.int64), np.concatenate(col_rows).astype(np.int64), np.concatenate(col_cnt).astype(np.int64)


def _perm(n, k):
    if k < 0 or n < k:
        return 0
    r = 1
    for i in range(k):
        r *= n - i
    return r


def _comb(n, k):
    return comb(n, k) if 0 <= k <= n else 0


class _Ego:
    """The closed-form occurrence counts of one ego: kind, d neighbours of which nd are dummies, sequence length L."""

    def __init__(self, kind, d, nd, L):
        self.kind, self.d, self.nd, self.L = kind, d, nd, L
        self.nn = d - nd
        self.m = min(L - 2, self.nn) if kind == 2 else min(L - 1, d)          # positions 1 .. m hold (non-dummy) neighbours

    def total(self):
        if self.kind == 0:
            return _perm(self.d, self.m)
        if self.kind == 1:
            return _comb(self.d, self.m)
        return self.nd * _perm(self.nn, self.m)

    def node(self, t, z, k):
        """Sequences with the neighbour of sorted position t (t = -1: the ego's own node; z: it is a dummy) at position k."""
        if t < 0:
            return self.total() if k == 0 else 0
        if k < 1:
            return 0
        m = self.m
        if self.kind == 0:
            return _perm(self.d - 1, m - 1) if k <= m else 0
        if self.kind == 1:
            return _comb(t, k - 1) * _comb(self.d - 1 - t, m - k) if k <= m else 0
        if z:
            return _perm(self.nn, m) if k == m + 1 else 0
        return self.nd * _perm(self.nn - 1, m - 1) if k <= m else 0

    def joint(self, ta, za, a, tb, zb, b):
        """Sequences with neighbour ta at position a AND neighbour tb at position b (a != b, ta != tb)."""
        if ta < 0:
            return self.node(tb, zb, b) if a == 0 else 0
        if tb < 0:
            return self.node(ta, za, a) if b == 0 else 0
        if a < 1 or b < 1:
            return 0
        m = self.m
        if self.kind == 0:
            return _perm(self.d - 2, m - 2) if (a <= m and b <= m) else 0
        if self.kind == 1:
            if ta > tb:
                ta, a, tb, b = tb, b, ta, a
            if not (a < b <= m):
                return 0
            return _comb(ta, a - 1) * _comb(tb - ta - 1, b - a - 1) * _comb(self.d - 1 - tb, m - b)
        if za and zb:
            return 0
        if not za and not zb:
            return self.nd * _perm(self.nn - 2, m - 2) if (a <= m and b <= m) else 0
        if za:
            a, b = b, a                                                        # b: the dummy's position
        return _perm(self.nn - 1, m - 1) if (b == m + 1 and a <= m) else 0


def collapsed_closed_form(d, L):
    """The same three arrays from the closed forms, no enumeration: per node the rows ascend."""
    sizes, esizes = np.asarray(d["sizes"], np.int64), np.asarray(d["esizes"], np.int64)
    u, v = np.asarray(d["u"], np.int64), np.asarray(d["v"], np.int64)
    N = int(sizes.sum())
    rev = np.zeros(len(u), bool) if d.get("rev") is None else np.asarray(d["rev"], bool)
    dummy = np.zeros(N, bool) if d.get("dummy") is None else np.asarray(d["dummy"], bool)
    eid = {}
    for e in range(len(u)):
        if not rev[e]:
            eid[(int(u[e]), int(v[e]))] = e
    adj = [[] for _ in range(N)]
    for (a, b) in sorted(eid):
        adj[a].append(b)
    col_ptr, col_rows, col_cnt = [0], [], []
    for x in range(N):
        nb = adj[x]
        nd = sum(1 for w in nb if dummy[w])
        kind = 1 if dummy[x] else (2 if nd else 0)
        ego = _Ego(kind, len(nb), nd, L)
        local = [(x, -1, False)] + [(w, t, bool(dummy[w])) for t, w in enumerate(nb)]
        pos = {n: (t, z) for n, t, z in local}
        ent = {}
        for n, t, z in local:
            for k in range(L):
                c = ego.node(t, z, k)
                if c > 0:
                    ent[n * L + k] = c
        for n, t, z in local:
            for w in adj[n]:
                if w not in pos:
                    continue
                tb, zb = pos[w]
                for a in range(L):
                    for b in range(L):
                        if a == b:
                            continue
                        c = ego.joint(t, z, a, tb, zb, b)
                        if c > 0:
                            ent[N * L + eid[(n, w)] * L * (L - 1) + off_slot(a, b, L)] = c
        rows = sorted(ent)
        col_rows += rows
        col_cnt += [ent[r] for r in rows]
        col_ptr.append(len(col_rows))
    return np.asarray(col_ptr, np.int64), np.asarray(col_rows, np.int64), np.asarray(col_cnt, np.int64)


# ------------------------------------------------------------------------------------------------ the batches of the GPU tests
def index_graphs():
    """(name, batch dict, L) of the index tests: every golden batch at its sequence length, lrp_ref.exact_graphs() (a hub one
    past the LDS staging limit of the fused kernels, one at it, a dummy hub past the pair-table limit), the hand-made graph at
    L = 2, 3, 4 and a dummy hub with 40 leaves at L = 4 (9,880 combinations)."""
    out = []
    cases = load_golden()
    for name in sorted(cases):
        for side in (("p", "g") if cases[name]["kind"] == "model" else ("g",)):
            out.append(("%s_%s" % (name, side), R.batch(cases[name], side), seq_len(cases[name])))
    for name, d, L, H in R.exact_graphs():
        if not (name.startswith("golden") and H != 16):               # the same batch at another width
            out.append((name, d, L))
    out += [("hand_made_L%d" % L, hand_made_graph(), L) for L in (2, 3, 4)]
    out.append(("dummy_hub_40", dummy_star(40), 4))
    return out


def exact_cases():
    """(name, batch dict, L, H, input width) of the exact op tests: lrp_ref.exact_graphs() (H = 16 and 64, L = 3 and 4; the input
    width drops to 16 on the hub cases, where sums over thousands of sequences would leave the exact range of fp32), the
    graph-side golden batches of the model cases, the hand-made graph and the 40-leaf dummy hub."""
    out = []
    for name, d, L, H in R.exact_graphs():
        out.append((name, d, L, H, H if name.startswith(("golden", "isolated")) else 16))
    cases = load_golden()
    for name in sorted(cases):
        if cases[name]["kind"] == "model":
            out.append((name + "_g", R.batch(cases[name], "g"), seq_len(cases[name]), 16, 16))
    out += [("hand_made_L3", hand_made_graph(), 3, 16, 16), ("hand_made_L4", hand_made_graph(), 4, 64, 64),
            ("dummy_hub_40", dummy_star(40), 4, 16, 16)]
    return out


def pool_linear(x, ef, weight, bias, index, pool):
    """dmplrp.py:180-185 in the dtype of x: lrp_ref.lrp_pool without activation and factor."""
    return R.lrp_pool(x, ef, weight, bias, None, index, "none", pool)[0]


# ------------------------------------------------------------------------------------------------ shifts in front of a BatchNorm
def bn_shift(batch_norm, num_mlp_layers, k):
    """Is parameter k of a DMPLRP layer a shift in front of a BatchNorm (nmlp.0.bias / emlp.0.bias, and nbias / ebias, which reach
    the same BatchNorm through the first Linear only)?  Its true gradient is zero -- the norm subtracts the batch mean -- and the
    reference's value is rounding noise (~1e-7 next to weight gradients of ~1), so a bound relative to it says nothing: such a
    gradient is held to |grad| < 1e-4 * the largest weight gradient of its layer, as tests/si_dual_model_ref.bn_shift holds the
    same parameters of DMPNN."""
    return bool(batch_norm) and num_mlp_layers >= 2 and k.endswith(("nmlp.0.bias", "emlp.0.bias", "nbias", "ebias"))


def layer_weight_grad_scale(case, k):
    """Largest golden gradient magnitude over the weights of the layer that holds parameter k."""
    prefix = k[:k.index(").") + 2] if ")." in k else ""
    a = case["arrays"]
    return max(float(np.abs(a["grad/" + n]).max()) for n in case["params"]
               if n.startswith(prefix) and n.endswith("weight") and "grad/" + n in a)
