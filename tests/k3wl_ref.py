"""Pure-Python restatement of the reference's 3-WL graph kernels (graph_classification/graph_kernels: `gram --k 3 --kernel WL | DWL |
LWL | LWLC`, i.e. GenerateThree::compute_colors_simple of src/GenerateThree.cpp:477-833 over the tuple graphs of :835, :987, :1229 and
:1376, driven by gram.cpp:252-308).  On the reader, the pairing function, the per-graph colour maps and the matrices of
tests/wl_ref.py; Python ints masked to 64 bits, no numpy, no torch.  tests/test_graph_kernels_k3wl_host.py holds it against the text
the reference's own binary wrote (tests/golden/graph_kernels_k3wl.json); the GPU tests hold the kernels against it.

The tuple graph is never built: its adjacency lists are restated as gathers from the colour cube C[a][b][c] of the previous
iteration.  The tuple graph is undirected and its add_edge pushes both ends, so every neighbour sits in a list TWICE; in WL and DWL all
three exchange loops also reach the triple itself, the edge-type map keeps the first insertion (type 1), and each of the three self
add_edge calls pushes twice: the triple's own colour enters the type-1 multiset SIX times (DWL: the global one, has_edge(v, v) being
false).  LWLC gives the first and the second exchange the same type 2, so it has two multisets.  Edge labels enter nowhere.
"""
import wl_ref
from wl_ref import M64, pairing

KERNELS = ("WL", "DWL", "LWL", "LWLC")


def triples(G, kernel):
    """The items of one graph in the reference's order: all ordered triples, row-major; LWLC: (i, i, i), then (i, i, j) for adjacent
    i, j, then pairwise distinct (i, j, k) with at least two of the three pairs adjacent."""
    n = G["n"]
    if kernel != "LWLC":
        return [(i, j, k) for i in range(n) for j in range(n) for k in range(n)]
    nb = [set(x) for x in G["nbrs"]]
    out = [(i, i, i) for i in range(n)]
    out += [(i, i, j) for i in range(n) for j in range(n) if j in nb[i]]
    for i in range(n):
        for j in range(n):
            if i == j:
                continue
            ij = j in nb[i]
            for k in range(n):
                if k != i and k != j and ij + (k in nb[j]) + (k in nb[i]) >= 2:
                    out.append((i, j, k))
    return out


def initial(G, kernel, use_node_labels=True, use_edge_labels=True):
    """{(i, j, k): colour} of iteration 0 (use_edge_labels is accepted and ignored, as in the reference)."""
    nb = [set(x) for x in G["nbrs"]]
    lab = G["labels"]
    out = {}
    for i, j, k in triples(G, kernel):
        if kernel != "LWLC":
            a, b, c = (1 if j in nb[i] else 2), (1 if k in nb[i] else 2), (1 if k in nb[j] else 2)
        elif i == j == k:
            a, b, c = 1, 1, 1
        elif i == j:
            a, b, c = 1, 3, 3
        else:
            a, b, c = (3 if j in nb[i] else 2), (3 if k in nb[i] else 2), (3 if k in nb[j] else 2)
        ci, cj, ck = 1, 2, 3
        if use_node_labels:
            ci, cj, ck = pairing((lab[i] + 1) & M64, 1), pairing((lab[j] + 1) & M64, 2), pairing((lab[k] + 1) & M64, 3)
        out[(i, j, k)] = pairing(pairing(pairing(a, b), c), pairing(pairing(ci, cj), ck))
    return out


def _fold(ms):
    """A non-empty multiset: ascending, start from the maximum, pair the rest in ascending order."""
    ms = sorted(ms)
    acc = ms.pop()
    for x in ms:
        acc = pairing(acc, x)
    return acc


def step(G, kernel, C):
    """One refinement: {(i, j, k): colour} -> {(i, j, k): colour}."""
    n, nbrs = G["n"], G["nbrs"]
    nb = [set(x) for x in nbrs]
    out = {}
    for (v, w, u), own in C.items():
        loc, glo = [[], [], []], [[], [], []]
        if kernel in ("LWL", "LWLC"):
            e1 = [C[(x, w, u)] for x in nbrs[v] if (x, w, u) in C] * 2
            e2 = [C[(v, x, u)] for x in nbrs[w] if (v, x, u) in C] * 2
            e3 = [C[(v, w, x)] for x in nbrs[u] if (v, w, x) in C] * 2
            loc = [e1, e2, e3] if kernel == "LWL" else [[], e1 + e2, e3]
        else:
            wl = kernel == "WL"
            for x in range(n):
                if x != v:
                    (loc if wl or x in nb[v] else glo)[0].extend([C[(x, w, u)]] * 2)
                if x != w:
                    (loc if wl or x in nb[w] else glo)[1].extend([C[(v, x, u)]] * 2)
                if x != u:
                    (loc if wl or x in nb[u] else glo)[2].extend([C[(v, w, x)]] * 2)
            (loc if wl else glo)[0].extend([own] * 6)
        folds = sorted(_fold(m) for m in loc if m) + sorted(_fold(m) for m in glo if m)
        acc = own
        for f in folds:
            acc = pairing(acc, f)
        out[(v, w, u)] = acc
    return out


def colors(G, num_iterations, kernel, use_node_labels=True, use_edge_labels=True):
    """[H + 1][items]: the colour of every item (in triples() order) after every iteration."""
    order = triples(G, kernel)
    C = initial(G, kernel, use_node_labels, use_edge_labels)
    out = [[C[t] for t in order]]
    for _ in range(num_iterations):
        C = step(G, kernel, C)
        out.append([C[t] for t in order])
    return out


def gram_matrices(graphs, num_iterations, kernel, use_node_labels=True, use_edge_labels=True):
    """The H + 1 integer matrices: the k = 1 WL maps and dot products over the triple colours."""
    feats = [wl_ref.features(colors(G, num_iterations, kernel, use_node_labels, use_edge_labels)) for G in graphs]
    return wl_ref.gram(feats, num_iterations, "WL")
