"""Pure-Python restatement of the reference's 2-WL graph kernels (graph_classification/graph_kernels: `gram --k 2 --kernel WL | DWL |
LWL | LWLC`, i.e. GenerateTwo::compute_colors_simple of src/GenerateTwo.cpp:450-750 over the tuple graphs of :752 on, driven by
gram.cpp:195-250).  On the reader, the pairing function, the per-graph colour maps and the matrices of tests/wl_ref.py; Python ints
masked to 64 bits, no numpy, no torch.  tests/test_graph_kernels_kwl_host.py holds it against the text the reference's own binary
wrote (tests/golden/graph_kernels_kwl.json); the GPU tests hold the kernels against it.

The tuple graph is never built: its adjacency lists are restated as gathers from the colour matrix C[a][b] of the previous
iteration.  The tuple graph is undirected and its add_edge pushes both ends, so every neighbour sits in a list TWICE; in WL and DWL
both exchange loops also reach the tuple itself, the edge-type map keeps the first insertion (type 1), and each of the two self
add_edge calls pushes twice: the tuple's own colour enters the type-1 multiset FOUR times (DWL: the global one, has_edge(v, v)
being false).
"""
import wl_ref
from wl_ref import M64, pairing

KERNELS = ("WL", "DWL", "LWL", "LWLC")


def tuples(G, kernel):
    """The tuples of one graph in the reference's order: all ordered pairs, row-major; LWLC: only i == j or j in N(i)."""
    n = G["n"]
    if kernel != "LWLC":
        return [(i, j) for i in range(n) for j in range(n)]
    nb = [set(x) for x in G["nbrs"]]
    return [(i, j) for i in range(n) for j in range(n) if i == j or j in nb[i]]


def initial(G, kernel, use_node_labels=True, use_edge_labels=True):
    """{(i, j): colour} of iteration 0."""
    nb = [set(x) for x in G["nbrs"]]
    out = {}
    for i, j in tuples(G, kernel):
        ci = pairing((G["labels"][i] + 1) & M64, 1) if use_node_labels else 1
        cj = pairing((G["labels"][j] + 1) & M64, 2) if use_node_labels else 2
        if j in nb[i]:
            c = pairing(3, G["elabel"][(i, j)]) if use_edge_labels else 3
        else:
            c = 1 if i == j else 2
        out[(i, j)] = pairing(pairing(ci, cj), c)
    return out


def _fold(ms):
    """A non-empty multiset: ascending, start from the maximum, pair the rest in ascending order."""
    ms = sorted(ms)
    acc = ms.pop()
    for x in ms:
        acc = pairing(acc, x)
    return acc


def step(G, kernel, C):
    """One refinement: {(i, j): colour} -> {(i, j): colour}."""
    n, nbrs = G["n"], G["nbrs"]
    nb = [set(x) for x in nbrs]
    out = {}
    for (v, w), own in C.items():
        l1, l2, g1, g2 = [], [], [], []
        if kernel in ("LWL", "LWLC"):
            l1 = [C[(x, w)] for x in nbrs[v] if (x, w) in C] * 2
            l2 = [C[(v, x)] for x in nbrs[w] if (v, x) in C] * 2
        else:
            for x in range(n):
                if x != v:
                    (l1 if kernel == "WL" or x in nb[v] else g1).extend([C[(x, w)]] * 2)
                if x != w:
                    (l2 if kernel == "WL" or x in nb[w] else g2).extend([C[(v, x)]] * 2)
            (l1 if kernel == "WL" else g1).extend([own] * 4)
        folds = sorted(_fold(m) for m in (l1, l2) if m) + sorted(_fold(m) for m in (g1, g2) if m)
        acc = own
        for f in folds:
            acc = pairing(acc, f)
        out[(v, w)] = acc
    return out


def colors(G, num_iterations, kernel, use_node_labels=True, use_edge_labels=True):
    """[H + 1][tuples]: the colour of every tuple (in tuples() order) after every iteration."""
    order = tuples(G, kernel)
    C = initial(G, kernel, use_node_labels, use_edge_labels)
    out = [[C[t] for t in order]]
    for _ in range(num_iterations):
        C = step(G, kernel, C)
        out.append([C[t] for t in order])
    return out


def gram_matrices(graphs, num_iterations, kernel, use_node_labels=True, use_edge_labels=True):
    """The H + 1 integer matrices: the k = 1 WL maps and dot products over the tuple colours."""
    feats = [wl_ref.features(colors(G, num_iterations, kernel, use_node_labels, use_edge_labels)) for G in graphs]
    return wl_ref.gram(feats, num_iterations, "WL")
