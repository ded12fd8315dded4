"""Pure-Python restatement of the reference's shortest-path and graphlet graph kernels (graph_classification/graph_kernels:
src/ShortestPathKernel.cpp, src/GraphletKernel.cpp), on the graphs of wl_ref.read_graphs.  Python ints masked to 64 bits and
dictionaries: no numpy, no torch.  tests/test_graph_kernels_spgr_host.py holds it against the text the reference's own binary
wrote (tests/golden/graph_kernels_spgr.json); the GPU tests hold the kernels against it.

SP.  d(a, b) is the hop distance for a != b, INT_MAX where b cannot be reached; d(a, a) is 2 where a has a neighbour and INT_MAX
where it has none (the reference's Floyd-Warshall runs in place over j >= i and starts the diagonal at "no edge").  Every ordered
pair (a, b), a != b, adds 1 to the triple (lo32(l_a), l_b, d(a, b)); a == b adds 2.  The reference's filter reads the triple's FIRST
component: a triple is dropped where lo32(l_a) is 0 or INT_MAX -- whatever the distance is, INT_MAX included.

GR.  Every unordered wedge u - v - w and every unordered triangle counts 1 under one unsigned 64-bit key; a wedge and a triangle of
the same key are the same feature.
"""
from wl_ref import M32, pairing

INT_MAX = 2147483647


def P(xs):
    """AuxiliaryMethods::pairing(vector): the fold that starts at the list's length."""
    c = len(xs)
    for x in xs:
        c = pairing(c, x)
    return c


def sp_distances(G):
    """[n][n] by one BFS per node, with the reference's diagonal."""
    n, nbrs = G["n"], G["nbrs"]
    out = []
    for a in range(n):
        d = [INT_MAX] * n
        seen = [False] * n
        seen[a] = True
        frontier, level = [a], 0
        while frontier:
            level += 1
            nxt = []
            for v in frontier:
                for w in nbrs[v]:
                    if not seen[w]:
                        seen[w] = True
                        d[w] = level
                        nxt.append(w)
            frontier = nxt
        d[a] = 2 if nbrs[a] else INT_MAX
        out.append(d)
    return out


def sp_features(G, use_node_labels=True):
    """{(lo32(l_a), l_b, d): count} of one graph."""
    n = G["n"]
    lab = G["labels"] if use_node_labels else [1] * n
    dist = sp_distances(G)
    feat = {}
    for a in range(n):
        la = lab[a] & M32
        if la == 0 or la == INT_MAX:
            continue
        for b in range(n):
            k = (la, lab[b], dist[a][b])
            feat[k] = feat.get(k, 0) + (2 if a == b else 1)
    return feat


def gr_features(G, use_node_labels=True, use_edge_labels=True):
    """{key: count} of one graph."""
    n, nbrs = G["n"], G["nbrs"]
    lab, el = G["labels"], G["elabel"]
    adj = [set(x) for x in nbrs]
    feat = {}

    def add(k):
        feat[k] = feat.get(k, 0) + 1

    for v in range(n):
        ns = sorted(nbrs[v])
        for i, u in enumerate(ns):
            for w in ns[i + 1:]:
                if w in adj[u]:
                    if not (v < u):                       # each triangle once, at its smallest node (u < w already)
                        continue
                    if not use_node_labels:
                        add(3)
                    elif use_edge_labels:
                        lu, lv, lw, uv, uw, vw = lab[u], lab[v], lab[w], el[(u, v)], el[(u, w)], el[(v, w)]
                        add(min(P([lu, uv, lv, vw, lw, uw]), P([lu, uw, lw, vw, lv, uv]), P([lv, uv, lu, uw, lw, vw]),
                                P([lv, vw, lw, uw, lu, uv]), P([lw, uw, lu, uv, lv, vw]), P([lw, vw, lv, uv, lu, uw])))
                    else:
                        add(P(sorted([lab[u], lab[v], lab[w]])))
                else:
                    if not use_node_labels:
                        add(2)
                    elif use_edge_labels:
                        lu, lv, lw, uv, vw = lab[u], lab[v], lab[w], el[(u, v)], el[(v, w)]
                        add(min(P([lu, uv, lv, vw, lw]), P([lw, vw, lv, uv, lu])))
                    else:
                        add(min(P([lab[u], lab[v], lab[w]]), P([lab[w], lab[v], lab[u]])))
    return feat


def gram(feats):
    """[B][B]: the dot products of the count dictionaries."""
    B = len(feats)
    out = [[0] * B for _ in range(B)]
    for i in range(B):
        for j in range(i, B):
            a, b = (feats[i], feats[j]) if len(feats[i]) <= len(feats[j]) else (feats[j], feats[i])
            s = sum(c * b[k] for k, c in a.items() if k in b)
            out[i][j] = out[j][i] = s
    return out


def sp_gram(graphs, use_node_labels=True):
    return gram([sp_features(G, use_node_labels) for G in graphs])


def gr_gram(graphs, use_node_labels=True, use_edge_labels=True):
    return gram([gr_features(G, use_node_labels, use_edge_labels) for G in graphs])

