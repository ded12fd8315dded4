"""Pure-Python restatement of the reference's WL / WLOA graph kernels at k = 1 (graph_classification/graph_kernels: the reader of
src/AuxiliaryMethods.cpp:41-342, the colours and matrices of src/ColorRefinementKernel.cpp:80-306, the writer of
AuxiliaryMethods.cpp:437-485).  Python ints masked to 64 bits, `sorted` and dictionaries: no numpy, no torch, so it runs wherever
the tests run.  tests/test_graph_kernels_host.py holds it against the text the reference's own binary wrote
(tests/golden/graph_kernels.json); the GPU tests hold the kernels against it.
"""
M64 = (1 << 64) - 1
M32 = (1 << 32) - 1


def pairing(a, b):
    """Szudzik's pairing in wrapping unsigned 64-bit arithmetic (AuxiliaryMethods.cpp:488-492)."""
    return (a * a + a + b) & M64 if a >= b else (a + b * b) & M64


def read_graphs(graph_indicator, A, node_labels=None, edge_labels=None):
    """The reader: one dict per graph {n, labels (or None), nbrs (list of lists, insertion order), elabel {(v, w): label}}.
    The number of graphs is the LAST value of graph_indicator; an `A` line (v, w) adds the undirected edge unless v's list already
    holds w; the label of an ordered pair is the label of the first line that names the pair in either order (the edge-label map's
    values are 32-bit)."""
    B = graph_indicator[-1] if graph_indicator else 0
    sizes = [0] * (B + 1)
    for g in graph_indicator:
        sizes[g] += 1
    offset, graphs, run = [0] * (B + 1), [], 0
    for g in range(B + 1):
        offset[g] = run
        labels = None if node_labels is None else [int(x) & M64 for x in node_labels[run:run + sizes[g]]]
        graphs.append({"n": sizes[g], "labels": labels, "nbrs": [[] for _ in range(sizes[g])],
                       "elabel": None if edge_labels is None else {}})
        run += sizes[g]
    for c, (a, b) in enumerate(A):
        g = graph_indicator[a - 1]
        G = graphs[g]
        v, w = a - 1 - offset[g], b - 1 - offset[g]
        if w not in G["nbrs"][v]:
            G["nbrs"][v].append(w)
            G["nbrs"][w].append(v)
        if edge_labels is not None:
            G["elabel"].setdefault((v, w), int(edge_labels[c]) & M32)
            G["elabel"].setdefault((w, v), int(edge_labels[c]) & M32)
    return graphs[1:]                                     # graph 0 holds nothing (the ids are 1-based) and is erased (gram.cpp:112)


def colors(G, num_iterations, use_node_labels=True, use_edge_labels=True):
    """[H + 1][n]: the colour of every node after every iteration."""
    n = G["n"]
    cur = list(G["labels"]) if use_node_labels else [1] * n
    out = [cur]
    for _ in range(num_iterations):
        nxt = []
        for v in range(n):
            ent = []
            for w in G["nbrs"][v]:
                if use_edge_labels:
                    ent.append(pairing(cur[w], G["elabel"][(v, w)]))
                ent.append(cur[w])
            c = cur[v]
            for e in sorted(ent):
                c = pairing(c, e)
            nxt.append(c)
        out.append(nxt)
        cur = nxt
    return out


def features(cols):
    """(values, counts, steps) of one graph: the distinct colours of all iterations in ascending unsigned order (the std::map), how
    often each occurs, and for every sorted POSITION p the step h whose slice [nums[h - 1], nums[h]) holds it, nums[h] being the
    number of distinct colours seen up to iteration h.  While colours grow this is the iteration that made the colour; once they
    wrap it is not, and the slice is what the reference uses."""
    count, nums = {}, []
    for row in cols:
        for c in row:
            count[c] = count.get(c, 0) + 1
        nums.append(len(count))
    vals = sorted(count)
    steps, h = [], 0
    for p in range(len(vals)):
        while p >= nums[h]:
            h += 1
        steps.append(h)
    return vals, [count[v] for v in vals], steps


def gram(feats, num_iterations, kernel="WL"):
    """The H + 1 integer matrices [B][B]: matrix h uses of every graph the entries with step <= h; WL is the dot product of the
    counts, WLOA the sum of their minima with matrix 0 left all zero (ColorRefinementKernel.cpp:136)."""
    B, S = len(feats), num_iterations + 1
    maps = [{v: (c, s) for v, c, s in zip(*f)} for f in feats]
    out = [[[0] * B for _ in range(B)] for _ in range(S)]
    for i in range(B):
        for j in range(i, B):
            a, b = (maps[i], maps[j]) if len(maps[i]) <= len(maps[j]) else (maps[j], maps[i])
            bucket = [0] * S
            for v, (ca, sa) in a.items():
                hit = b.get(v)
                if hit is not None:
                    bucket[max(sa, hit[1])] += min(ca, hit[0]) if kernel == "WLOA" else ca * hit[0]
            run = 0
            for h in range(S):
                run += bucket[h]
                val = 0 if (kernel == "WLOA" and h == 0) else run
                out[h][i][j] = out[h][j][i] = val
    return out


def gram_matrices(graphs, num_iterations, kernel="WL", use_node_labels=True, use_edge_labels=True):
    feats = [features(colors(G, num_iterations, use_node_labels, use_edge_labels)) for G in graphs]
    return gram(feats, num_iterations, kernel)


def libsvm_text(G, classes):
    """The normalised matrix as the reference prints it: G_ij / (sqrt(G_ii) sqrt(G_jj)) in double, 0 where that product is 0, at the
    stream's default precision (%g)."""
    import math
    d = [math.sqrt(float(G[i][i])) for i in range(len(classes))]
    lines = []
    for i, cls in enumerate(classes):
        parts = ["%d 0:%d" % (cls, i + 1)]
        for j in range(len(classes)):
            x = d[i] * d[j]
            parts.append("%d:%s" % (j + 1, "%g" % (float(G[i][j]) / x if x != 0 else 0.0)))
        lines.append(" ".join(parts))
    return "\n".join(lines) + "\n"
