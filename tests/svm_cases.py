"""Shared by tests/test_graph_kernels_svm_host.py (composed path, CPU tensors) and tests/test_gpu_graph_kernels_svm.py (dn_svm.hip): the
golden cases of tests/golden/graph_kernels_svm.json (written by the reference's seed_svm.py on scikit-learn) and the checks both
paths must pass.

The agreement band.  Two eps-optimal solutions of one dual agree only up to a distance that depends on the problem, so the golden
holds it measured: `delta[c]` = the largest absolute difference between scikit-learn's decision values at tol = 1e-3 and at
tol = 1e-7 for C value c.  The band of a case is 10 x its largest delta (`band`; the factor is room for this solver's different
iterates at the same eps: fp64 kernel rows where libsvm keeps float ones, ties to the lowest index where libsvm takes the last).
Every decision value must lie within the band of the golden's; predictions must be equal wherever every golden decision value of
the row lies outside the band; the values excluded that way are counted and must stay at or below 5 % of the case's.

KKT, computed here in fp64 on the CPU from the returned alpha: 0 <= alpha <= C, m - M <= eps = 1e-3 with libsvm's I_up / I_low, and
|y^T alpha| at most 10 x the residual of the golden's dual coefficients with a floor of 1e-12 C l (the rounding of l additions of
magnitudes up to C)."""
import functools
import hashlib
import json
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "graph_kernels_svm.json")
EPS = 1e-3


@functools.lru_cache(maxsize=None)
def golden():
    with open(GOLDEN) as f:
        g = json.load(f)
    return g


def cases():
    return golden()["cases"]


def case(name):
    return [c for c in cases() if c["name"] == name][0]


def names():
    return [c["name"] for c in cases()]


def gram_texts(c):
    """The case's gram texts (bin300: rebuilt from its count rows with write_libsvm and held against the stored digests)."""
    if "gram_text" in c:
        return c["gram_text"]
    from dummynode4graphlearning_amd import graph_kernels as gk
    import tempfile
    X = np.array(c["counts"], dtype=np.int64)
    out = []
    with tempfile.TemporaryDirectory() as tmp:
        for d, sha in zip(c["dims"], c["gram_text_sha256"]):
            p = os.path.join(tmp, "g.gram")
            gk.write_libsvm(torch.from_numpy(X[:, :d] @ X[:, :d].T), c["classes"], p)
            with open(p) as f:
                out.append(f.read())
            assert hashlib.sha256(out[-1].encode()).hexdigest() == sha
    return out


def write_files(c, root):
    """<root>/data/<name>/<name>_graph_labels.txt and <root>/gram/<name>__WL1_<i>.gram (and the origin's): what the command line reads."""
    data, gdir = os.path.join(root, "data"), os.path.join(root, "gram")
    os.makedirs(os.path.join(data, c["name"], "raw"), exist_ok=True)
    os.makedirs(gdir, exist_ok=True)
    with open(os.path.join(data, c["name"], "raw", c["name"] + "_graph_labels.txt"), "w") as f:       # (found in raw/)
        f.write("".join("%d\n" % k for k in c["classes"]))
    for i, text in enumerate(gram_texts(c)):
        with open(os.path.join(gdir, "%s__WL1_%d.gram" % (c["name"], i)), "w") as f:
            f.write(text)
    for i, text in enumerate(c.get("origin_gram_text", [])):
        with open(os.path.join(gdir, "%s__WL1_%d.gram" % (c["origin_name"], i)), "w") as f:
            f.write(text)
    return data, gdir


@functools.lru_cache(maxsize=None)
def raw_matrices(name):
    """What the evaluation normalises: the matrices read from the case's files (with the origin's added where the case has one)."""
    import tempfile
    from dummynode4graphlearning_amd import graph_kernels_svm as svm
    c = case(name)
    with tempfile.TemporaryDirectory() as tmp:
        _, gdir = write_files(c, tmp)
        return svm.read_dataset_grams(gdir, c["name"], "WL1", c["n_iters"], add_origin="origin_name" in c)


@functools.lru_cache(maxsize=None)
def normalized(name):
    from dummynode4graphlearning_amd import graph_kernels_svm as svm
    return torch.stack([svm.normalize_gram_svm(torch.from_numpy(m)) for m in raw_matrices(name)]).contiguous()


def splits(c):
    return [tuple(list(x) for x in sp) for sp in c["splits"]]


def solve(name, device, fused, iters_per_launch=None):
    from dummynode4graphlearning_amd import graph_kernels_svm as svm, ops
    c = case(name)
    K = normalized(name).to(device)
    with ops.svm_fused(fused):
        return svm.solve_batch(K, np.array(c["classes"]), splits(c), eps=EPS, iters_per_launch=iters_per_launch)


def check_kkt(c, batch, K):
    """K: the normalised matrices on the CPU."""
    table, rows = batch["table"], batch["rows"]
    alpha = batch["alpha"].cpu().numpy()
    K = K.numpy()
    nC = len(golden()["C"])
    worst = 0.0
    for s in range(table.shape[0]):
        m, off, l, npos, C = int(table[s, 0]), int(table[s, 1]), int(table[s, 2]), int(table[s, 3]), table[s, 4]
        r, a = rows[off:off + l], alpha[off:off + l]
        y = np.where(np.arange(l) < npos, 1.0, -1.0)
        assert (a >= 0).all() and (a <= C).all(), (c["name"], s)
        G = (y[:, None] * y[None, :] * K[m][np.ix_(r, r)]) @ a - 1.0
        v = -y * G
        up = np.where(y > 0, a < C, a > 0)
        low = np.where(y > 0, a > 0, a < C)
        gap = (v[up].max() if up.any() else -np.inf) - (v[low].min() if low.any() else np.inf)
        worst = max(worst, gap)
        assert gap <= EPS, (c["name"], s, gap)
    # |y^T alpha| per solve against the golden's residual: the solves of a split are ordered (matrix, C, pair)
    s = 0
    for sp, fits in enumerate(c["fits"]):
        for m, per_c in enumerate(fits):
            for ci in range(nC):
                for p, yta in enumerate(per_c[ci]["yta"]):
                    off, l, npos, C = int(table[s, 1]), int(table[s, 2]), int(table[s, 3]), table[s, 4]
                    a = alpha[off:off + l]
                    mine = abs(a[:npos].sum() - a[npos:].sum())
                    assert mine <= max(10.0 * yta, 1e-12 * C * l), (c["name"], sp, m, ci, p, mine, yta)
                    s += 1
    assert s == table.shape[0]
    return worst


def check_band(c, batch):
    """Decision values within the band, predictions equal outside it, the excluded share <= 5 %.  Returns (share, worst distance)."""
    from dummynode4graphlearning_amd import graph_kernels_svm as svm
    band, nC = c["band"], len(golden()["C"])
    classes = np.array(c["classes"])
    _, _, _, _, preds = svm.select(batch, classes, splits(c))
    total = inside = 0
    worst = 0.0
    for sp, fits in enumerate(c["fits"]):
        for m, per_c in enumerate(fits):
            for ci in range(nC):
                want = np.array(per_c[ci]["decision"], dtype=np.float64)
                got = batch["decision"][sp][m][ci]
                assert got.shape == want.shape
                dist = np.abs(got - want).max()
                worst = max(worst, dist)
                assert dist <= band, (c["name"], sp, m, ci, dist, band)
                near = np.abs(want) <= band
                total += want.size
                inside += int(near.sum())
                sure = ~near.any(axis=1)
                assert np.array_equal(preds[sp][m][ci][sure], np.array(per_c[ci]["prediction"])[sure]), (c["name"], sp, m, ci)
    assert inside / total <= 0.05, (c["name"], inside, total)
    return inside / total, worst


def check_table(c, batch):
    """On exact_table cases: the accuracy arrays, the chosen C values and the printed lines equal the golden's."""
    from dummynode4graphlearning_amd import graph_kernels_svm as svm
    tr, va, te, chosen, _ = svm.select(batch, np.array(c["classes"]), splits(c))
    acc = np.array(c["accuracies"])                                          # [split][train / valid / test][matrix]
    assert np.array_equal(tr, acc[:, 0]) and np.array_equal(va, acc[:, 1]) and np.array_equal(te, acc[:, 2])
    assert np.array_equal(chosen, np.array(c["chosen_c"]))
    if c["lines"] is not None:
        assert svm.format_table("WL1", c["name"], tr, va, te) == c["lines"]


def check_case(name, batch):
    c = case(name)
    worst_gap = check_kkt(c, batch, normalized(name))
    share, worst = check_band(c, batch)
    if c["exact_table"]:
        check_table(c, batch)
    print("%s: largest m - M %.3g, largest distance to the golden's decision values %.3g (band %.3g), share inside the band %.4f"
          % (name, worst_gap, worst, c["band"], share))
