"""Kernel-SVM evaluation of gram matrices: the counterpart of the reference's third graph-kernel stage
(graph_classification/graph_kernels/seed_svm.py, driven by run.py after gram.out and merge_grams.py), quirks kept.

  reader            seed_svm.py:47-51 (load_svmlight_file, column 0 dropped)     read_gram (own parser: scikit-learn is not needed)
  normalisation     seed_svm.py:54-65  g_ij / sqrt(g_ii g_jj)                     normalize_gram_svm (NOT graph_kernels.normalize_gram,
                                                                                  which is the C++ tool's sqrt(g_ii) * sqrt(g_jj))
  split             seed_svm.py:125-135 torch.manual_seed + random_split          split_indices (a local generator)
  C search          seed_svm.py:15-44  SVC(kernel="precomputed", tol=1e-3)        kernel_svm_evaluation / evaluate_dataset: every
                                                                                  (seed, matrix, C, class pair) dual in ONE batch
                                                                                  (ops.svm_smo: dn_svm.hip, or ops.svm_smo_composed)
  table             seed_svm.py:158-185                                           format_table
  command line      seed_svm.py:68-102, run.py:116-151 (--add_origin)             python -m dummynode4graphlearning_amd.graph_kernels_svm

Multi-class is libsvm's one-vs-one over the sorted classes present in the training split: in the pair (a, b), a < b, class a is +1; a
positive decision value votes for a, anything else for b, and the first class with the most votes wins.

Two precision routes.  The file route (read_gram) sees the `%g`-rounded values of the .gram text and is the parity route: it
normalises what seed_svm.py normalises.  The in-memory route hands evaluate_dataset the exact integer matrices of wl_gram_matrices
and its siblings; its normalised values can differ from the file route's in the seventh digit.

Refused with ValueError: a gram matrix that is not square (the reference's feat_index branch multiplies row indices by a factor and
is not reproduced), a training split with a single class (as scikit-learn refuses it), and a matrix none of whose C values reaches
a validation accuracy above 0 (the reference dereferences None there)."""
import os
import sys

import numpy as np
import torch

from . import ops

C_GRID = np.power(10.0, np.arange(3.0, -4.0, -1))
ORIGIN_PREFIXES = ("LINE_", "DUMMY_", "CONJ_")


# ------------------------------------------------------------------------------------------------ reader, normalisation, split
def read_gram(path):
    """(float64 [n, n] numpy matrix, int64 classes) of a libsvm text `class 0:i 1:v 2:v ...` as graph_kernels.write_libsvm and the
    reference's binary write it; the `0:i` column is dropped.  ValueError unless every line is dense and the matrix square."""
    with open(path) as f:
        text = f.read()
    n = sum(1 for line in text.split("\n") if line.strip())
    if n == 0:
        raise ValueError("%s: no rows" % path)
    flat = np.fromstring(text.replace(":", " "), dtype=np.float64, sep=" ")
    if flat.size % n or (flat.size // n) % 2 != 1 or flat.size // n < 3:
        raise ValueError("%s: %d numbers in %d rows is not a dense `class 0:i 1:v ...` text" % (path, flat.size, n))
    table = flat.reshape(n, -1)
    cols = (table.shape[1] - 1) // 2
    if not (table[:, 1::2] == np.arange(cols, dtype=np.float64)[None, :]).all():
        raise ValueError("%s: the feature indices of a row are not 0, 1, 2, ... (a sparse or shuffled row)" % path)
    G = np.ascontiguousarray(table[:, 4::2])
    if G.shape[0] != G.shape[1]:
        raise ValueError("%s: %d rows of %d values: the matrix is not square (the reference's feat_index branch for such files is not "
                         "reproduced)" % (path, G.shape[0], G.shape[1]))
    return G, table[:, 0].astype(np.int64)


def normalize_gram_svm(G):
    """float64 G_ij / sqrt(G_ii * G_jj), 0 where either diagonal entry is 0: seed_svm.normalize_gram_matrix, its order of operations.
    A CPU tensor or array is normalised with numpy (correctly rounded square roots, as the reference's math.sqrt: torch's vectorised
    CPU square root differs in the last bit now and then) and is the parity route; a device tensor stays on its device."""
    G = torch.as_tensor(G)
    if not G.is_cuda:
        Gd = G.to(torch.float64).numpy()
        d = np.diagonal(Gd)
        ok = (d != 0)[:, None] & (d != 0)[None, :]
        x = np.sqrt(np.where(ok, d[:, None] * d[None, :], 1.0))
        return torch.from_numpy(np.where(ok, Gd / x, 0.0))
    Gd = G.to(torch.float64)
    d = torch.diagonal(Gd)
    ok = (d != 0).unsqueeze(1) & (d != 0).unsqueeze(0)
    x = torch.sqrt(torch.where(ok, d.unsqueeze(1) * d.unsqueeze(0), torch.ones_like(Gd)))
    return torch.where(ok, Gd / x, torch.zeros_like(x))


def split_indices(n, seed):
    """The reference's 80 / 10 / 10 split as three lists: what torch.manual_seed(seed); random_split(np.arange(n), [...]) yields, drawn
    from a local generator (the global one is left alone)."""
    n, g = int(n), torch.Generator()
    g.manual_seed(int(seed))
    perm = torch.randperm(n, generator=g).tolist()
    n_train, n_valid = int(n * 0.8), int(n * 0.1)
    return perm[:n_train], perm[n_train:n_train + n_valid], perm[n_train + n_valid:]


# ------------------------------------------------------------------------------------------------ evaluation
def _stack(matrices, device, normalize):
    """[M, n, n] float64 on `device` (None: where the first matrix lives), each matrix normalised where it lives first."""
    ms = [torch.as_tensor(m) for m in matrices]
    if not ms:
        raise ValueError("no gram matrices")
    device = ms[0].device if device is None else torch.device(device)
    for m in ms:
        if m.dim() != 2 or m.shape[0] != m.shape[1] or m.shape != ms[0].shape:
            raise ValueError("a gram matrix of shape %s: every matrix must be square and of one size" % (tuple(m.shape),))
    if normalize:
        ms = [normalize_gram_svm(m) for m in ms]
    return torch.stack([m.to(device=device, dtype=torch.float64) for m in ms]).contiguous()


def _solve_plan(classes, splits, num_matrices, Cs):
    """The batch of one evaluation: per split its sorted training classes and pairs, and for every (split, matrix, C, pair) a table
    row {matrix, offset, length, positives, C} over its own copy of the pair's row list (class a's training rows, then class b's,
    each in the split's order -- libsvm's grouping)."""
    table, rows, plans, off = [], [], [], 0
    for train, _, _ in splits:
        tc = classes[train]
        present = np.unique(tc)
        if present.size < 2:
            raise ValueError("The number of classes has to be greater than one; got %d class" % present.size)
        train = np.asarray(train, dtype=np.int64)
        pairs = [(a, b) for x, a in enumerate(present) for b in present[x + 1:]]
        first = len(table)
        for m in range(num_matrices):
            for c in Cs:
                for a, b in pairs:
                    ra, rb = train[tc == a], train[tc == b]
                    rows += [ra, rb]
                    table.append((m, off, ra.size + rb.size, ra.size, float(c)))
                    off += ra.size + rb.size
        plans.append((present, pairs, first))
    return np.array(table, dtype=np.float64), np.concatenate(rows).astype(np.int32), plans


def _vote(dec, num_classes, pairs_index):
    """libsvm's vote over one-vs-one decision values dec [rows, pairs]: positive -> the pair's first class, else its second; the
    first class with the most votes.  Returns class positions [rows]."""
    votes = np.zeros((dec.shape[0], num_classes), dtype=np.int64)
    for p, (x, z) in enumerate(pairs_index):
        win = dec[:, p] > 0
        votes[:, x] += win
        votes[:, z] += ~win
    return votes.argmax(1)


def solve_batch(K, classes, splits, Cs=None, eps=1e-3, iters_per_launch=None):
    """Every dual of an evaluation and its decision values.  K [M, n, n] float64 normalised matrices on one device, classes [n],
    splits a list of (train, valid, test) index lists.  Returns a dict: `decision` [splits][M][C] -> numpy [n, pairs] (one-vs-one
    decision values of ALL n rows, libsvm's sign: positive = the pair's first class), `present` / `pairs` per split, and the raw
    solver output (`table`, `rows`, `alpha`, `rho`, `iterations`, `status`)."""
    Cs = C_GRID if Cs is None else np.asarray(Cs, dtype=np.float64)
    classes = np.asarray(classes)
    M, n = int(K.shape[0]), int(K.shape[1])
    if classes.shape[0] != n:
        raise ValueError("%d classes for %d x %d matrices" % (classes.shape[0], n, n))
    table_h, rows_h, plans = _solve_plan(classes, splits, M, Cs)
    table, rows = torch.from_numpy(table_h).to(K.device), torch.from_numpy(rows_h).to(K.device)
    max_len = int(table_h[:, 2].max())
    fused = ops.svm_fused_enabled() and ops.svm_smo_supported(K, max_len)
    alpha, rho, iterations, status = (ops.svm_smo if fused else ops.svm_smo_composed)(K, table, rows, eps, iters_per_launch)
    # decision values: per matrix one product K_m @ W, column s of W = the solve's alpha * y scattered to its rows
    S = table_h.shape[0]
    offs, lens, npos = table_h[:, 1].astype(np.int64), table_h[:, 2].astype(np.int64), table_h[:, 3].astype(np.int64)
    solve_of = torch.from_numpy(np.repeat(np.arange(S), lens)).to(K.device)
    within = torch.from_numpy(np.arange(rows_h.size) - np.repeat(offs, lens)).to(K.device)
    sign = torch.where(within < torch.from_numpy(npos).to(K.device)[solve_of], 1.0, -1.0).to(torch.float64)
    W = torch.zeros((n, S), dtype=torch.float64, device=K.device)
    W[rows.long(), solve_of] = alpha * sign
    mat_of = torch.from_numpy(table_h[:, 0].astype(np.int64)).to(K.device)
    dec = torch.empty((n, S), dtype=torch.float64, device=K.device)
    for m in range(M):
        cols = torch.nonzero(mat_of == m).view(-1)
        dec[:, cols] = K[m] @ W[:, cols]
    dec = (dec - rho.unsqueeze(0)).cpu().numpy()
    decision = []
    for present, pairs, first in plans:
        P = len(pairs)
        decision.append([[dec[:, first + (m * len(Cs) + c) * P: first + (m * len(Cs) + c + 1) * P] for c in range(len(Cs))]
                         for m in range(M)])
    return dict(decision=decision, present=[p[0] for p in plans], pairs=[p[1] for p in plans], Cs=Cs, fused=fused, table=table_h,
                rows=rows_h, alpha=alpha, rho=rho, iterations=iterations, status=status)


def _accuracy(pred, true):
    return float(np.average(pred == true)) * 100.0


def select(batch, classes, splits):
    """seed_svm.kernel_svm_evaluation's search over a solved batch: per (split, matrix) the C values in order, a candidate replacing
    the best only when its validation accuracy is strictly higher; train and test accuracy of the best fit.  Returns the three
    [splits, M] arrays, the chosen C [splits, M] and the predictions [splits][M][C] -> class per row."""
    classes = np.asarray(classes)
    S, M, Cs = len(splits), len(batch["decision"][0]), batch["Cs"]
    train_acc, valid_acc, test_acc, chosen = (np.zeros((S, M)) for _ in range(4))
    predictions = []
    for s, (train, valid, test) in enumerate(splits):
        present = batch["present"][s]
        where = {c: x for x, c in enumerate(present)}
        pairs_index = [(where[a], where[b]) for a, b in batch["pairs"][s]]
        predictions.append([])
        for m in range(M):
            best_valid, best = 0.0, None
            preds = [present[_vote(batch["decision"][s][m][c], present.size, pairs_index)] for c in range(len(Cs))]
            predictions[s].append(preds)
            for c in range(len(Cs)):
                acc = _accuracy(preds[c][valid], classes[valid])
                if best_valid < acc:
                    best_valid, best = acc, c
            if best is None:
                raise ValueError("matrix %d, split %d: no C reaches a validation accuracy above 0 (the reference dereferences None "
                                 "here: best_clf stays unset)" % (m, s))
            valid_acc[s, m], chosen[s, m] = best_valid, Cs[best]
            train_acc[s, m] = _accuracy(preds[best][train], classes[train])
            test_acc[s, m] = _accuracy(preds[best][test], classes[test])
    return train_acc, valid_acc, test_acc, chosen, predictions


def kernel_svm_evaluation(matrices, classes, train_index, valid_index, test_index, C=None, eps=1e-3, device=None, normalize=False,
                          iters_per_launch=None):
    """The three accuracy arrays [num_matrices] of ONE split: seed_svm.kernel_svm_evaluation on whole (normalised) matrices and the
    split's index lists (normalize=True normalises them here)."""
    tr, va, te = evaluate_dataset(matrices, classes, None, C=C, eps=eps, device=device, normalize=normalize,
                                  splits=[(list(train_index), list(valid_index), list(test_index))], iters_per_launch=iters_per_launch)
    return tr[0], va[0], te[0]


def evaluate_dataset(matrices, classes, seeds, C=None, eps=1e-3, device=None, normalize=True, splits=None, iters_per_launch=None):
    """The three [len(seeds), num_matrices] accuracy arrays (train, valid, test) of a dataset.  matrices: a list of [n, n] tensors or
    arrays, read from files or already on the device from wl_gram_matrices and its siblings (normalize=True: normalize_gram_svm
    first, as seed_svm.py does after reading).  Every (seed, matrix, C, class pair) dual is solved in one batch."""
    K = _stack(matrices, device, normalize)
    if splits is None:
        splits = [split_indices(K.shape[1], seed) for seed in seeds]
    batch = solve_batch(K, classes, splits, C, eps, iters_per_launch)
    return select(batch, classes, splits)[:3]


# ------------------------------------------------------------------------------------------------ the table
def kernel_name(kernel, k):
    """seed_svm.py:87-89."""
    return kernel + str(k) if kernel == "WL" or k != 1 else kernel


def format_table(kernel, dataset, train_all, valid_all, test_all):
    """The reference's output lines (seed_svm.py:158-185), character for character: one per matrix, then the -avg line over each
    seed's argmax of the validation accuracy.  `kernel` as kernel_name gives it."""
    train_all, valid_all, test_all = (np.asarray(x, dtype=np.float64) for x in (train_all, valid_all, test_all))

    def line(tag, tr, va, te):
        return "\t".join(str(x) for x in (tag, dataset, round(tr.mean(), 2), round(tr.std(), 2), round(va.mean(), 2), round(va.std(), 2),
                                          round(te.mean(), 2), round(te.std(), 2)))

    lines = [line("%s-%d" % (kernel, k), train_all[:, k], valid_all[:, k], test_all[:, k]) for k in range(valid_all.shape[1])]
    best = np.expand_dims(valid_all.argmax(axis=1), axis=1)
    take = lambda x: np.take_along_axis(x, best, axis=1).squeeze(axis=1)  # noqa: E731
    return lines + [line(kernel + "-avg", take(train_all), take(valid_all), take(test_all))]


# ------------------------------------------------------------------------------------------------ command line
def origin_dataset(dataset):
    """run.py:126-133: the dataset a DUMMY_ / LINE_ / CONJ_ dataset was made from."""
    for prefix in ORIGIN_PREFIXES:
        if dataset.startswith(prefix):
            return dataset[len(prefix):]
    raise ValueError("--add_origin: %s has none of the prefixes %s" % (dataset, ", ".join(ORIGIN_PREFIXES)))


def _as_merged_file(G):
    """What seed_svm.py reads back after merge_grams.py wrote the sum: dump_svmlight_file prints doubles with %.16g, one digit short of
    a round trip, so a sum can come back one bit off.  Each distinct value is printed and parsed once."""
    values, inverse = np.unique(G, return_inverse=True)
    return np.array([float("%.16g" % v) for v in values.tolist()], dtype=np.float64)[inverse].reshape(G.shape)


def read_dataset_grams(gram_dir, dataset, kernel, n_iters, add_origin=False):
    """The matrices seed_svm.py would read for a dataset: <gram_dir>/<dataset>__<kernel>_<i>.gram for i = 0 .. n_iters, absent files
    skipped; add_origin adds the origin dataset's matrix i to each (run.py + merge_grams.py, in memory)."""
    out = []
    for i in range(n_iters + 1):
        path = os.path.join(gram_dir, "%s__%s_%d.gram" % (dataset, kernel, i))
        if not os.path.exists(path):
            continue
        G, _ = read_gram(path)
        if add_origin:
            O, _ = read_gram(os.path.join(gram_dir, "%s__%s_%d.gram" % (origin_dataset(dataset), kernel, i)))
            if O.shape != G.shape:
                raise ValueError("%s: the origin's matrix is %s, not %s" % (path, O.shape, G.shape))
            G = _as_merged_file(O + G)
        out.append(G)
    return out


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(prog="python -m dummynode4graphlearning_amd.graph_kernels_svm",
                                 description="C-SVC evaluation of gram files over seeds, in the reference's output")
    ap.add_argument("--gram_dir", type=str, default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "GM", "EXP"),
                    help="the directory of gram matrices")
    ap.add_argument("--dataset_dir", type=str, default="../data_processing/tu_data", help="the directory of gram matrices")
    ap.add_argument("--k", type=int, default=1, help="complexity of kernel functions")
    ap.add_argument("--kernel", type=str, default="WL", help="kernel function")
    ap.add_argument("--n_iters", type=int, default=5, help="number of runs")
    ap.add_argument("--seeds", nargs="+", help="seeds")
    ap.add_argument("--datasets", nargs="+", help="datasets")
    ap.add_argument("--add_origin", type=str, default="false", help="add the origin dataset's gram matrices (run.py's switch)")
    ap.add_argument("--device", default="cuda")
    args = ap.parse_args(argv)
    kernel = kernel_name(args.kernel, args.k)
    for dataset in args.datasets:
        tried = [os.path.join(args.dataset_dir, dataset, dataset + "_graph_labels.txt"),
                 os.path.join(args.dataset_dir, dataset, "raw", dataset + "_graph_labels.txt")]
        found = [p for p in tried if os.path.exists(p)]
        if not found:
            print("%s and %s are not found." % tuple(tried))
            continue
        with open(found[0], "r") as f:
            classes = np.asarray(f.readlines(), dtype=np.int32)
        matrices = read_dataset_grams(args.gram_dir, dataset, kernel, args.n_iters, add_origin=args.add_origin == "true")
        if len(matrices) == 0:
            print("Gram matrices for %s are not found." % (dataset))
            continue
        accs = evaluate_dataset(matrices, classes, [int(s) for s in args.seeds], device=args.device)
        for line in format_table(kernel, dataset, *accs):
            print(line)
    return 0


if __name__ == "__main__":
    sys.exit(main())
