"""CPU tests of the kernel-SVM evaluation (graph_kernels_svm.py on ops.svm_smo_composed) against tests/golden/graph_kernels_svm.json,
which the reference's seed_svm.py wrote on scikit-learn: reader, normalisation (bit-equal), splits, table text, the --add_origin sum,
the composed path end to end on CPU tensors (KKT, agreement band, predictions, tables: tests/svm_cases.py states the bounds), the
two-row closed form, the error paths and the command line."""
import hashlib
import os

import numpy as np
import pytest
import torch

import svm_cases as S


def _svm():
    from dummynode4graphlearning_amd import graph_kernels_svm
    return graph_kernels_svm


# ------------------------------------------------------------------------------------------------ reader, normalisation, split, table
def test_read_gram_drops_column_zero_and_refuses_what_it_cannot_read(tmp_path):
    svm = _svm()
    p = tmp_path / "a.gram"
    p.write_text("1 0:1 1:1 2:0.5\n-1 0:2 1:0.5 2:1e-05\n")
    G, classes = svm.read_gram(str(p))
    assert G.dtype == np.float64 and G.tolist() == [[1.0, 0.5], [0.5, 1e-05]] and classes.tolist() == [1, -1]
    p.write_text("1 0:1 1:1 2:0.5 3:2\n-1 0:2 1:0.5 2:1 3:2\n")
    with pytest.raises(ValueError, match="not square"):
        svm.read_gram(str(p))
    p.write_text("1 0:1 2:1 1:0.5\n-1 0:2 1:0.5 2:1\n")
    with pytest.raises(ValueError, match="feature indices"):
        svm.read_gram(str(p))
    p.write_text("1 0:1 1:1 2:0.5\n-1 0:2 1:0.5\n")
    with pytest.raises(ValueError, match="not a dense"):
        svm.read_gram(str(p))
    p.write_text("\n")
    with pytest.raises(ValueError, match="no rows"):
        svm.read_gram(str(p))


@pytest.mark.parametrize("name", S.names())
def test_read_and_normalise_equal_the_golden_bit_for_bit(name):
    c = S.case(name)
    raw, norm = S.raw_matrices(name), S.normalized(name)
    assert len(raw) == c["n_iters"] + 1
    sha = lambda a: hashlib.sha256(np.ascontiguousarray(a, dtype=np.float64).tobytes()).hexdigest()  # noqa: E731
    if "merged_sha256" in c:                                                 # --add_origin: the origin's matrix added in memory equals
        for mine, want, row in zip(raw, c["merged_sha256"], c["merged_row5"]):        # what seed_svm.read_lib_svm read from the merged file
            assert mine[5].tolist() == row and sha(mine) == want
    if "normalized" in c:
        assert np.array_equal(norm.numpy(), np.array(c["normalized"], dtype=np.float64))
    else:
        for g, want, row in zip(norm.numpy(), c["normalized_sha256"], c["normalized_row5"]):
            assert g[5].tolist() == row and sha(g) == want
    assert (norm[:, 2] == 0).all() or name in ("two_rows", "DUMMY_TOYS")     # the synthetic cases' zero row


def test_normalisation_is_the_script_order_not_the_tools():
    """g / sqrt(g_ii g_jj) against g / (sqrt(g_ii) sqrt(g_jj)): the two differ in the last bit somewhere on this matrix."""
    from dummynode4graphlearning_amd import graph_kernels as gk
    import math
    rng = np.random.default_rng(5)
    X = rng.poisson(3.0, size=(40, 9)).astype(np.int64)
    X[7] = 0
    G = torch.from_numpy(X @ X.T)
    mine = _svm().normalize_gram_svm(G).numpy()
    want = np.zeros((40, 40))
    for i in range(40):
        for j in range(40):
            if G[i, i] != 0 and G[j, j] != 0:
                want[i, j] = float(G[i, j]) / math.sqrt(float(G[i, i]) * float(G[j, j]))
    assert np.array_equal(mine, want) and (mine[7] == 0).all() and (mine[:, 7] == 0).all()
    assert not np.array_equal(mine, gk.normalize_gram(G).numpy())


@pytest.mark.parametrize("name", [n for n in S.names() if n != "two_rows"])
def test_split_indices_reproduce_the_global_generators_permutation(name):
    c = S.case(name)
    state = torch.random.get_rng_state()
    for seed, want in zip(c["seeds"], c["splits"]):
        assert [list(x) for x in _svm().split_indices(len(c["classes"]), seed)] == want
    assert torch.equal(torch.random.get_rng_state(), state)                  # the global generator is not touched


@pytest.mark.parametrize("name", [n for n in S.names() if n != "two_rows"])
def test_format_table_prints_the_golden_lines(name):
    c = S.case(name)
    acc = np.array(c["accuracies"])
    assert _svm().format_table("WL1", name, acc[:, 0], acc[:, 1], acc[:, 2]) == c["lines"]
    assert _svm().kernel_name("WL", 1) == "WL1" and _svm().kernel_name("SP", 1) == "SP" and _svm().kernel_name("LWL", 2) == "LWL2" \
        and _svm().kernel_name("SP", 0) == "SP0"


# ------------------------------------------------------------------------------------------------ the composed path end to end
@pytest.mark.parametrize("name", S.names())
def test_composed_path_on_cpu_tensors(name):
    batch = S.solve(name, "cpu", fused=False)
    assert not batch["fused"] and int(batch["status"].max()) == 0
    S.check_case(name, batch)


def test_vote_ties_go_to_the_first_class():
    c = S.case("tri45")
    assert c["vote_ties"] > 0
    votes = np.array([[0.5, -0.5, 0.5], [-1.0, 1.0, -1.0], [0.0, 0.0, 0.0]])        # one vote each; one each; 0 is not positive: 1, 2, 2
    assert _svm()._vote(votes, 3, [(0, 1), (0, 2), (1, 2)]).tolist() == [0, 0, 2]


def test_two_rows_closed_form():
    """K = [[1, 0.5], [0.5, 1]], y = (+1, -1): alpha_1 = alpha_2 = min(C, 2), rho = 0, for all seven C."""
    from dummynode4graphlearning_amd import ops
    K = torch.tensor([[[1.0, 0.5], [0.5, 1.0]]], dtype=torch.float64)
    Cs = _svm().C_GRID
    table = torch.tensor([[0, 2 * i, 2, 1, c] for i, c in enumerate(Cs)], dtype=torch.float64)
    rows = torch.tensor([0, 1] * len(Cs), dtype=torch.int32)
    alpha, rho, iterations, status = ops.svm_smo_composed(K, table, rows, 1e-3)
    assert alpha.view(-1, 2).tolist() == [[min(c, 2.0)] * 2 for c in Cs]
    assert rho.tolist() == [0.0] * len(Cs) and iterations.tolist() == [1] * len(Cs) and status.tolist() == [0] * len(Cs)


# ------------------------------------------------------------------------------------------------ error paths, command line
def test_error_paths():
    svm = _svm()
    K = [torch.eye(10, dtype=torch.float64)]
    classes = np.array([0] * 8 + [1] * 2)
    with pytest.raises(ValueError, match="greater than one; got 1 class"):
        svm.kernel_svm_evaluation(K, classes, list(range(8)), [8], [9], device="cpu")
    with pytest.raises(ValueError, match="square"):
        svm.evaluate_dataset([torch.ones(4, 5)], [0, 1, 0, 1], [0], device="cpu")
    # the identity kernel on a balanced training split decides every other row by rho = 0 alone: never positive, so always the pair's
    # second class; a validation row of the first class is then wrong at every C
    classes = np.array([0, 1, 0, 1, 0, 1, 0, 1, 0, 1])
    with pytest.raises(ValueError, match="no C reaches a validation accuracy above 0"):
        svm.kernel_svm_evaluation(K, classes, list(range(8)), [8], [9], device="cpu")
    from dummynode4graphlearning_amd import ops
    K3 = torch.eye(3, dtype=torch.float64).unsqueeze(0)
    rows = torch.tensor([0, 1, 2], dtype=torch.int32)
    for bad in ([[1, 0, 2, 1, 1.0]], [[0, 2, 2, 1, 1.0]], [[0, 0, 2, 3, 1.0]], [[0, 0, 2, 1, 0.0]], [[0, 0, 0, 0, 1.0]], [[0, 0.5, 2, 1, 1.0]]):
        with pytest.raises(ValueError, match="table"):
            ops.svm_smo_composed(K3, torch.tensor(bad, dtype=torch.float64), rows, 1e-3)
    with pytest.raises(ValueError, match="rows"):
        ops.svm_smo_composed(K3, torch.tensor([[0, 0, 2, 1, 1.0]], dtype=torch.float64), torch.tensor([0, 3], dtype=torch.int32), 1e-3)
    with pytest.raises(ValueError, match="eps"):
        ops.svm_smo_composed(K3, torch.tensor([[0, 0, 2, 1, 1.0]], dtype=torch.float64), rows, 0.0)


def test_command_line_messages_and_table_on_the_cpu(tmp_path, capsys):
    """The toy files of the golden through the command line with --add_origin true on the composed path: missing-file messages as
    seed_svm.py prints them; the table within what the band allows (the GPU test holds the stdout against the golden's lines)."""
    svm = _svm()
    c = S.case("DUMMY_TOYS")
    data, gdir = S.write_files(c, str(tmp_path))
    os.makedirs(os.path.join(data, "EMPTY"))
    with open(os.path.join(data, "EMPTY", "EMPTY_graph_labels.txt"), "w") as f:
        f.write("0\n1\n")
    argv = ["--gram_dir", gdir, "--dataset_dir", data, "--k", "1", "--kernel", "WL", "--n_iters", str(c["n_iters"]), "--add_origin", "true",
            "--device", "cpu", "--seeds"] + [str(s) for s in c["seeds"]] + ["--datasets", "NOWHERE", "EMPTY", "DUMMY_TOYS"]
    assert svm.main(argv) == 0
    out = capsys.readouterr().out.splitlines()
    assert out[0] == "%s and %s are not found." % (os.path.join(data, "NOWHERE", "NOWHERE_graph_labels.txt"),
                                                   os.path.join(data, "NOWHERE", "raw", "NOWHERE_graph_labels.txt"))
    assert out[1] == "Gram matrices for EMPTY are not found."
    assert len(out) == 2 + len(c["lines"])
    assert [ln.split("\t")[:2] for ln in out[2:]] == [ln.split("\t")[:2] for ln in c["lines"]]
    with pytest.raises(ValueError, match="none of the prefixes"):
        svm.origin_dataset("TOYS")
