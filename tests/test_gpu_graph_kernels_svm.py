"""GPU tests of the batched SMO kernel (dn_svm.hip through ops.svm_smo and graph_kernels_svm.py) against
tests/golden/graph_kernels_svm.json, which the reference's seed_svm.py wrote on scikit-learn.  tests/svm_cases.py states the checks
and their bounds (KKT in fp64 on the CPU, the measured agreement band, predictions outside it, tables on exact cases).

* every golden case on the fused path, the launches counted by their tag;
* slicing: iters_per_launch in {1, 7, default} gives the same bits (alpha, rho, iteration counts), and so do two runs;
* the 42 solves of the 3-class case's first split in one launch against the same solves launched one by one, bit for bit;
* the two-row closed form; the command line on the toy gram files against the golden's lines.
"""
import numpy as np
import pytest
import torch

import svm_cases as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _ops():
    from dummynode4graphlearning_amd import ops
    return ops


def _svm():
    from dummynode4graphlearning_amd import graph_kernels_svm
    return graph_kernels_svm


@pytest.mark.parametrize("name", S.names())
def test_fused_path_meets_the_golden(name):
    ops = _ops()
    with ops.KernelTimer() as timer:
        batch = S.solve(name, DEV, fused=True)
    tags = timer.summary()
    assert batch["fused"] and tags["svm_smo"][0] >= 1 and int(batch["status"].max()) == 0
    S.check_case(name, batch)


def _state(batch):
    return batch["alpha"].cpu(), batch["rho"].cpu(), batch["iterations"].cpu()


@pytest.mark.parametrize("name", ["bin48", "tri45"])
def test_slicing_does_not_change_a_bit(name):
    want = _state(S.solve(name, DEV, fused=True))
    assert int(want[2].max()) > 7                                            # more than one launch at 7 iterations each
    for ipl in (1, 7, None):
        got = _state(S.solve(name, DEV, fused=True, iters_per_launch=ipl))
        for a, b in zip(got, want):
            assert torch.equal(a, b), (name, ipl)


def test_one_launch_equals_the_solves_one_by_one():
    ops, svm = _ops(), _svm()
    c = S.case("tri45")
    K = S.normalized("tri45").to(DEV)
    table_h, rows_h, _ = svm._solve_plan(np.array(c["classes"]), S.splits(c)[:1], int(K.shape[0]), svm.C_GRID)
    assert table_h.shape[0] == 42
    table, rows = torch.from_numpy(table_h).to(DEV), torch.from_numpy(rows_h).to(DEV)
    with ops.KernelTimer() as timer:
        alpha, rho, iterations, status = ops.svm_smo(K, table, rows, S.EPS, iters_per_launch=1 << 20)
    assert timer.summary()["svm_smo"][0] == 1 and int(status.max()) == 0     # all 42 workgroups in ONE launch, run to the end
    for s in range(42):
        a1, r1, i1, s1 = ops.svm_smo(K, table[s:s + 1].contiguous(), rows, S.EPS, iters_per_launch=1 << 20)
        off, l = int(table_h[s, 1]), int(table_h[s, 2])
        assert torch.equal(a1[off:off + l], alpha[off:off + l]) and torch.equal(r1[0], rho[s]) and torch.equal(i1[0], iterations[s])


def test_two_rows_closed_form():
    """K = [[1, 0.5], [0.5, 1]], y = (+1, -1): alpha_1 = alpha_2 = min(C, 2), rho = 0, for all seven C."""
    ops, Cs = _ops(), _svm().C_GRID
    K = torch.tensor([[[1.0, 0.5], [0.5, 1.0]]], dtype=torch.float64, device=DEV)
    table = torch.tensor([[0, 2 * i, 2, 1, c] for i, c in enumerate(Cs)], dtype=torch.float64, device=DEV)
    rows = torch.tensor([0, 1] * len(Cs), dtype=torch.int32, device=DEV)
    alpha, rho, iterations, status = ops.svm_smo(K, table, rows, 1e-3)
    assert alpha.view(-1, 2).tolist() == [[min(c, 2.0)] * 2 for c in Cs]
    assert rho.tolist() == [0.0] * len(Cs) and iterations.tolist() == [1] * len(Cs) and status.tolist() == [0] * len(Cs)


def test_refusals_before_a_launch():
    ops = _ops()
    K = torch.eye(4, dtype=torch.float64, device=DEV).unsqueeze(0).contiguous()
    rows = torch.tensor([0, 1, 2, 3], dtype=torch.int32, device=DEV)
    table = torch.tensor([[0, 0, 4, 2, 1.0]], dtype=torch.float64, device=DEV)
    with pytest.raises(ValueError, match="rows"):
        ops.svm_smo(K, table, torch.tensor([0, 1, 2, 4], dtype=torch.int32, device=DEV), 1e-3)
    with pytest.raises(ValueError, match="table"):
        ops.svm_smo(K, torch.tensor([[0, 2, 4, 2, 1.0]], dtype=torch.float64, device=DEV), rows, 1e-3)
    with pytest.raises(ValueError, match="eps"):
        ops.svm_smo(K, table, rows, 0.0)
    with pytest.raises(ValueError, match="iters_per_launch"):
        ops.svm_smo(K, table, rows, 1e-3, iters_per_launch=0)
    assert not ops.svm_smo_supported(K, ops.svm_max_rows() + 1) and ops.svm_smo_supported(K, ops.svm_max_rows())
    assert not ops.svm_smo_supported(K.cpu(), 4)


def test_command_line_prints_the_golden_lines(tmp_path, capsys):
    ops, svm = _ops(), _svm()
    c = S.case("DUMMY_TOYS")
    data, gdir = S.write_files(c, str(tmp_path))
    argv = ["--gram_dir", gdir, "--dataset_dir", data, "--k", "1", "--kernel", "WL", "--n_iters", str(c["n_iters"]), "--add_origin", "true",
            "--device", DEV, "--datasets", "DUMMY_TOYS", "--seeds"] + [str(s) for s in c["seeds"]]
    with ops.svm_fused(True), ops.KernelTimer() as timer:
        assert svm.main(argv) == 0
    assert timer.summary()["svm_smo"][0] >= 1
    assert capsys.readouterr().out.splitlines() == c["lines"]
