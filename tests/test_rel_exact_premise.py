"""CPU self-tests of tests/rel_exact_ref.py (no GPU): every operand set of tests/test_gpu_rel_exact.py is built here, by the same case
id, and held to its premise; the numpy restatement of the relation index, the row-table decoder and the float64 references are checked
against naive loops; the RGCN layer restatement is pinned to oracle.layers.rgcn_layer bit for bit.  A premise failure is a failure of
these tests; the GPU tests then compare bits on operands proven exact."""
import numpy as np
import pytest
import torch

import exact_ref as X
import gc_exact_ref as G
import rel_exact_ref as R
from oracle import layers as OL


# ---- A ---------------------------------------------------------------------------------------------------------------------------
def _same_index(a, b, what):
    for k in R.INDEX_TABLES:
        assert np.array_equal(a[k], b[k]), "%s: %s differs" % (what, k)
    assert a["P"] == b["P"] and a["rel_ptr_host"] == b["rel_ptr_host"], what


@pytest.mark.parametrize("name", [k for k, v in R.INDEX_CASES.items() if len(v[0]) <= 600])
def test_index_restatement_equals_the_naive_loops_on_the_small_cases(name):
    src, dst, et, N, Rn = R.INDEX_CASES[name]
    _same_index(R.rel_index_ref(src, dst, et, N, Rn), R.rel_index_naive(src, dst, et, N, Rn), name)


def test_index_restatement_equals_the_naive_loops_on_random_builds():
    rng = np.random.default_rng(5)
    n = 0
    while n < 40:
        src, dst, et, N, Rn = R.sweep_case(rng)
        if len(src) > 400 or N > 120:
            continue
        _same_index(R.rel_index_ref(src, dst, et, N, Rn), R.rel_index_naive(src, dst, et, N, Rn), "random build %d" % n)
        n += 1


def test_index_cases_are_the_ones_named():
    c = R.INDEX_CASES
    ix = {k: R.rel_index_ref(*v) for k, v in c.items()}
    assert ix["E0"]["P"] == 0 and ix["E0"]["rel_ptr_host"] == [0] * 4 and list(ix["E0"]["seg_ptr"]) == [0]
    assert ix["N1-R1-self-loops"]["P"] == 1
    assert ix["one-segment"]["P"] == 1 and len(c["one-segment"][0]) == 300
    assert ix["every-edge-its-own-segment"]["P"] == len(c["every-edge-its-own-segment"][0]) == 200
    rp = ix["empty-relations"]["rel_ptr_host"]
    assert rp[0] == rp[1] and rp[3] == rp[4] and rp[5] == rp[6] and rp[1] < rp[2] < rp[3] < rp[5]
    assert int((c["self-loops"][0] == c["self-loops"][1]).sum()) > 20
    for k, (deg, ptr) in (("ends-without-in-edges", (1, "dptr")), ("ends-without-out-edges", (0, "optr"))):
        cnt = np.diff(ix[k][ptr])
        assert cnt[0] == 0 and cnt[-1] == 0 and cnt[1:-1].sum() > 0 and deg in (0, 1)
    for k, N in (("keys-2^12", 1024), ("keys-2^12+1", 1025), ("keys-2^12-top-only", 1024), ("keys-2^12+1-top-only", 1025)):
        src, dst, et = c[k][:3]
        key = et * N + dst
        assert key.max() == N * 4 - 1 and int((key == key.max()).sum()) >= 3
        assert ("top-only" in k) != bool((key == 0).any())
    assert 1024 * 4 == 2 ** 12 and 1025 * 4 - 1 >= 2 ** 12            # 12 bits hold the largest key of the first, 13 the second's
    rp = ix["table-edges"]["rel_ptr_host"]
    assert [b - a for a, b in zip(rp[:-1], rp[1:])] == R.TABLE_EDGE_SIZES and len(c["table-edges"][0]) > ix["table-edges"]["P"]


@pytest.mark.parametrize("step", R.TABLE_STEPS)
def test_row_table_decoder_accepts_the_restated_tables_and_refuses_broken_ones(step):
    for name, case in R.INDEX_CASES.items():
        ix = R.rel_index_ref(*case)
        M = R.table_rows(ix["P"], case[4], step)
        table, pp = R.row_table_ref(ix["rel_ptr_host"], step, M)
        R.check_row_table(table, ix["rel_ptr_host"], step, pp, name)
    ix = R.rel_index_ref(*R.INDEX_CASES["table-edges"])
    rp = ix["rel_ptr_host"]
    M = R.table_rows(ix["P"], len(rp) - 1, step)
    table, pp = R.row_table_ref(rp, step, M)
    last_full = int(np.flatnonzero(table[:, 2] > table[:, 1])[-1])

    def broken(edit):
        t, q = table.copy(), pp.copy()
        edit(t, q)
        with pytest.raises(AssertionError):
            R.check_row_table(t, rp, step, q)

    def short(t, q): t[last_full, 2] -= 1                               # a chunk one row short  # noqa: E704
    def twice(t, q): t[last_full, 1] -= 1                               # a row in two pieces (and across the boundary)  # noqa: E704
    def wrong_rel(t, q): t[last_full, 0] -= 1                           # noqa: E704
    def long(t, q): t[0, 2] = t[1, 2]; t[1, 1] = t[1, 2]               # two pieces merged: over the step or across relations  # noqa: E704,E702
    def bad_ptr(t, q): q[-2] -= 1                                       # noqa: E704
    for edit in (short, twice, wrong_rel, long, bad_ptr):
        broken(edit)


# ---- B ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", R.agg_params(), ids=R.agg_ids())
def test_agg_case_holds_its_premise(p):
    c = R.agg_case(*p)
    worst = c.premise()
    assert max(worst.values()) < 2 ** 24
    sizes = [b - a for a, b in zip(c.ix["rel_ptr_host"][:-1], c.ix["rel_ptr_host"][1:])]
    edge = (4095, 4096, 4097) if c.square else (1023, 1024, 1025)
    assert set(edge) <= set(sizes) and 0 in sizes
    assert c.split == (p[2] == "f32s" and c.square)


def test_agg_reference_equals_a_naive_loop():
    rng = np.random.default_rng(2)
    N, Rn, E = 12, 3, 60
    src, dst, et = (torch.from_numpy(rng.integers(0, n, E)) for n in (N, N, Rn))
    x, W, s = G.int_rows(rng, N, 5, G.F32), torch.stack([X.signed_weight(rng, 5, 4, 2) for _ in range(Rn)]), G.scales(rng, E)
    for sc in (None, s):
        want = R.agg_naive(x, W, src, dst, et, N, sc)
        assert torch.equal(R.agg_ref(x, W, src, dst, et, N, None if sc is None else sc.view(-1, 1)), want)


def test_a_misplaced_edge_scale_changes_the_reference():
    """What the scaled cases are for: the scales permuted by the other pass's order (operm forward, perm1 backward) change bits."""
    c = R.agg_case(16, 16, "f32x", True)
    src, dst, et = (torch.from_numpy(a) for a in (c.src, c.dst, c.et))
    perm1, operm = torch.from_numpy(c.ix["perm1"]), torch.from_numpy(c.ix["operm"])
    wrong = torch.empty_like(c.scale)
    wrong[perm1] = c.scale[operm]                                   # position i of the (relation, destination) order gets scale[operm[i]]
    assert not torch.equal(R.agg_ref(c.x, c.W, src, dst, et, c.N, wrong.view(-1, 1)), c.out)


# ---- C ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", R.conv_params(), ids=[R.conv_id(p) for p in R.conv_params()])
def test_conv_case_holds_its_premise(p):
    R.conv_case(*p).premise()


def test_conv_reference_equals_the_oracle():
    c = R.conv_case(7, 32, "mean", True, True, "f32")
    src, dst, et = (torch.from_numpy(a) for a in (c.src, c.dst, c.et))
    for aggr in ("mean", "add"):
        a = R.rgcn_conv_ref(c.x, src, dst, et, c.p["weight"], c.p["root"], c.p["bias"], aggr)
        assert torch.equal(a, OL.rgcn_conv(c.x, src, dst, et, c.p["weight"], c.p["root"], c.p["bias"], aggr))


@pytest.mark.parametrize("H,dt", [(32, "f32"), (32, "bf16"), (64, "f32"), (64, "bf16")])
def test_mean_case_holds_its_premise(H, dt):
    R.MeanCase(H, dt).premise()


# ---- D ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.LAYER_CASES))
def test_layer_case_holds_its_premise(name):
    c = R.layer_case(name)
    c.premise()
    n = c.norms
    for k in ("in_norm", "out_norm", "edge_in", "edge_both"):          # powers of two, exact in fp32 and in bf16, square roots included
        for t in (n[k], n[k].sqrt())[:2 if k.endswith("_norm") else 1]:
            assert torch.equal(t.to(torch.bfloat16).double(), t), (name, k)


@pytest.mark.parametrize("edge_norm", ["none", "in", "both"])
@pytest.mark.parametrize("self_loop", [True, False])
@pytest.mark.parametrize("reg", [("basis", -1), ("basis", 2), ("bdd", 4)])
@pytest.mark.parametrize("shape", [(32, 32, "f32"), (48, 80, "bf16")], ids=["32x32", "48x80"])
def test_layer_restatement_is_pinned_to_the_oracle(edge_norm, self_loop, reg, shape):
    """rgcn_ref equals oracle.layers.rgcn_layer bit for bit: output and every gradient.  rgcn_ref takes h through the fused factorisation
    (sum + self loop) s_in, the oracle through the per-edge norm and the normed self-loop term: this pin is what makes it independent
    of the code under test.  Two small shapes only (a square and a non-square width; the oracle gathers an [E, in, out] weight
    tensor) -- the restatement has no width-dependent branch."""
    c = R.LayerCase(shape[0], shape[1], shape[2], edge_norm, self_loop, reg[0], reg[1], seed=1)
    xr, pr = X.leaf(c.x), {k: X.leaf(v) for k, v in c.p.items()}
    out = OL.rgcn_layer(xr, c.srct, c.dstt, c.ett, pr, regularizer=reg[0], num_rels=c.R, num_bases=reg[1], edge_norm=edge_norm, act="relu")
    out.backward(c.coef)
    assert torch.equal(out.detach(), c.ref[0]) and torch.equal(xr.grad, c.ref[1])
    for k in pr:
        assert torch.equal(pr[k].grad, c.ref[2][k]), k


@pytest.mark.parametrize("name", list(R.DEGREE_CASES))
@pytest.mark.parametrize("self_loop", [True, False])
def test_norm_reference_equals_the_oracle(name, self_loop):
    src, dst, N = R.DEGREE_CASES[name]
    n = R.norms_ref(src, dst, N, self_loop)
    s, d = torch.from_numpy(src), torch.from_numpy(dst)
    inn, outn, en = OL.rgcn_norms(s, d, N, "both", self_loop)
    assert torch.equal(n["in_norm"].float(), inn.view(-1)) and torch.equal(n["out_norm"].float(), outn.view(-1))
    assert torch.equal(n["edge_in"].float(), OL.rgcn_norms(s, d, N, "in", self_loop)[2].view(-1))
    if name == "powers-of-four":
        assert torch.equal(n["edge_both"].float(), en.view(-1))
    assert (n["in_deg"] == 0).any() or name == "E0" and N == 7
    if name == "hub-5000":
        assert n["in_deg"][0] == 5000
