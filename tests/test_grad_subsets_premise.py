"""CPU self-tests of tests/grad_subset_ref.py (no GPU): every case of tests/test_gpu_grad_subsets.py is built here, by the same
constructor and arguments, and held to its premise; each restatement is checked against a naive per-edge / per-row Python loop on one
small case; and the None pattern the restatement reports for a `requires_grad` pattern is torch.autograd's own.  A premise failure is
a failure of these tests; the GPU tests then compare bits on operands proven exact."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import exact_ref as X
import grad_subset_ref as S

CASES = S.all_cases()


def test_the_reference_module_loads_no_hip_library():
    """(in a fresh interpreter: this process may have imported the package for another test)"""
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); import grad_subset_ref; "
            "bad = [m for m in sys.modules if m.startswith('dummynode4graphlearning_amd')]; assert not bad, bad")
    here = os.path.dirname(os.path.abspath(__file__))
    subprocess.check_call([sys.executable, "-c", code % (os.path.dirname(here), here)])


@pytest.mark.parametrize("cid,make,args", CASES, ids=[c[0] for c in CASES])
def test_premise_holds(cid, make, args):
    make(*args).premise()


def test_a_broken_premise_is_reported():
    c = S.MlpCase(33, 64, "bf16", 1, True, 0.0, True, seed=9)
    c.ins["x"] = c.ins["x"] * 300.0                           # rows over 256 quanta
    with pytest.raises(X.PremiseError):
        c.premise()
    c = S.MlpCase(33, 64, "f32s", 1, True, 0.0, True, seed=9)
    c.ins["w0"] = c.ins["w0"] * 257.0                         # a narrow operand of nine significant bits
    with pytest.raises(X.PremiseError):
        c.premise()


def _subsets_of(cid, c):
    if cid.startswith("dmp_edge"):
        subs = S.subsets(c.names, "singles")
        assert len(subs) == 11
        return subs
    if cid.startswith(("relu_mlp", "layer")):
        return S.subsets(c.names, "first")
    return S.subsets(c.names)


# one case of every operator (the small ones: the loops below are per edge and per row)
PATTERN_CASES = [c for c in CASES if c[0] in (
    "linear_act-33-64-bf16-True-True", "relu_mlp-3-64-bf16-0.25-33", "conv-64-bf16-True", "neighbor_sum-5-bf16-1", "rel_agg-5-7-bf16-True",
    "linear_any-300-5-128-bf16", "si_embed-77-20-bf16", "dual_agg-1-above-16-bf16", "dual_agg-2-below-16-f32", "dmp_edge-above-64-bf16",
    "typed-typed-two_graphs-f32", "typed-expand-two_graphs-f32", "typed-reduce-two_graphs-f32", "layer-small-64-bf16-8", "batchnorm-64-64-f32")]


def test_every_operator_has_a_pattern_case():
    assert len(PATTERN_CASES) == 15


@pytest.mark.parametrize("cid,make,args", PATTERN_CASES, ids=[c[0] for c in PATTERN_CASES])
def test_none_pattern_is_autograds_own_and_subset_gradients_are_the_full_ones(cid, make, args):
    c = make(*args)
    full_out, full = c.run()
    assert all(v is not None for v in full.values())
    for sub in _subsets_of(cid, c):
        out, got = c.run(sub)
        assert {k: v is None for k, v in got.items()} == c.none_pattern(sub) == {k: k not in sub for k in c.names}, (cid, sub)
        assert all(torch.equal(a, b) for a, b in zip(out, full_out))
        for k in sub:
            assert torch.equal(got[k], full[k]), (cid, sub, k)         # a gradient does not depend on who else asks for one
    if len(c.coefs) == 2:                                           # one output left out of the loss
        for used in ((0,), (1,)):
            _, got = c.run(used=used)
            assert {k: v is None for k, v in got.items()} == c.none_pattern(c.names, used) == dict.fromkeys(c.names, False)


def test_naive_loops_agree_with_the_restatements():
    eq = lambda a, b, what: (_ for _ in ()).throw(AssertionError(what)) if not torch.equal(a, b) else None  # noqa: E731
    c = S.relu_mlp_case(3, 64, "bf16", 0.25, 33)
    eq(S.mlp_naive(c), c.run()[0][0], "relu_mlp")
    c = S.linear_act_case(33, 64, "bf16", False, True)
    eq(S.mlp_naive(c), c.run()[0][0], "linear_act")
    c = S.conv_case(64, "bf16", True)
    eq(S.conv_naive(c), c.run()[0][0], "conv")
    c = S.neighbor_sum_case(5, "bf16", 1)
    out, g = c.run()
    eq(S.neighbor_sum_naive(c), out[0], "neighbor_sum")
    eq(S.edge_dot_ref(c), g["edge_scale"], "edge_dot")
    c = S.si_embed_case(77, 20, "bf16")
    eq(S.si_embed_naive(c), c.run()[0][0], "si_embed")
    for m in (S.DUAL_SUB, S.DUAL_MULT):
        c = S.dual_agg_case(m, "above", 16, "bf16")
        for a, b in zip(S.dual_agg_naive(c), c.run()[0]):
            eq(a, b, "dual_agg %d" % m)
    c = S.dmp_edge_case("above", 64, "bf16")
    eq(S.dmp_edge_naive(c), c.run()[0][0], "dmp_edge_update")
    for kind in ("typed", "expand", "reduce"):
        for graph in ("two_graphs", "zoo"):
            c = S.typed_case(kind, graph, "f32")
            eq(S.typed_naive(c), c.run()[0][0], "%s %s" % (kind, graph))
    c = S.linear_any_case(300, 5, 128, "bf16")
    eq(c.ins["x"] @ c.ins["weight"].t() + c.ins["bias"], c.run()[0][0], "linear_any")
    c = S.batchnorm_case(64, 64, "f32")
    mean, var = c.stats()
    want = (c.ins["x"] - mean) / torch.sqrt(var + c.EPS) * c.ins["weight"] + c.ins["bias"]
    assert float((want - c.run()[0][0]).abs().max()) < 1e-12


def test_pair_rows_restates_the_grouping_of_the_pair_index():
    """rows = the non-empty (destination, edge type) pairs grouped by edge type (stable: by destination inside a type)"""
    for graph in S.HGT_GRAPHS:
        N, src, dst, et = S.HGT_GRAPHS[graph](4)
        rd, rr = S.pair_rows(dst, et, 4)
        pairs = sorted(set(zip(et.tolist(), dst.tolist())))
        assert [(int(b), int(a)) for a, b in zip(rd, rr)] == pairs
    N, src, dst, et = S.zoo(4)
    assert np.bincount(dst, minlength=N)[5] >= 300


def test_relu_bwd_cases_are_exact():
    for n in S.RELU_BWD_NUMEL:
        for slope in (0.0, 0.25):
            for mode in ("bf16", "f32"):
                g, y, want = S.relu_bwd_case(n, slope, mode)
                assert g.numel() == n and torch.equal(want, torch.where(y > 0, g, slope * g))


def test_graphs_are_the_ones_named():
    src, dst, et = S.conv_graph(True)
    assert len(set(dst[et == 1])) == 1 and len(set(src[et == 2])) == 1 and len(set(dst[et == 0])) > 50
    src, dst, et = S.conv_graph(False)
    assert all(len(set(dst[et == r])) > 30 and len(set(src[et == r])) > 30 for r in range(3))
    for kind in ("below", "above"):
        u, v, rev = S.dual_graph(kind)
        assert np.bincount(v)[0] == S.HUB_SPLIT + (kind == "above")
