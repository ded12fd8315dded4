"""The two-launch backward of the bf16 two-layer MLP at H = 256 (dn_mlp_bwd_fused_bf16 per layer) against the three launches it
replaces (DN_MLP_BWD_FUSED=0: weight gradient 2, input-gradient chain, weight gradient 1): gw1, gw2, gb1, gb2 and g0 bit for bit,
on random operands (any change of tile order, k-slot, column-sum partition or rounding point shows), at the row counts where the
kernel's paths change; one case on integer operands against float64 (tests/exact_ref.py); the fused path twice, bitwise."""
from contextlib import contextmanager
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import exact_ref as X

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H = 256
SLOPES = (0.0, 1.0 / 5.5)


@contextmanager
def fused(on):
    from dummynode4graphlearning_amd import ops
    old = ops.MLP_BWD_FUSED_ENABLED, ops.MLP_BWD_FUSED_MIN_ROWS
    ops.MLP_BWD_FUSED_ENABLED, ops.MLP_BWD_FUSED_MIN_ROWS = on, 0          # (the default keeps small batches on the three launches)
    try:
        yield
    finally:
        ops.MLP_BWD_FUSED_ENABLED, ops.MLP_BWD_FUSED_MIN_ROWS = old


def _operands(n, seed):
    gen = torch.Generator().manual_seed(seed)
    r = lambda *s, scale=1.0: (torch.randn(*s, generator=gen) * scale).to(torch.bfloat16).to(DEV)   # noqa: E731
    return dict(x=r(n, H), w1=r(H, H, scale=1 / 16), b1=r(H, scale=0.5), w2=r(H, H, scale=1 / 16), b2=r(H, scale=0.5), g=r(n, H))


def _backward(op, slope, bias, need_x, on):
    """(tags, gw1, gw2, gb1, gb2, g0) of relu_mlp's backward with the fused launches on / off."""
    from dummynode4graphlearning_amd import ops
    x = op["x"].clone().requires_grad_(need_x)
    p = {k: op[k].clone().requires_grad_(True) for k in ("w1", "b1", "w2", "b2")}
    lins = [SimpleNamespace(weight=p["w1"], bias=p["b1"] if bias else None), SimpleNamespace(weight=p["w2"], bias=p["b2"] if bias else None)]
    timer = ops.KernelTimer()
    with fused(on):
        y = ops.relu_mlp(x, lins, slope=slope)
        with timer:
            y.backward(op["g"])
    tags = [r[0] for r in timer.records]
    return tags, p["w1"].grad, p["w2"].grad, p["b1"].grad, p["b2"].grad, x.grad


def _compare(n, seed):
    op = _operands(n, seed)
    for slope in SLOPES:
        for bias in (True, False):
            for need_x in (True, False):
                ref = _backward(op, slope, bias, need_x, False)
                got = _backward(op, slope, bias, need_x, True)
                what = "rows=%d slope=%g bias=%s input_grad=%s: " % (n, slope, bias, need_x)
                assert "mlp_bwd_fused" not in ref[0] and ref[0].count("rows_wgrad") == 2 and ref[0].count("rows_chain2") == 1, ref[0]
                assert got[0].count("mlp_bwd_fused") == (2 if need_x else 1) and "rows_chain2" not in got[0], got[0]
                assert got[0].count("rows_wgrad") == (0 if need_x else 1), got[0]
                for name, a, b in zip(("gw1", "gw2", "gb1", "gb2", "g0"), got[1:], ref[1:]):
                    assert (a is None) == (b is None), what + name
                    if a is not None:
                        assert a.dtype == b.dtype and a.shape == b.shape, what + name
                        assert torch.equal(a.view(torch.int16), b.view(torch.int16)), "%s%s differs in %d elements" % (
                            what, name, int((a.view(torch.int16) != b.view(torch.int16)).sum()))


def _boundary():
    """First chunk boundary of the dense table of a few hundred rows, read from the table."""
    from dummynode4graphlearning_amd import ops
    chunks, _, n = ops._dense_table(300, torch.device(DEV))[1]
    assert n >= 2
    return int(chunks[0, 2])


@pytest.mark.parametrize("rows", [1, 31, 32, 33, 95, "boundary-1", "boundary+1"])
def test_fused_backward_matches_three_launches(rows):
    if isinstance(rows, str):
        rows = _boundary() + (1 if rows.endswith("+1") else -1)
    _compare(rows, 100 + rows)


def test_more_chunks_than_one_round_of_workgroups():
    """257 chunks of the minimum size (128 rows) + a ragged tail: more workgroups than CUs, so a second round starts while the
    first is running.  At the launch level, on one chunk table for both sides (the MLP's own table would hold 256 chunks of 192)."""
    from dummynode4graphlearning_amd import ops
    n = 128 * 257 + 5
    table = ops.make_row_chunks([0, n], DEV, chunk_rows=128)
    assert table[2] == 258 > 256
    op = _operands(n, 7)
    with torch.no_grad():
        h1, _, bits1, bits2 = ops.rows_chain2(op["x"], op["w1"], op["b1"], True, op["w2"], op["b2"], True, want_bits=True)
        for slope in SLOPES:
            gw2r, gb2r = ops.rows_wgrad(op["g"], h1, table, 1, colsum_of=1, mask_a_bits=bits2, colsum_lp=True, slope=slope)
            g1r, g0r = ops.rows_chain2(op["g"], op["w2"], None, False, op["w1"], None, False, mask0_bits=bits2, mask1_bits=bits1,
                                       w_kn=(True, True), slope=slope)
            gw1r, gb1r = ops.rows_wgrad(g1r, op["x"], table, 1, colsum_of=1, colsum_lp=True)
            gw2, gb2, g1 = ops.mlp_bwd_fused(op["g"], h1, op["w2"], table, mask_in_bits=bits2, mask_out_bits=bits1, slope=slope)
            gw1, gb1, g0 = ops.mlp_bwd_fused(g1, op["x"], op["w1"], table, slope=slope)
            for name, a, b in (("gw2", gw2, gw2r[0]), ("gb2", gb2, gb2r[0]), ("g1", g1, g1r), ("gw1", gw1, gw1r[0]), ("gb1", gb1, gb1r[0]),
                               ("g0", g0, g0r)):
                assert a.dtype == b.dtype and a.shape == b.shape, name
                assert torch.equal(a.view(torch.int16), b.view(torch.int16)), "slope=%g: %s differs" % (slope, name)


def test_fused_backward_exact_on_integer_operands():
    """Integer rows, signed-permutation weights, small-integer biases, gradients in {-1, 0, 1}: every sum is exact whatever its
    order, so all five results equal the float64 reference rounded once to bf16.  Three chunks, a ragged last tile."""
    from dummynode4graphlearning_amd import ops
    rng = np.random.default_rng(71)
    n = 2 * _boundary() + 33
    x = X.sparse_rows(rng, n, H, nnz=2, max_exp=1)
    w1, w2 = X.signed_weight(rng, H, H, 1), X.signed_weight(rng, H, H, 1)
    b1, b2 = X.small_ints(rng, H), X.small_ints(rng, H)
    g = X.tri_coef(rng, n, H)
    h1_bound = X.linear_bounds(x, w1, b1, g.abs() @ w2.abs())
    X.check_premise(h1_bound, "bf16")
    X.check_premise(X.linear_bounds(h1_bound["y"], w2, b2, g), "bf16")
    xr, w1r, b1r, w2r, b2r = (X.leaf(t) for t in (x, w1, b1, w2, b2))
    lin = torch.nn.functional.linear
    torch.relu(lin(torch.relu(lin(xr, w1r, b1r)), w2r, b2r)).backward(g)
    bf = lambda t: t.to(DEV, torch.bfloat16)   # noqa: E731
    op = dict(x=bf(x), w1=bf(w1), b1=bf(b1), w2=bf(w2), b2=bf(b2), g=bf(g))
    tags, gw1, gw2, gb1, gb2, g0 = _backward(op, 0.0, True, True, True)
    assert tags.count("mlp_bwd_fused") == 2, tags
    assert ops._dense_table(n, torch.device(DEV))[1][2] == 3
    X.assert_bits(gw2, w2r.grad, "weight gradient 2")
    X.assert_bits(gb2, b2r.grad, "bias gradient 2")
    X.assert_bits(gw1, w1r.grad, "weight gradient 1")
    X.assert_bits(gb1, b1r.grad, "bias gradient 1")
    X.assert_bits(g0, xr.grad, "input gradient")


def test_fused_backward_is_repeatable():
    op = _operands(3 * _boundary() + 17, 5)
    a = _backward(op, SLOPES[1], True, True, True)
    b = _backward(op, SLOPES[1], True, True, True)
    assert a[0].count("mlp_bwd_fused") == 2
    for u, v in zip(a[1:], b[1:]):
        assert torch.equal(u.view(torch.int16), v.view(torch.int16))


def test_default_threshold_keeps_small_batches_on_three_launches():
    """ops.MLP_BWD_FUSED_MIN_ROWS: below it the backward is the three launches, from it on the two fused ones."""
    from dummynode4graphlearning_amd import ops
    assert ops.MLP_BWD_FUSED_ENABLED and ops.MLP_BWD_FUSED_MIN_ROWS > 300
    op = _operands(300, 9)
    x = op["x"].clone().requires_grad_(True)
    lins = [SimpleNamespace(weight=op[w].clone().requires_grad_(True), bias=None) for w in ("w1", "w2")]
    old = ops.MLP_BWD_FUSED_MIN_ROWS
    try:
        for min_rows, want in ((old, 0), (301, 0), (300, 2)):
            ops.MLP_BWD_FUSED_MIN_ROWS = min_rows
            timer = ops.KernelTimer()
            y = ops.relu_mlp(x, lins)
            with timer:
                y.backward(op["g"])
            tags = [r[0] for r in timer.records]
            assert tags.count("mlp_bwd_fused") == want and tags.count("rows_wgrad") == 2 - want, (min_rows, tags)
    finally:
        ops.MLP_BWD_FUSED_MIN_ROWS = old
