"""CPU self-tests of the exact operand construction of tests/exact_ref.py (no GPU): before any kernel is held to bit equality, the
operands must make the arithmetic itself exact -- independent of summation order, precision of the accumulator and storage points."""
import numpy as np
import pytest
import torch

import exact_ref as X
from oracle import layers as OL


def _case(seed, H=64, R=8, split=False, **kw):
    rng = np.random.default_rng(seed)
    src, dst, et, nptr, _ = X.si_batch(rng, 10, R, 20, 2.5)
    N = int(nptr[-1])
    p = X.layer_params(rng, H, R, **kw)
    x = X.split_rows(rng, N, H, 2) if split else X.sparse_rows(rng, N, H, 3, 1)
    coef = X.tri_coef(rng, N, H)
    return torch.from_numpy(src), torch.from_numpy(dst), torch.from_numpy(et), N, p, x, coef


def _oracle(x, src, dst, et, p, R, dtype, coef, kw):
    xr = X.leaf(x, dtype=dtype)
    pr = {k: X.leaf(v, dtype=dtype) for k, v in p.items()}
    out = OL.rgin_layer(xr, src, dst, et, pr, num_rels=R, num_bases=kw.get("num_bases", -1), regularizer=kw.get("regularizer", "basis"),
                        num_mlp_layers=kw.get("num_mlp_layers", 2), act="relu")
    out.backward(coef.to(dtype))
    return out.detach(), xr.grad, {k: v.grad for k, v in pr.items()}


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("kw", [{}, dict(regularizer="bdd", num_bases=4), dict(num_bases=3), dict(num_mlp_layers=1)])
def test_fp32_oracle_in_another_order_equals_fp64(split, kw):
    """The oracle in fp32, nodes shuffled and relations renumbered (so every sum runs in another order), equals the oracle in fp64."""
    R = 8
    src, dst, et, N, p, x, coef = _case(3, R=R, split=split, **kw)
    want = _oracle(x, src, dst, et, p, R, torch.float64, coef, kw)
    rng = np.random.default_rng(4)
    perm = torch.from_numpy(rng.permutation(N))                 # new id of node i: inv[i]
    inv = torch.empty_like(perm)
    inv[perm] = torch.arange(N)
    rp = torch.from_numpy(rng.permutation(R))                   # relation r becomes rp[r]
    q = dict(p)
    if kw.get("regularizer") == "bdd":
        w = torch.empty_like(p["weight"])
        w[rp] = p["weight"]
        q["weight"] = w
    elif "w_comp" in p:
        wc = torch.empty_like(p["w_comp"])
        wc[rp] = p["w_comp"]
        q["w_comp"] = wc
    else:
        w = torch.empty_like(p["weight"])
        w[rp] = p["weight"]
        q["weight"] = w
    eperm = torch.from_numpy(rng.permutation(len(src)))
    got = _oracle(x[perm], inv[src][eperm], inv[dst][eperm], rp[et][eperm], q, R, torch.float32, coef[perm], kw)
    assert torch.equal(got[0].double(), want[0][perm])
    assert torch.equal(got[1].double(), want[1][perm])
    for k in p:
        g = got[2][k].double()
        if k == "weight" and "w_comp" not in p:
            g = g[rp]
        if k == "w_comp":
            g = g[rp]
        assert torch.equal(g, want[2][k]), k


def test_per_relation_reference_equals_the_oracle():
    for kw in ({}, dict(regularizer="bdd", num_bases=4), dict(num_bases=3), dict(num_mlp_layers=0), dict(self_loop=False)):
        R = 8
        src, dst, et, N, p, x, coef = _case(5, R=R, **kw)
        rk = {k: v for k, v in kw.items() if k != "self_loop"}
        want = _oracle(x, src, dst, et, p, R, torch.float64, coef, rk)
        xr = X.leaf(x)
        pr = {k: X.leaf(v) for k, v in p.items()}
        out = X.rgin_ref(xr, src, dst, et, pr, R, **rk)
        out.backward(coef)
        assert torch.equal(out.detach(), want[0]) and torch.equal(xr.grad, want[1]), kw
        for k in p:
            assert torch.equal(pr[k].grad, want[2][k]), (kw, k)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_bf16_round_trip_of_every_intermediate_is_the_identity(seed):
    R = 8
    src, dst, et, N, p, x, coef = _case(seed, R=R)
    xr = X.leaf(x)
    pr = {k: X.leaf(v) for k, v in p.items()}
    st = {}
    out = X.rgin_ref(xr, src, dst, et, pr, R, stages=st)
    out.backward(coef)
    b = X.layer_bounds(x, src, dst, et, p, R, coef)
    X.check_premise(b, "bf16")
    ts = [x, out.detach(), xr.grad] + [v.detach() for v in st.values()] + [v.grad for v in st.values() if v.grad is not None]
    ts += [v for v in p.values()]
    for t in ts:
        assert torch.equal(t.to(torch.bfloat16).double(), t)
    for k, v in pr.items():                                     # parameter gradients: fp32 accumulation exact
        assert torch.equal(v.grad.float().double(), v.grad), k


@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("act", ["relu", "leaky_relu"])
def test_absolute_value_bound_dominates_every_intermediate(seed, act):
    R = 8
    src, dst, et, N, p, x, coef = _case(seed, R=R)
    xr = X.leaf(x)
    pr = {k: X.leaf(v) for k, v in p.items()}
    st = {}
    out = X.rgin_ref(xr, src, dst, et, pr, R, act=act, slope=0.25, stages=st)
    out.backward(coef)
    b = X.layer_bounds(x, src, dst, et, p, R, coef)
    for k, v in st.items():
        assert bool((v.detach().abs() <= b[k]).all()), k
        if v.grad is not None:
            assert bool((v.grad.abs() <= b["g:" + k]).all()), k
    assert bool((out.detach().abs() <= b["out"]).all()) and bool((xr.grad.abs() <= b["g:x"]).all())
    for k, v in pr.items():
        assert bool((v.grad.abs() <= b["g:" + k]).all()), k
    # every partial sum of a sum of terms is bounded by the sum of the terms' magnitudes: the per-destination message sums, in any
    # prefix, stay within the bound of h
    e = torch.argsort(dst, stable=True)
    W = p["weight"]
    msg = torch.bmm(x[src[e]].unsqueeze(1), W[et[e]]).squeeze(1)
    pref = torch.zeros(N, x.shape[1], dtype=torch.float64)
    for i in range(len(e)):
        pref[dst[e[i]]] += msg[i]
        assert float(pref[dst[e[i]]].abs().max()) <= float(b["h"][dst[e[i]]].max()) + 1


def test_premise_errors_are_construction_errors():
    rng = np.random.default_rng(0)
    big = X.sparse_rows(rng, 4, 8, nnz=8, max_exp=8)
    assert X.sig_bits(torch.tensor([3.0, 4.0, 0.0, -5.0 * 1024])) == 3
    assert X.sig_bits(torch.tensor([3.25, 0.5])) == 4 and X.sig_bits(torch.tensor([float((1 << 16) + 1)])) == 17
    with pytest.raises(X.PremiseError):
        X.check_premise({"h": big * 16}, "bf16")
    with pytest.raises(X.PremiseError):
        X.check_premise({"h": torch.ones(1)}, "f32", split_operands=[torch.tensor([float((1 << 17) + 1)])])


def test_assert_bits_reports_the_first_wrong_element():
    ref = torch.arange(12, dtype=torch.float64).view(4, 3)
    got = ref.float().clone()
    got[2, 1] += 1
    got[3, 0] -= 1
    with pytest.raises(AssertionError, match=r"2 of 12 elements differ; first at \(2, 1\).*relation 5, graph 9"):
        X.assert_bits(got, ref, "t", rel=[0, 0, 5, 5], graph=[0, 0, 9, 9])
    X.assert_bits(ref.to(torch.bfloat16), ref, "exact")
    # a final bf16 output above 256: the reference rounded once, to nearest even
    X.assert_bits(torch.tensor([256.0, 260.0]).to(torch.bfloat16), torch.tensor([257.0, 259.0], dtype=torch.float64), "rne")


def test_leaky_gradients_are_held_to_their_quantum():
    """Behind two leaky-ReLU masks at slope 0.25 the gradients are multiples of 1/16: a dummy node's summed gradient rows then pass 8
    significant bits long before they pass 256.  Whenever check_premise passes (limits in quanta), every stored stage -- the
    pre-aggregated rows per (node, relation) of both directions included -- round-trips through bf16; dense upstream rows fail it."""
    R, H = 8, 64
    passed = failed = 0
    for seed, rows in ((0, 1.0), (1, 1.0), (2, 0.1), (3, 0.1), (4, 0.1)):
        rng = np.random.default_rng(seed)
        src, dst, et, nptr, _ = (torch.from_numpy(a) for a in X.si_batch(rng, 12, R, 49, 2.1))
        N = int(nptr[-1])
        p = X.layer_params(rng, H, R)
        x = X.sparse_rows(rng, N, H, 3, 0)
        coef = X.tri_coef(rng, N, H)
        coef[torch.from_numpy(rng.random(N) >= rows)] = 0.0
        xr, pr, st = X.leaf(x), {k: X.leaf(v) for k, v in p.items()}, {}
        out = X.rgin_ref(xr, src, dst, et, pr, R, act="leaky_relu", slope=0.25, stages=st)
        out.backward(coef)
        q_f = X.quantum(x, *p.values(), *st.values())
        q_b = X.quantum(coef, *(v.grad for v in st.values() if v.grad is not None))
        try:
            X.check_premise(X.layer_bounds(x, src, dst, et, p, R, coef), "bf16", q_fwd=q_f, q_bwd=q_b)
        except X.PremiseError:
            failed += 1
            continue
        passed += 1
        gh = st["h"].grad
        stored = [out.detach(), xr.grad] + [v.detach() for v in st.values()] + [v.grad for v in st.values() if v.grad is not None]
        stored += [x.new_zeros(N * R, H).index_add(0, dst * R + et, x[src]), gh.new_zeros(N * R, H).index_add(0, src * R + et, gh[dst])]
        for t in stored:
            assert torch.equal(t.to(torch.bfloat16).double(), t)
    assert passed and failed, (passed, failed)
