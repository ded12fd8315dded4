"""CPU self-tests of tests/cnn_exact_cases.py (no GPU): every case of tests/test_gpu_si_cnn_exact.py is built here, by the same
parameters, and held to its premise.

* the magnitudes: every value of the float64 restatement (tests/eseq_ref.py) is an integer, and the same formulas on the operands'
  magnitudes -- a bound of every partial sum in any order -- stay below 2^24, so fp32 computes the layer and its gradients without
  rounding whatever the order of a kernel's sums;
* ops.eseq_conv_pool_composed in fp32 on the CPU equals the restatement with np.array_equal on y, gate_out, dx, dW and dbias: the
  restatement's "ties go to the first slot" is torch's own rule, and the premise holds for a second, independent fp32 implementation;
* the inputs contain ties that matter: live outputs whose window maximum is attained by two slots (without them the tie rule of the
  forward kernel and of the dconv gather would stay untested, as it does on normal inputs);
* the lengths, the gate zeros and the tile counts are the ones the cases are named for.

A premise failure is a failure of these tests; the GPU tests then compare bits on operands proven exact."""
import numpy as np
import pytest
import torch

import cnn_exact_cases as X


def _composed(d, p, act, residual):
    from dummynode4graphlearning_amd import ops
    xt, Wt, bt = (torch.from_numpy(np.array(d[k])).requires_grad_(True) for k in ("x", "W", "bias"))
    y, g2 = ops.eseq_conv_pool_composed(xt, Wt, bt, torch.from_numpy(np.array(d["gate"])), p, act, residual)
    (y * torch.from_numpy(np.array(d["coef"]))).sum().backward()
    assert y.dtype == torch.float32
    return [t.detach().numpy() for t in (y, g2.reshape(y.shape[0], -1), xt.grad, Wt.grad, bt.grad)]


@pytest.mark.parametrize("C", X.WIDTHS)
def test_every_case_is_exact_in_fp32_and_the_composed_path_equals_the_restatement(C):
    for k, p in X.KP:
        for act in X.ACTS:
            for residual in ((False, True) if (k, p) in X.KEEPS_LENGTH else (False,)):
                what = "C%d k%d p%d %s res=%s" % (C, k, p, act, residual)
                want = X.reference(C, k, p, act, residual)
                for w, name in zip(want, X.NAMES):
                    assert w.dtype == np.float64 and np.array_equal(w, np.rint(w)), "%s: %s is not integer valued" % (what, name)
                assert X.magnitude_bound(C, k, p, act, residual) < 2 ** 24, what
                got = _composed(X.inputs(C, k, p), p, act, residual)
                for g, w, name in zip(got, want, X.NAMES):
                    assert g.shape == w.shape and np.array_equal(g, w), "%s: %s differs" % (what, name)
                assert want[0].any() and want[2].any() and want[3].any() and want[4].any(), what


def test_the_inputs_contain_ties_that_carry_a_gradient():
    ties, live = X.tie_count(48, 3, 1, "none")
    assert ties > 0 and live > 0
    assert ties < live // 4                                            # ... and are the exception: the maxima still tell the slots apart
    relu_ties, relu_live = X.tie_count(48, 3, 1, "relu")
    assert relu_live == live and relu_ties >= ties                     # relu adds the ties at 0 (no gradient) to the ones above


def test_a_tie_taken_to_the_last_slot_changes_the_gradients():
    """What the ties are for: the restatement with ">=" in place of ">" (ties to the LAST slot) gives another dx and dW."""
    import eseq_ref as R
    d = X.inputs(48, 3, 1)
    y, g2, saved = R.layer_forward(d["x"], d["gate"], d["W"], d["bias"], 1, "none", False)
    a = X.conv_rows(saved["x0"], d["W"], d["bias"], 1)
    L1, L2 = a.shape[1], y.shape[1]
    win = np.zeros(y.shape, np.int64)
    best = np.full(y.shape, -np.inf)
    for t in range(L2):
        for j in range(3):
            s = t - 1 + j
            if 0 <= s < L1:
                take = a[:, s] >= best[:, t]
                best[:, t] = np.where(take, a[:, s], best[:, t])
                win[:, t] = np.where(take, s, win[:, t])
    assert np.array_equal(best * g2[:, :, None], y)                    # the same forward values ...
    first = R.layer_backward(saved, d["coef"])
    last = R.layer_backward(dict(saved, win=win), d["coef"])
    assert not np.array_equal(first[0], last[0]) and not np.array_equal(first[1], last[1])     # ... other gradients


@pytest.mark.parametrize("kp", X.KP, ids=[X.kp_id(kp) for kp in X.KP])
def test_the_cases_are_the_ones_named(kp):
    k, p = kp
    d = X.inputs(16, k, p)
    gate, lens = d["gate"], d["lens"]
    assert lens == [70, 0, 1, 2, max(k - 1, 1), k, 63, 40] and gate.shape == (X.B, X.L) == (8, 70)
    for b, n in enumerate(lens):
        assert not gate[b, :X.L - n].any()                             # right-aligned: nothing left of the support
    assert not gate[1].any() and gate[2].sum() == 1 and gate[6].sum() == 63
    assert not gate[0, [0, 23, 51, 69]].any() and gate[0].sum() == 66
    assert 12 <= gate[7].sum() <= 36 and not gate[7, :30].any()        # about 60 % of 40 kept
    assert set(np.unique(gate)) == {0.0, 1.0}
    for name, lo, hi in (("x", -3, 3), ("W", -2, 2), ("bias", -4, 4), ("coef", -3, 3)):
        a = d[name]
        assert a.dtype == np.float32 and lo <= a.min() < 0 < a.max() <= hi and np.array_equal(a, np.rint(a)), name
    assert 0.55 < (d["W"] == 0).mean() < 0.65                          # half set to 0, and a fifth of the rest drawn as 0
    L1, L2, step = X.L + 2 * p - k + 1, X.out_len(k, p), 64 - (k - 1)
    assert d["coef"].shape == (8, L2, 16)
    assert -(-L2 // step) == 2 and -(-X.L // 64) == 2 and -(-L1 // 32) == 3                 # output, dgrad and wgrad tiles
    if (k, p) == (5, 0):                                               # the first output tile of the short sequences is dead
        for b in (1, 2, 3):
            first_live = max(X.L - lens[b] - 2 * (k - 1) + 2 * p, 0)
            assert step <= first_live
    assert ((k, p) in X.KEEPS_LENGTH) == (L2 == X.L)
