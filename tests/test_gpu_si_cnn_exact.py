"""Bit-exact parity of the CNN layer's kernels (dn_eseq.hip behind ops.eseq_conv_pool) with the float64 restatement tests/eseq_ref.py,
on the integer operands of tests/cnn_exact_cases.py, whose premise -- fp32 computes every sum of the layer and of its gradients
without rounding -- tests/test_si_cnn_exact_premise.py proves without a GPU.

* the full cross product C in {16, 32, .., 128} x the ten (k, padding) pairs of the predicate x {relu, none}, residual off, and on
  where the layer keeps the length ((3, 1) and (5, 2)): y, gate_out, dx, dW and dbias with np.array_equal, all five kernel tags seen
  and the composed path not.  C / 16 = 2, 3, 5, 6, 7 are the odd splits of conv_tile's four waves; about 3 % of the live outputs tie
  between two slots of the max window at a value that carries a gradient, so "ties go to the first slot" in the forward kernel and
  the slot match of the dconv gather decide bits; a wrong entry cannot hide under a tensor's largest magnitude;
* lens is only a bound: None and "every length L" give the bits of the tight lengths (the dead-tile shortcuts of the forward, the
  input-gradient and the weight-gradient kernels against the full computation);
* leaky_relu (slope 1 / 5.5: not exact) at C in {32, 48, 80, 96, 112} on the inputs and under the bound of tests/test_gpu_si_cnn.py
  (eseq_ref.close, 1e-4 of a tensor's largest magnitude), at the (k, padding) pairs that file's grid leaves out."""
import numpy as np
import pytest
import torch

import cnn_exact_cases as X
from test_gpu_si_cnn import CORNERS, FUSED_TAGS, _check_against_ref, _op_inputs, _run_op, _tags

pytestmark = pytest.mark.gpu
DEV = "cuda"
LEAKY = [(32, (4, 0)), (48, (4, 1)), (80, (5, 0)), (96, (5, 1)), (112, (3, 1))]


def _ops():
    from dummynode4graphlearning_amd import ops
    return ops


def _run(C, k, p, act, residual, lens="tight"):
    d = X.inputs(C, k, p)
    lens = {"tight": d["lens"], "none": None, "L": [X.L] * X.B}[lens]
    (got, _), tags = _tags(lambda: _run_op(np.array(d["x"]), np.array(d["gate"]), lens, np.array(d["W"]), np.array(d["bias"]), p, act,
                                           residual, np.array(d["coef"])))
    assert FUSED_TAGS <= tags and "eseq_layer_composed" not in tags, tags
    return got


def _first_difference(g, w):
    bad = np.argwhere(g != w)
    at = tuple(int(v) for v in bad[0])
    return "%d of %d entries differ, first at %s: got %r, want %r" % (len(bad), w.size, at, float(g[at]), float(w[at]))


@pytest.mark.parametrize("act", X.ACTS)
@pytest.mark.parametrize("kp", X.KP, ids=[X.kp_id(kp) for kp in X.KP])
@pytest.mark.parametrize("C", X.WIDTHS)
def test_layer_equals_the_float64_restatement_bit_for_bit(C, kp, act):
    ops = _ops()
    k, p = kp
    d = X.inputs(C, k, p)
    assert ops.eseq_fused_supported(torch.from_numpy(np.array(d["x"])).to(DEV), torch.from_numpy(np.array(d["W"])).to(DEV), p, act)
    for residual in ((False, True) if kp in X.KEEPS_LENGTH else (False,)):
        got = _run(C, k, p, act, residual)
        want = X.reference(C, k, p, act, residual)
        for g, w, name in zip(got, want, X.NAMES):
            assert g.dtype == np.float32 and g.shape == w.shape, name
            assert np.array_equal(g, w), "C%d k%d p%d %s res=%s %s: %s" % (C, k, p, act, residual, name, _first_difference(g, w))
        assert not got[0][1].any() and not got[2][1].any()                # the sequence of length 0: exact zeros


@pytest.mark.parametrize("case", [(48, 3, 1), (112, 5, 0)], ids=["C48_k3_p1", "C112_k5_p0"])
def test_lens_is_only_a_bound(case):
    """lens=None and every length given as L (no dead tile anywhere) against the tight lengths: the same bits in all five tensors."""
    C, k, p = case
    for act in X.ACTS:
        tight = _run(C, k, p, act, (k, p) in X.KEEPS_LENGTH)
        for loose in ("none", "L"):
            got = _run(C, k, p, act, (k, p) in X.KEEPS_LENGTH, lens=loose)
            for g, w, name in zip(got, tight, X.NAMES):
                assert np.array_equal(g, w), "C%d k%d p%d %s lens=%s %s: %s" % (C, k, p, act, loose, name, _first_difference(g, w))


def test_the_leaky_relu_cases_complete_the_ten_pairs():
    assert set(CORNERS) | {kp for _, kp in LEAKY} == set(X.KP) and len(X.KP) == 10
    assert [C for C, _ in LEAKY] == [32, 48, 80, 96, 112]


@pytest.mark.parametrize("C,kp", LEAKY, ids=["C%d_%s" % (C, X.kp_id(kp)) for C, kp in LEAKY])
def test_leaky_relu_at_the_odd_widths_against_the_float64_restatement(C, kp):
    k, p = kp
    x, gate, lens, W, bias = _op_inputs(C, k, 100 * k + p + C)
    for residual in (True, False):
        (got, _), tags = _tags(lambda: _run_op(x, gate, lens, W, bias, p, "leaky_relu", residual))
        assert FUSED_TAGS <= tags and "eseq_layer_composed" not in tags, tags
        got = _check_against_ref(x, gate, lens, W, bias, p, "leaky_relu", residual, "k%d p%d C%d leaky_relu res=%s" % (k, p, C, residual))
        assert not got[0][9].any()                                        # the all-zero-gate sequence: exact zeros
        assert (got[0] < 0).any()                                         # the negative side of the activation is reached
