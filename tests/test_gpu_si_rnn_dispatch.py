"""The template instances and the reverse tiles of dn_eseq_rnn.hip that the grid of tests/test_gpu_si_rnn.py does not launch, on that
file's inputs, reference and bound (torch's own nn.LSTM / nn.GRU / nn.RNN in float64 on the CPU; 1e-4 of each tensor's largest
magnitude):

* Hd = 48 (three waves) at the LSTM and at the tanh cell -- DN_RNN_DISPATCH's <kLstm, 3> and <kTanh, 3>, which no test launched -- and
  at the GRU, unidirectional and bidirectional, residual on and off, on the grid inputs (B = 33, L = 70); with the existing grid
  every one of the twelve (cell, Hd) pairs of the dispatch now has a parametrized id, which test_every_dispatch_instance_runs
  enumerates from the parametrize marks;
* the reverse direction's trip count: a tile of 16 sequences that all have length 0, given to the op as lens[b] = 0 with an all-zero
  gate -- first_step returns L, no step runs and only the zero-fill loops write, forward and backward -- and a tile of 16 sequences
  of length 1 (one step), beside a tile of mixed lengths (B = 48, L = 20, Hd = 32, bidirectional, each cell); each of the two tiles
  alone (B = 16) and with one full-length sequence behind it (B = 17: a second tile with one live row);
* lens is only a bound: lens=None and "every length L" against the tight lengths, y, dx and every parameter gradient bit for bit.
  To the left of a tile's support the extra reverse steps are gated to zero in y, their dP rows are exact zeros (dh = 0 and dy
  gate = 0 there) and the W_hh gradient only gains products with zero, so nothing but the sign of a zero may differ.

torch's own fp32 run of the Hd = 48 cases on the CPU (ops.eseq_rnn_composed) lies at most 1.3e-6 of a tensor's largest magnitude
from the float64 reference (LSTM 1.3e-6, GRU 5.7e-7, tanh 8.7e-7; the reverse-tile batches at most 5.7e-7), so the bound leaves
seventy-fold room for another summation order and the device's expf / tanhf."""
import numpy as np
import pytest
import torch

import test_gpu_si_rnn as G
from test_gpu_si_rnn import CELLS, DEV, FUSED_TAGS, _close_all, _op_inputs, _reference, _run_op, _tags

pytestmark = pytest.mark.gpu
WIDE = [("LSTM", 48), ("GRU", 48), ("RNN", 48)]                   # (the GRU ran at 48 before, in one test of its own: here on the grid)
MIXED = [20, 1, 2, 3, 5, 19, 10, 7, 20, 4, 13, 1, 16, 8, 11, 6]


def _ops():
    from dummynode4graphlearning_amd import ops
    return ops


# ---------------------------------------------------------------------------------------------- Hd = 48
@pytest.mark.parametrize("bi", [False, True], ids=["uni", "bi"])
@pytest.mark.parametrize("cell,Hd", WIDE, ids=["%s-%d" % v for v in WIDE])
def test_op_at_three_waves_against_torch_float64(cell, Hd, bi):
    ops = _ops()
    d = _op_inputs(cell, bi, Hd, 1000 + 7 * Hd + 2 * CELLS.index(cell) + bi)
    assert d["lens"][:10] == G.FIXED_LENS and len(d["lens"]) == 33
    assert ops.eseq_rnn_supported(torch.from_numpy(d["x"]).to(DEV), {n: torch.from_numpy(a).to(DEV) for n, a in d["params"].items()}, cell, bi)
    for residual in (True, False):
        got, tags = _tags(lambda: _run_op(d, residual))
        assert FUSED_TAGS <= tags and "eseq_rnn_composed" not in tags, tags
        _close_all(got, _reference(d, residual, (cell, bi, Hd, "grid")), "%s bi=%s Hd=%d res=%s" % (cell, bi, Hd, residual))
        assert set(got) == {"y", "dx"} | {"d" + n for n in d["params"]}
        assert not got["y"][10].any()                                # the all-zero-gate sequence: exact zeros
        assert not got["y"][2, :69].any() and got["y"][2, 69].any()  # length 1: the pad steps are gated out, the live step is not
        assert got["y"][1].all()                                     # length 0 as an all-ones mask: every position is live
        assert not got["dx"][10].any() and not got["dx"][2, :69].any()


def _marks(fn):
    return {m.args[0]: list(m.args[1]) for m in fn.pytestmark if m.name == "parametrize"}


def test_every_dispatch_instance_runs():
    """ESEQ_RNN_CELLS x ESEQ_RNN_WIDTHS against the parametrized ids of the two op grids: all 12 (cell, Hd) pairs appear."""
    ops = _ops()
    old = _marks(G.test_op_against_torch_float64)
    new = _marks(test_op_at_three_waves_against_torch_float64)
    ran = {(c, h) for c in old["cell"] for h in old["Hd"]} | {(c, h) for c, h in new["cell,Hd"]}
    want = {(c, h) for c in ops.ESEQ_RNN_CELLS for h in ops.ESEQ_RNN_WIDTHS}
    assert len(want) == 12 and ran == want, sorted(want - ran)
    assert set(old["bi"]) == set(new["bi"]) == {False, True}


# ---------------------------------------------------------------------------------------------- reverse tiles
def _batch(cell, lens, seed, L=20):
    """_op_inputs at Hd = 32, bidirectional, with the gates of the length-0 sequences all zero (not all one): lens goes to the op as it is."""
    d = _op_inputs(cell, True, 32, seed, B=len(lens), L=L, lens=list(lens))
    for b, n in enumerate(lens):
        if n == 0:
            d["gate"][b] = 0.0
    if len(lens) >= 16 and lens[0] == L:
        d["gate"][0, [0, 7, L - 1]] = 0.0                            # gate zeros inside the full-length sequence
    return d


def _run_with_lens(d, lens, residual=True):
    """G._run_op with lens handed over untouched (0 and None included)."""
    ops = _ops()
    xt = torch.from_numpy(d["x"]).to(DEV).requires_grad_(True)
    pt = {n: torch.from_numpy(a).to(DEV).requires_grad_(True) for n, a in d["params"].items()}
    with ops.eseq_fused(True):
        y = ops.eseq_rnn(xt, lens, pt, torch.from_numpy(d["gate"]).to(DEV), d["cell"], d["bi"], residual)
    (y * torch.from_numpy(d["coef"]).to(DEV)).sum().backward()
    out = {"y": y.detach().cpu().numpy(), "dx": xt.grad.cpu().numpy()}
    out.update({"d" + n: t.grad.cpu().numpy() for n, t in pt.items()})
    return out


BATCHES = {"B48": MIXED + [0] * 16 + [1] * 16, "B16_len0": [0] * 16, "B17_len0": [0] * 16 + [20], "B16_len1": [1] * 16,
           "B17_len1": [1] * 16 + [20]}


@pytest.mark.parametrize("name", list(BATCHES))
@pytest.mark.parametrize("cell", CELLS)
def test_reverse_tiles_with_no_step_and_with_one_step(cell, name):
    lens = BATCHES[name]
    d = _batch(cell, lens, 300 + 17 * len(lens) + lens[-1] + CELLS.index(cell))
    got, tags = _tags(lambda: _run_with_lens(d, lens))
    assert FUSED_TAGS <= tags and "eseq_rnn_composed" not in tags, tags
    want = _reference(d, True, (cell, name, "reverse-tiles"))
    _close_all(got, want, "%s %s" % (cell, name))
    assert all(np.isfinite(v).all() for v in got.values())
    L = d["x"].shape[1]
    for b, n in enumerate(lens):
        if n == 0:
            assert not got["y"][b].any() and not got["dx"][b].any(), "sequence %d (length 0)" % b
        elif n < L:
            assert not got["y"][b, :L - n].any() and not got["dx"][b, :L - n].any(), "sequence %d left of its support" % b
        if 0 < n < L or (n == L and b > 0):
            assert got["y"][b, L - n:].all()                        # live positions: both directions wrote them
    if max(lens) == 0:                                               # nothing live at all: every gradient is an exact zero
        assert not any(v.any() for v in got.values())


@pytest.mark.parametrize("cell", CELLS)
def test_lens_is_only_a_bound(cell):
    lens = BATCHES["B48"]
    d = _batch(cell, lens, 300 + 17 * len(lens) + lens[-1] + CELLS.index(cell))
    tight = _run_with_lens(d, lens)
    for loose in (None, [d["x"].shape[1]] * len(lens)):
        got = _run_with_lens(d, loose)
        assert set(got) == set(tight)
        for k in tight:
            assert np.array_equal(got[k], tight[k]), "%s lens=%s: %s differs at %d entries" % (
                cell, "None" if loose is None else "L", k, int((got[k] != tight[k]).sum()))
