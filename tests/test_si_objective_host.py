"""CPU tests of the SI training objective's host side: ops.si_objective_composed, the schedules, SIObjective and the epoch meters of
subgraph_isomorphism/objective.py against the goldens the reference's own train_epoch / evaluate_epoch produced
(tests/golden/si_objective.npz), and the float64 restatement of tests/objective_ref.py against the same goldens.

Bounds (u = 2^-24): a term is a sum of n non-negative addends, |x - golden| <= (n + 8) u golden; an elementwise gradient is a product
of at most five rounded factors, relative 16 u and exact zero where the golden is zero; d pred_c mixes signs, (n + 8) u sum|addends|."""
import numpy as np
import pytest
import torch

import objective_ref as R

META, A, CASES = R.golden()
output_of, weights_of, objective_of, run_case, grads_of, check_against_golden = (R.output_of, R.weights_of, R.objective_of, R.run_case,
                                                                                R.grads_of, R.check_against_golden)
EXACT = sorted(t for t, c in CASES.items() if c["kind"] == "exact")
GENERAL = sorted(t for t, c in CASES.items() if c["kind"] == "general")


@pytest.mark.parametrize("tag", EXACT)
def test_composed_reproduces_the_exact_goldens_bitwise(tag):
    out, loss, terms = run_case(tag)
    assert terms.dtype == torch.float64 and terms.shape == (7,) and loss.dim() == 0 and not terms.requires_grad
    assert np.array_equal(terms.numpy(), A[tag + "/terms"]) and float(loss.detach()) == A[tag + "/terms"][1]
    for k, g in grads_of(tag).items():
        assert np.array_equal(out[k].grad.double().numpy(), g), k


@pytest.mark.parametrize("tag", GENERAL)
def test_composed_reproduces_the_general_goldens(tag):
    out, loss, terms = run_case(tag)
    grads = {k: (None if t.grad is None else t.grad.numpy()) for k, t in out.items() if t is not None and t.dtype != torch.bool}
    check_against_golden(tag, terms.numpy(), grads, "composed")


@pytest.mark.parametrize("tag", EXACT + GENERAL)
def test_restatement_agrees_with_the_goldens(tag):
    case, inp = CASES[tag], R.inputs(A, tag)
    want = R.objective(**R.kwargs_of(inp, case["cfg"], case["is_graph"]))
    g = want["grads"]
    reps = [k for k in R.REP_KEYS if k in inp]
    grads = {"pred_c": g["pred_c"].reshape(-1, 1), "pred_v": g["pred_v"], "pred_e": g["pred_e"]}
    grads.update({k: g["reps"][i] for i, k in enumerate(reps)})
    gold = grads_of(tag)
    if case["kind"] == "exact":
        assert np.array_equal(want["terms"], A[tag + "/terms"])
        assert all(np.array_equal(grads[k], gold[k]) for k in gold)
    else:                 # (d pred_x: an exact sum of two products against a rounded one: check_two_addends; the rest by the bounds above)
        check_against_golden(tag, want["terms"], {k: v for k, v in grads.items() if k in gold and k not in want["abs"]}, "restatement",
                             skip=tuple(want["abs"]))
        for k, mag in want["abs"].items():
            R.check_two_addends(grads[k], gold[k], mag, "restatement %s %s" % (tag, k))


def test_a_fully_masked_row_takes_the_regularisers_gradient():
    """train.py:784 fills pred_v in place outside autograd: a masked entry of a row with negative pred_c gets a gradient."""
    out, _, _ = run_case("exact_MSE")
    inp = R.inputs(A, "exact_MSE")
    row = int(np.flatnonzero(~inp["g_v_mask"].any(1))[0])
    assert inp["pred_c"][row, 0] < 0 and bool((out["pred_v"].grad[row] != 0).all())


def test_schedule_table_is_equal_as_python_floats():
    from dummynode4graphlearning_amd.subgraph_isomorphism import schedule_value
    s = META["schedules"]
    table = A["schedules/table"]
    for i, spec in enumerate(s["specs"]):
        for j, step in enumerate(s["steps"]):
            assert schedule_value(spec, step, s["total_steps"]) == float(table[i, j]), (spec, step)
    assert len({float(x) for x in table[2]}) > 4                                                # (the table moves)


def test_epoch_scalars_and_train_meter_reproduce_the_recorded_epoch():
    from dummynode4graphlearning_amd.subgraph_isomorphism import SITrainMeter
    e = META["epoch"]
    obj, meter, pairs = objective_of(e["cfg"], e["total_steps"]), SITrainMeter(), 0
    for i in range(e["steps"]):
        tag = "epoch/%d" % i
        inp = R.inputs(A, tag)
        step = e["epoch"] * e["steps"] + i
        s = obj.scalars(step)
        assert [s[k] for k in ("neg_pred_slp", "match_loss_w", "match_reg_w", "rep_reg_w")] == A["epoch/scalars"][i].tolist()
        nw, ew = weights_of(inp)
        loss, terms = obj(output_of(inp), torch.from_numpy(inp["counts"]), nw, ew, step=step)
        cfg = dict(e["cfg"], neg_pred_slp=s["neg_pred_slp"], match_loss_w=s["match_loss_w"], match_reg_w=s["match_reg_w"], rep_reg_w=s["rep_reg_w"])
        R.check_terms(terms.numpy(), A[tag + "/terms"], R.objective(**R.kwargs_of(inp, cfg))["terms_n"], tag)
        meter.update(terms, len(inp["counts"]))
        pairs += len(inp["counts"])
    res = meter.result()
    assert list(res) == list(R.TERMS)
    for k, want in zip(("eval", "bp_loss"), A["epoch/avg"]):                                     # sums of three products: a few double roundings
        assert abs(res[k] - want) <= 8 * 2.0 ** -53 * abs(want) + pairs * 64 * R.U * abs(want), (k, res[k], want)
    assert SITrainMeter().result()["bp_loss"] == 0.0


@pytest.mark.parametrize("rid", range(len(META["eval"])))
def test_eval_meter_reproduces_the_recorded_epoch(rid):
    run = META["eval"][rid]
    R.check_eval_result(run, R.eval_meter(run).result())


def test_refusals():
    from dummynode4graphlearning_amd import ops
    from dummynode4graphlearning_amd.subgraph_isomorphism import SIEvalMeter, SIObjective, schedule_value
    with pytest.raises(NotImplementedError, match="AUC"):
        SIObjective(eval_metric="AUC")
    with pytest.raises(NotImplementedError):
        SIObjective(bp_loss="AUC")
    for spec in ("cosine$1$0", "anneal_cosine$1", "anneal_sine$1$0", "cyclical_cosine$a$b", None, "", True):
        with pytest.raises(ValueError):
            schedule_value(spec, 0, 10)
    with pytest.raises(ValueError):
        SIObjective(match_reg_w="linear$0$1")
    out = {k: None for k in R.OUT_KEYS}
    out["pred_c"] = torch.tensor([[1.0], [2.0]])
    meter = SIEvalMeter(4)
    meter.update(out, torch.tensor([1, 2]))
    with pytest.raises(ValueError, match="Only one class"):
        meter.result()
    with pytest.raises(ValueError):
        SIEvalMeter(4).result()
    meter.update(out, torch.tensor([1, 0]))
    assert meter.result()["AUC"] == 0.5
    with pytest.raises(ValueError):
        meter.update(out, torch.tensor([1, 0]))                                                 # beyond the capacity
    with pytest.raises(NotImplementedError):
        ops.si_objective(out["pred_c"], torch.tensor([1.0, 0.0]), "AUC", "MSE", 0.1, 0.1, 0.1, 0.1)
    assert ops.SI_OBJECTIVE_FUSED_DEFAULT in (True, False) and isinstance(ops.objective_fused(True), ops._ThreadSwitch)


def test_inputs_are_unchanged_after_a_call():
    tag = "gen_all_B5"
    inp = R.inputs(A, tag)
    out = output_of(inp)
    nw, ew = weights_of(inp)
    counts = torch.from_numpy(inp["counts"])
    before = {k: t.detach().clone() for k, t in out.items() if t is not None}
    keep = (nw.clone(), ew.clone(), counts.clone())
    assert not inp["g_v_mask"].all() and bool((out["pred_v"].detach()[~out["g_v_mask"]] != 0).all())    # there is something to zero
    loss, _ = objective_of(CASES[tag]["cfg"])(out, counts, nw, ew)
    loss.backward()
    assert all(torch.equal(out[k].detach(), v) for k, v in before.items())
    assert torch.equal(nw, keep[0]) and torch.equal(ew, keep[1]) and torch.equal(counts, keep[2])
