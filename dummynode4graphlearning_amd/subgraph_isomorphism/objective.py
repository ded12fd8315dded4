"""The SI training objective, its scalar schedules and the epoch meters: what subgraph_isomorphism/train.py computes between the
model's forward and `backward()` (train.py:648-751, :776-828) and what evaluate_epoch reports (train.py:1101-1173), on top of
ops.si_objective / ops.si_eval_errors (dn_objective.hip).  The loops themselves, gradient clipping, the optimizer, LR schedulers, the
per-step AUC and the ragged masked_select copies of evaluate_results are out of scope.

One deviation from the reference, on purpose: the model's OutputDict and the weight tensors are left as they were.  The reference
zeroes their masked entries in place (train.py:783-784, :794-795); the values and gradients computed here are the ones that gives.
"""
import math

import torch

from .. import ops

EPS = 1e-8                 # constants.py:7: the epoch averages divide by EPS + the number of pairs
NUM_CYCLES = 2             # constants.py:39
_PI = 3.141592653589793
_SHAPES = ("linear", "cosine")
_FLAT = ("none", "constant")


def _phase(step, first, last, cycles):
    return float(cycles * (step - first)) / max(1, last - first) % 1


def anneal_fn(fn, current_step, num_init_steps=600, num_anneal_steps=10000, num_cycles=NUM_CYCLES, value1=0.0, value2=1.0):
    """utils/anneal.py: value1 -> value2 over the first half of each of num_cycles cycles of [num_init_steps, num_anneal_steps], value2
    over the second half and behind the last step; below num_init_steps one warm-up cycle of twice that length from value2 to value1."""
    if current_step < num_init_steps:
        return anneal_fn(fn, current_step, 0, num_init_steps * 2, 1, value2, value1)
    if current_step > num_anneal_steps or not fn or fn in _FLAT:
        return value2
    if fn not in _SHAPES:
        raise NotImplementedError(fn)
    t = _phase(current_step, num_init_steps, num_anneal_steps, num_cycles)
    if not t < 0.5:
        return value2
    if fn == "linear":
        return float(value1 + (value2 - value1) * t * 2)
    return float(value1 + (value2 - value1) * (1 - math.cos(_PI * t * 2)) / 2)


def cyclical_fn(fn, current_step, num_init_steps=600, num_cyclical_steps=10000, num_cycles=NUM_CYCLES, value1=0.0, value2=1.0):
    """utils/cyclical.py: value1 -> value2 -> value1 in each of num_cycles cycles (a triangle or a cosine wave); the warm-up and the
    steps behind the last one as anneal_fn."""
    if current_step < num_init_steps:
        return cyclical_fn(fn, current_step, 0, num_init_steps * 2, 1, value2, value1)
    if current_step > num_cyclical_steps or not fn or fn in _FLAT:
        return value2
    if fn not in _SHAPES:
        raise NotImplementedError(fn)
    t = _phase(current_step, num_init_steps, num_cyclical_steps, num_cycles)
    if fn == "cosine":
        return float(value1 + (value2 - value1) * (1 - math.cos(_PI * t * 2)) / 2)
    if t < 0.5:
        return float(value1 + (value2 - value1) * (t * 2))
    return float(value2 + (value1 - value2) * (t * 2 - 1))


def schedule_value(spec, step, total_steps):
    """The value of one of the reference's str2value settings at a step, as train.py:648-751 reads it: a number is itself;
    "anneal_<fn>$a$b" and "cyclical_<fn>$a$b" run anneal_fn / cyclical_fn from a to b over total_steps with no warm-up and NUM_CYCLES
    cycles.  Anything else raises ValueError."""
    if isinstance(spec, bool):
        raise ValueError("not a schedule: %r" % (spec,))
    if isinstance(spec, (int, float)):
        return float(spec)
    if not isinstance(spec, str):
        raise ValueError("not a schedule: %r" % (spec,))
    for prefix, fn in (("anneal_", anneal_fn), ("cyclical_", cyclical_fn)):
        if spec.startswith(prefix):
            parts = spec.rsplit("$", 3)
            if len(parts) != 3:
                raise ValueError("a schedule reads %s<fn>$a$b (got %r)" % (prefix, spec))
            shape = parts[0][len(prefix):]
            if shape and shape not in _SHAPES + _FLAT:
                raise ValueError("unknown schedule shape %r in %r" % (shape, spec))
            return fn(shape, step, 0, total_steps, NUM_CYCLES, float(parts[1]), float(parts[2]))
    raise ValueError("not a schedule: %r" % (spec,))


def _refined(model, name, weights):
    weights = weights.float()
    return weights if model is None else getattr(model, name)(weights)


class SIObjective:
    """The objective of one training step.  obj(output, counts, node_weights, edge_weights, step, model, is_graph) -> (loss, terms):
    loss to call backward on, terms [7] float64 on the device in the order ops.SI_OBJECTIVE_TERMS (what train.py:815-821 reads with
    seven .item() calls; feed them to SITrainMeter).  The four scalars are schedule_value specs, evaluated at `step`."""

    def __init__(self, bp_loss="MSE", eval_metric="MSE", neg_pred_slp="anneal_cosine$1.0$0.01", match_loss_w=1.0,
                 match_reg_w="anneal_cosine$0.01$0.0", rep_reg_w=1e-5, total_steps=1):
        if bp_loss not in ops.SI_OBJECTIVE_CRITERIA:
            raise NotImplementedError("bp_loss %r (MAE, MSE or SMSE)" % (bp_loss,))
        if eval_metric == "AUC":
            raise NotImplementedError("eval_metric AUC per step: the reference sorts the batch on the host there; the epoch AUC is "
                                      "SIEvalMeter.result()['AUC']")
        if eval_metric not in ops.SI_OBJECTIVE_CRITERIA:
            raise NotImplementedError("eval_metric %r (MAE, MSE or SMSE)" % (eval_metric,))
        self.bp_loss, self.eval_metric = bp_loss, eval_metric
        self.specs = {"neg_pred_slp": neg_pred_slp, "match_loss_w": match_loss_w, "match_reg_w": match_reg_w, "rep_reg_w": rep_reg_w}
        self.total_steps = int(total_steps)
        for spec in self.specs.values():
            schedule_value(spec, 0, self.total_steps)

    def scalars(self, step):
        """{neg_pred_slp, match_loss_w, match_reg_w, rep_reg_w} at a step."""
        return {k: schedule_value(v, step, self.total_steps) for k, v in self.specs.items()}

    def __call__(self, output, counts, node_weights=None, edge_weights=None, step=0, model=None, is_graph=True):
        s = self.scalars(step)
        side = {"pred_v": None, "v_mask": None, "v_target": None, "pred_e": None, "e_mask": None, "e_target": None}
        if node_weights is not None and output["pred_v"] is not None and is_graph:
            side.update(pred_v=output["pred_v"], v_mask=output["g_v_mask"], v_target=_refined(model, "refine_node_weights", node_weights))
        if edge_weights is not None and output["pred_e"] is not None:
            side.update(pred_e=output["pred_e"], e_mask=output["g_e_mask"], e_target=_refined(model, "refine_edge_weights", edge_weights))
        reps = tuple(output[k] for k in ("p_v_rep", "p_e_rep", "g_v_rep", "g_e_rep") if output[k] is not None)
        return ops.si_objective(output["pred_c"], counts.float(), self.bp_loss, self.eval_metric, s["neg_pred_slp"], s["rep_reg_w"],
                                s["match_loss_w"], s["match_reg_w"], reps=reps, **side)


class SITrainMeter:
    """The epoch sums of train_epoch (train.py:822-828, :940-946) kept on the device: update is ONE device op, result ONE read."""

    def __init__(self):
        self.total, self.count = None, 0

    def update(self, terms, bsz):
        if self.total is None:
            self.total = torch.zeros_like(terms)
        self.total.add_(terms, alpha=int(bsz))
        self.count += int(bsz)

    def result(self):
        """{term: total / (EPS + pairs)} in the order ops.SI_OBJECTIVE_TERMS."""
        total = [0.0] * len(ops.SI_OBJECTIVE_TERMS) if self.total is None else self.total.tolist()
        return {k: t / (EPS + self.count) for k, t in zip(ops.SI_OBJECTIVE_TERMS, total)}


class SIEvalMeter:
    """The per-sample errors of evaluate_epoch (train.py:1101-1173) in device buffers of `capacity` pairs: update writes one batch's
    AE, SE, NED, EED at the meter's offset with no host read; result reads once and returns AE / SE / NED / EED (tensors on the host),
    MAE, MSE, RMSE, MNED, MEED and AUC = roc_auc_score(counts > 0, relu(pred_c) > 0), which for binary scores is (TPR + TNR) / 2."""

    def __init__(self, capacity, device=None):
        self.capacity, self.count, self.device, self.buf = int(capacity), 0, device, None
        if self.capacity < 1:
            raise ValueError("capacity must be >= 1 (got %d)" % self.capacity)

    def _buffers(self, device):
        if self.buf is None:
            self.buf = [torch.zeros(self.capacity, dtype=torch.float32, device=device) for _ in range(4)]
            self.buf.append(torch.zeros(self.capacity, dtype=torch.int32, device=device))
        return self.buf

    def update(self, output, counts, node_weights=None, edge_weights=None, model=None, is_graph=True):
        pred_c = output["pred_c"]
        bsz = int(pred_c.numel())
        if self.count + bsz > self.capacity:
            raise ValueError("SIEvalMeter: %d pairs do not fit behind %d of a capacity of %d" % (bsz, self.count, self.capacity))
        pv = wv = pe = we = None
        if node_weights is not None and output["pred_v"] is not None and is_graph:
            pv, wv = output["pred_v"], _refined(model, "refine_node_weights", node_weights)
        if edge_weights is not None and output["pred_e"] is not None:
            pe, we = output["pred_e"], _refined(model, "refine_edge_weights", edge_weights)
        ops.si_eval_errors(pred_c, counts.float(), pv, wv, pe, we, self.count, *self._buffers(self.device or pred_c.device))
        self.count += bsz

    def result(self):
        n = self.count
        if n == 0:
            raise ValueError("SIEvalMeter.result: no pairs")
        ae, se, ned, eed, cls = self.buf
        host = torch.cat([ae[:n].double(), se[:n].double(), ned[:n].double(), eed[:n].double(), cls[:n].double()]).cpu()   # the one read
        ae, se, ned, eed, cls = (host[i * n:(i + 1) * n] for i in range(5))
        tn, fn, fp, tp = (float((cls == k).sum()) for k in (0, 1, 2, 3))
        if tp + fn == 0 or tn + fp == 0:
            raise ValueError("Only one class present in y_true. ROC AUC score is not defined in that case.")
        mse = float(se.mean())
        return {"AE": ae.float(), "SE": se.float(), "NED": ned.float(), "EED": eed.float(), "MAE": float(ae.mean()), "MSE": mse,
                "RMSE": mse ** 0.5, "MNED": float(ned.mean()), "MEED": float(eed.mean()),
                "AUC": (tp / (tp + fn) + tn / (tn + fp)) / 2}
