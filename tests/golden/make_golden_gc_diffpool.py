"""Golden vectors of the DiffPool graph classifier: the reference's own models/diffpool.py, imported UNMODIFIED by file path, run in
float64 on the CPU under the stand-ins of _ref_standins_dense.py (torch_geometric's dense names; parity with a real torch_geometric
unpinned, see there).

Run on the authoring box only (needs the reference checkout; DN_REFERENCE overrides its place):
    python tests/golden/make_golden_gc_diffpool.py
Writes gc_diffpool.npz (data only).

Per case <tag>: the batch (x, edge_index, batch, y), init/<key> = the state_dict at construction, one TRAINING step from it --
logp, loss = F.nll_loss(logp, y), grad/<parameter>, after/<BatchNorm buffer> -- and eval_logp, the eval() forward after that step.
Case A also holds one DiffPoolLayer call at level 0 (layer0/x, adj, link, ent: diffpool_layers[0] on the padded batch) and one at a
dense level (layer1/...: diffpool_layers[1] on level 0's outputs), both in training mode from the initial state.

Asserted here for every case: at every max readout (over the clusters of each level and of final_embed, training and eval forward) the
runner-up lies more than 1e-3 |winner| below the winner, so that an fp32 run cannot flip an argmax; seeds are tried until it holds.
One kind of exact tie is let through, the column in which ALL clusters of a graph hold the same value: the x1 / x2 blocks of a level
are BatchNorm(ReLU(.)), so every cluster whose pre-activation is negative holds the same value BatchNorm(0) of that column, bit for
bit in any precision, and it is the maximum only where no cluster is positive (with 3 clusters and 16 such columns per graph,
every batch has some).  Two equal values above a third do not pass.  Which of the equal clusters the max picks changes
nothing: the value is the same, the BatchNorm statistics see the same column gradient sum, and the gradient that reaches the chosen
cluster's input stops at its ReLU.  The number of such ties is stored in the case's meta."""
import copy
import importlib.util
import json
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _ref_standins_dense as SD  # noqa: E402

REF = os.environ.get("DN_REFERENCE", "/root/reference")
DIMS = {"gnn_dim_hidden": 8, "dim_embedding": 16, "dim_embedding_MLP": 10}
MARGIN = 1e-3


def _reference():
    SD.install()
    path = os.path.join(REF, "graph_classification", "graph_neural_networks", "models", "diffpool.py")
    spec = importlib.util.spec_from_file_location("ref_diffpool", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _graph(rng, n, extra, loops=0, multi=0, isolated=None):
    """Edges of one graph on n nodes: `extra` random directed edges, `loops` self loops, `multi` repeated edges; node `isolated`
    (if any) touches nothing."""
    live = [v for v in range(n) if v != isolated]
    e = []
    if len(live) > 1:
        for _ in range(extra):
            a, b = rng.choice(live, size=2, replace=False)
            e.append((int(a), int(b)))
        for _ in range(multi):
            e.append(e[int(rng.integers(len(e)))])
    for _ in range(loops):
        v = int(rng.choice(live))
        e.append((v, v))
    return e


def _collate(graphs, F_, rng, classes):
    xs, ei, bs, base = [], [], [], 0
    for g, (n, edges) in enumerate(graphs):
        xs.append(rng.standard_normal((n, F_)))
        ei += [(a + base, b + base) for a, b in edges]
        bs += [g] * n
        base += n
    ei = np.asarray(ei, dtype=np.int64).reshape(-1, 2).T
    return dict(x=torch.from_numpy(np.concatenate(xs)), edge_index=torch.from_numpy(np.ascontiguousarray(ei)),
                batch=torch.tensor(bs, dtype=torch.long), y=torch.from_numpy(rng.integers(0, classes, size=len(graphs))).long())


def _batch_a(rng):
    # sizes 3 / 9 / 1 / 6: multi-edges, self loops, an isolated node (node 4 of the second graph), a one-node graph with a self loop
    return [(3, _graph(rng, 3, 4, loops=1, multi=1)), (9, _graph(rng, 9, 16, loops=2, multi=3, isolated=4)),
            (1, [(0, 0)]), (6, _graph(rng, 6, 9, loops=0, multi=2))]


def _batch_b(rng):
    return [(n, _graph(rng, n, 2 * n, loops=1, multi=1)) for n in (7, 12, 4, 10, 5)]


def _batch_c(rng):
    # dummy-augmented, TU-shaped: undirected real edges both ways, the dummy node LAST and joined both ways to every real node (its
    # degree is the graph's n - 1 real nodes each way); all graphs of one size, so the padded batch has no padding
    out = []
    for _ in range(4):
        n, e = 8, []
        for _ in range(9):
            a, b = rng.choice(n - 1, size=2, replace=False)
            e += [(int(a), int(b)), (int(b), int(a))]
        e += [(n - 1, v) for v in range(n - 1)] + [(v, n - 1) for v in range(n - 1)]
        out.append((n, e))
    return out


def _batch_d(rng):
    return [(n, _graph(rng, n, 2 * n, loops=1, multi=2)) for n in (14, 5, 9, 11, 3, 8)]


CASES = [  # tag, layers, max_num_nodes, features, classes, batch
    ("A", 2, 12, 5, 3, _batch_a),
    ("B", 1, 30, 4, 2, _batch_b),
    ("C", 2, 8, 6, 2, _batch_c),
    ("D", 3, 40, 5, 3, _batch_d),
]


class _Readouts:
    """Forward hooks on every level: the tensors torch.max(x, dim=1) is taken of."""

    def __init__(self, model):
        self.seen, self.ties = [], 0
        for layer in model.diffpool_layers:
            layer.register_forward_hook(lambda m, i, o: self.seen.append(o[0].detach()))
        model.final_embed.register_forward_hook(lambda m, i, o: self.seen.append(o.detach()))

    def margin_ok(self):
        for x in self.seen:
            if x.shape[1] < 2:
                continue
            top = torch.topk(x, 2, dim=1).values
            gap = top[:, 0] - top[:, 1]
            shared = x.max(dim=1).values == x.min(dim=1).values              # ALL clusters of the column hold one value
            self.ties += int(shared.sum())
            if not bool(((gap > MARGIN * top[:, 0].abs()) | shared).all()):
                return False
        return True


def _run_case(ref, tag, layers, max_nodes, F_, classes, make_batch, seed):
    rng = np.random.default_rng(seed)
    data = _collate(make_batch(rng), F_, rng, classes)
    cfg = dict(DIMS, num_layers=layers)
    args = SimpleNamespace(num_features=F_, num_classes=classes, max_num_nodes=max_nodes, additional=json.dumps(cfg))
    torch.manual_seed(seed)
    model = ref.DiffPool(args).double().train()
    out = {"x": data["x"].numpy(), "edge_index": data["edge_index"].numpy(), "batch": data["batch"].numpy(), "y": data["y"].numpy()}
    init = copy.deepcopy(model.state_dict())
    for k, v in init.items():
        out["init/" + k] = v.numpy()
    watch = _Readouts(model)
    d = SimpleNamespace(**data)
    logp = model(d)
    loss = F.nll_loss(logp, data["y"])
    loss.backward()
    out["logp"], out["loss"] = logp.detach().numpy(), np.asarray(float(loss.detach()))
    for k, p in model.named_parameters():
        out["grad/" + k] = (p.grad if p.grad is not None else torch.zeros_like(p)).numpy()
    for k, v in model.state_dict().items():
        if "running_" in k or "num_batches" in k:
            out["after/" + k] = v.numpy().copy()
    model.eval()
    with torch.no_grad():
        out["eval_logp"] = model(d).numpy()
    if not watch.margin_ok():
        return None
    if tag == "A":
        fresh = ref.DiffPool(args).double().train()
        fresh.load_state_dict(init)
        xd, mask = SD.to_dense_batch(data["x"], data["batch"])
        adj = SD.to_dense_adj(data["edge_index"], data["batch"])
        with torch.no_grad():
            r0 = fresh.diffpool_layers[0](xd, adj, mask)
            r1 = fresh.diffpool_layers[1](r0[0], r0[1])
        for name, r in (("layer0", r0), ("layer1", r1)):
            for key, v in zip(("x", "adj", "link", "ent"), r):
                out["%s/%s" % (name, key)] = v.numpy()
    meta = dict(tag=tag, num_layers=layers, max_num_nodes=max_nodes, num_features=F_, num_classes=classes, seed=seed,
                additional=cfg, num_graphs=int(data["batch"].max()) + 1, exact_ties=watch.ties)
    return meta, out


def make():
    torch.set_default_dtype(torch.float64)
    ref = _reference()
    store, metas = {}, []
    for tag, layers, max_nodes, F_, classes, make_batch in CASES:
        for seed in range(100, 1100):
            got = _run_case(ref, tag, layers, max_nodes, F_, classes, make_batch, seed)
            if got is not None:
                break
        assert got is not None, "no seed of case %s keeps the readout margins" % tag
        meta, out = got
        metas.append(meta)
        for k, v in out.items():
            store[tag + "/" + k] = v
        print("case %s: seed %d, loss %.6f, exact ties %d" % (tag, meta["seed"], float(out["loss"]), meta["exact_ties"]))
    store["meta"] = np.frombuffer(json.dumps(metas).encode(), dtype=np.uint8)
    path = os.path.join(HERE, "gc_diffpool.npz")
    np.savez_compressed(path, **store)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    make()
