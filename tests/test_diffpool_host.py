"""DiffPool without a GPU, in float64 against the reference's own run (tests/golden/gc_diffpool.npz, make_golden_gc_diffpool.py):
the ragged restatement tests/diffpool_ref.py equals it to 1e-10, and so does the package's model on CPU tensors -- the COMPOSED path
(the same ragged mathematics in torch ops) under the reference's state_dict names."""
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import diffpool_ref as R

TOL = 1e-10


@pytest.fixture(scope="module")
def gold(golden_dir):
    z = np.load(os.path.join(golden_dir, "gc_diffpool.npz"))
    return z, {m["tag"]: m for m in json.loads(bytes(z["meta"]).decode())}


def _close(got, want, what):
    got, want = torch.as_tensor(got).double(), torch.as_tensor(want).double()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = float((got - want).abs().max()) if want.numel() else 0.0
    assert err <= TOL * max(1.0, float(want.abs().max()) if want.numel() else 0.0), (what, err)


def _case(z, tag):
    t = lambda k: torch.from_numpy(z[tag + "/" + k])  # noqa: E731
    ei, batch = t("edge_index"), t("batch")
    B = int(batch.max()) + 1
    ptr = [0] + torch.cumsum(torch.bincount(batch, minlength=B), 0).tolist()
    init = {k[len(tag) + 6:]: torch.from_numpy(z[k]) for k in z.files if k.startswith(tag + "/init/")}
    return t, t("x"), ei[0], ei[1], batch, t("y"), ptr, init


def _params(init):
    return {k: (v.clone().requires_grad_(True) if v.is_floating_point() and "running_" not in k else v.clone()) for k, v in init.items()}


TAGS = ["A", "B", "C", "D"]


@pytest.mark.parametrize("tag", TAGS)
def test_the_restatement_equals_the_reference(gold, tag):
    z, meta = gold
    t, x, src, dst, batch, y, ptr, init = _case(z, tag)
    p, after = _params(init), {}
    logp = R.forward(p, meta[tag]["num_layers"], x, src, dst, ptr, True, after)
    loss = F.nll_loss(logp, y)
    loss.backward()
    _close(logp.detach(), t("logp"), "logp")
    _close(loss.detach(), t("loss"), "loss")
    for k, v in p.items():
        if v.requires_grad:
            _close(torch.zeros_like(v) if v.grad is None else v.grad, t("grad/" + k), "grad " + k)
    names = [k[len(tag) + 7:] for k in z.files if k.startswith(tag + "/after/")]
    assert sorted(names) == sorted(after) and names
    for k in names:
        _close(after[k], t("after/" + k), "after " + k)
    with torch.no_grad():
        q = dict(init, **after)
        _close(R.forward(q, meta[tag]["num_layers"], x, src, dst, ptr, False), t("eval_logp"), "eval logp")


def test_the_restated_layers_return_all_four_outputs(gold):
    z, _ = gold
    t, x, src, dst, batch, y, ptr, init = _case(z, "A")
    with torch.no_grad():
        r0 = R.layer0(init, "diffpool_layers.0.", x, src, dst, ptr, True)
        r1 = R.dense_layer(init, "diffpool_layers.1.", r0[0], r0[1], True)
    for name, r in (("layer0", r0), ("layer1", r1)):
        for key, v in zip(("x", "adj", "link", "ent"), r):
            _close(v, t("%s/%s" % (name, key)), name + " " + key)


def _model(meta, additional, dtype=torch.float64):
    from dummynode4graphlearning_amd import graph_classification as GC
    args = SimpleNamespace(num_features=meta["num_features"], num_classes=meta["num_classes"], max_num_nodes=meta["max_num_nodes"],
                           additional=additional)
    return GC.DiffPool(args).to(dtype)


@pytest.mark.parametrize("tag", TAGS)
def test_the_composed_path_equals_the_reference_on_cpu_tensors(gold, tag):
    from dummynode4graphlearning_amd import GraphBatch
    z, meta = gold
    t, x, src, dst, batch, y, ptr, init = _case(z, tag)
    model = _model(meta[tag], json.dumps(meta[tag]["additional"]))
    model.load_state_dict(init, strict=True)
    model.train()
    data = GraphBatch(x, torch.stack([src, dst]), batch, y=y, num_graphs=meta[tag]["num_graphs"])
    logp = model(data)
    loss = F.nll_loss(logp, y)
    loss.backward()
    _close(logp.detach(), t("logp"), "logp")
    _close(loss.detach(), t("loss"), "loss")
    for k, v in model.named_parameters():
        _close(torch.zeros_like(v) if v.grad is None else v.grad, t("grad/" + k), "grad " + k)
    for k, v in model.state_dict().items():
        if "running_" in k or "num_batches" in k:
            _close(v, t("after/" + k), "after " + k)
    model.eval()
    with torch.no_grad():
        _close(model(data), t("eval_logp"), "eval logp")


def test_the_package_layers_return_all_four_outputs(gold):
    from dummynode4graphlearning_amd import GraphBatch
    from dummynode4graphlearning_amd.graph import diffpool_index_of
    z, meta = gold
    t, x, src, dst, batch, y, ptr, init = _case(z, "A")
    model = _model(meta["A"], meta["A"]["additional"])                       # (a dict is taken too)
    model.load_state_dict(init, strict=True)
    model.train()
    l0, l1 = model.diffpool_layers[0], model.diffpool_layers[1]
    assert l0.compute_losses is False                                        # the model switches them off ...
    l0.compute_losses = l1.compute_losses = True                             # ... a layer on its own computes them
    data = GraphBatch(x, torch.stack([src, dst]), batch, num_graphs=meta["A"]["num_graphs"])
    with torch.no_grad():
        r0 = l0(x, diffpool_index_of(data))
        r1 = l1(r0[0], r0[1])
    for name, r in (("layer0", r0), ("layer1", r1)):
        for key, v in zip(("x", "adj", "link", "ent"), r):
            _close(v, t("%s/%s" % (name, key)), name + " " + key)


@pytest.mark.parametrize("tag", TAGS)
def test_state_dict_names_and_shapes_are_the_references(gold, tag):
    z, meta = gold
    init = _case(z, tag)[7]
    model = _model(meta[tag], json.dumps(meta[tag]["additional"]), torch.float32)
    own = model.state_dict()
    assert list(own) == list(init)                                           # the same keys in the same order
    assert all(tuple(own[k].shape) == tuple(init[k].shape) for k in init)
    model.load_state_dict({k: v.float() if v.is_floating_point() else v for k, v in init.items()}, strict=True)
    pre = "diffpool_layers.0.gnn_pool."
    for k in ("conv1.lin_rel.weight", "conv1.lin_root.weight", "conv1.lin_root.bias", "bn1.running_mean", "bn2.num_batches_tracked",
              "lin.weight"):
        assert pre + k in own
    assert pre + "conv1.lin_rel.bias" not in own and "diffpool_layers.0.gnn_embed.lin.weight" not in own


def test_cluster_counts_defaults_and_the_additional_argument():
    from dummynode4graphlearning_amd import graph_classification as GC
    mk = lambda n, add: GC.DiffPool(SimpleNamespace(num_features=4, num_classes=2, max_num_nodes=n, additional=add))  # noqa: E731
    m = mk(621, None)                                                        # the defaults: 2 layers, factor 0.25
    assert [l.gnn_pool.lin.out_features for l in m.diffpool_layers] == [156, 39]
    assert m.diffpool_layers[0].gnn_embed.conv3.lin_rel.out_features == 128 and m.lin1.out_features == 50
    assert m.lin1.in_features == 3 * (2 * 64 + 128)
    one = dict(GC.diffpool.DEFAULT_CONFIG, num_layers=1)
    assert [l.gnn_pool.lin.out_features for l in mk(111, json.dumps(one)).diffpool_layers] == [12]          # ceil(0.1 * 111)
    three = dict(GC.diffpool.DEFAULT_CONFIG, num_layers=3)
    assert [l.gnn_pool.lin.out_features for l in mk(40, three).diffpool_layers] == [10, 3, 1]


def test_an_edge_between_two_graphs_is_refused():
    from dummynode4graphlearning_amd import GraphBatch, _lib
    from dummynode4graphlearning_amd.graph import diffpool_index_of
    data = GraphBatch(torch.zeros(4, 2), torch.tensor([[0, 1], [1, 2]]), torch.tensor([0, 0, 1, 1]))
    with pytest.raises(_lib.DnHipError, match="joins two graphs"):
        diffpool_index_of(data)


def test_an_edge_outside_the_rows_is_refused_before_it_indexes_anything():
    from dummynode4graphlearning_amd import GraphBatch, _lib
    from dummynode4graphlearning_amd.graph import diffpool_index_of
    for bad in (7, -1):
        data = GraphBatch(torch.zeros(4, 2), torch.tensor([[0, 1], [1, bad]]), torch.tensor([0, 0, 1, 1]))
        with pytest.raises(_lib.DnHipError, match="outside the batch's 4 rows"):
            diffpool_index_of(data)


def test_the_index_is_rebuilt_when_the_edges_change_in_place():
    from dummynode4graphlearning_amd import GraphBatch
    from dummynode4graphlearning_amd.graph import diffpool_index_of
    data = GraphBatch(torch.zeros(4, 2), torch.tensor([[0, 0], [1, 1]]), torch.tensor([0, 0, 1, 1]))
    first = diffpool_index_of(data)
    assert diffpool_index_of(data) is first                                  # cached on the batch
    assert first.out_deg.view(-1).tolist() == [2, 1, 1, 1]
    data.edge_index[0, 1] = 1                                                # the same size, another edge: (1, 1) for (0, 1)
    again = diffpool_index_of(data)
    assert again is not first and again.out_deg.view(-1).tolist() == [1, 1, 1, 1]
