"""The SI count models RGIN / RGCN (SURVEY.md 8b "SI model"): GraphAdjModel and the encoders, embeddings and filter it builds.

Same constructor (the **kw dict of train.py:84-105 build_model), state_dict keys / shapes, initial values under a given
torch.manual_seed (the RNG is used in the reference's order: enc -> filter -> emb -> graph rep -> pattern rep -> pred,
basemodel.py:43-59), forward(pattern, graph) -> OutputDict, refine_node_weights and expand(**kw) as
subgraph_isomorphism/models/basemodel.py:15-219, 629-982, rgin.py:175-260 and rgcn.py:215-300.  The rep nets are this
package's RGINRepNet / RGCNRepNet; the glue around them runs on dn_simodel.hip:

* filter gate + batch lengths + id / label checks in one launch (replaces ScalarFilter + get_filter_gate and the two Python
  mask loops of batch_convert_len_to_mask), read back once per forward;
* code embedding enc[key] @ W in one launch per side, its weight gradient deterministic;
* the Sum / Mean / Max head on the ragged rows: the [enc_v | enc_vl | out_deg | in_deg | rep] rows are pooled per graph without
  building the concatenation or the padded tensor.  The padded head (pred.py on split_and_batchify_graph_feats) stays for the
  per-position weights (pred_return_weights containing "node") and for training with pred_dropout > 0.

forward has no CPU path; construction, state_dict and expand work on the CPU."""
from collections import OrderedDict

import numpy as np
import torch as th
import torch.nn as nn
import torch.nn.functional as F

from .. import ops
from .attn_pred import ATTN_PRED_NETS, BaseAttnPredictNet, DIAMNet, MaxAttnPredictNet, MeanAttnPredictNet, build_attn_pred_net
from .dl import split_and_batchify_graph_feats
from .pred import MaxPredictNet, MeanPredictNet, SumPredictNet
from .rgcn import RGCNRepNet
from .rgin import RGINRepNet

NODEID, NODELABEL, EDGELABEL, DUMMYFLAG = "id", "label", "label", "is_dummy"      # constants.py:14-23
_UNSUPPORTED_PRED_NETS = ("MeanAttnPredictNet", "SumAttnPredictNet", "MaxAttnPredictNet", "MeanMemAttnPredictNet",
                          "SumMemAttnPredictNet", "MaxMemAttnPredictNet", "DIAMNet")
_ATTN_HEADS = (BaseAttnPredictNet, DIAMNet)


def _constructor_refusal(pred_net):
    if pred_net in ATTN_PRED_NETS:
        return ("pred_net=%s is not accepted by the constructor; build the model with one of the pooling heads and attach it with "
                "model.set_pred_net(%r, **kw)" % (pred_net, pred_net))
    return "pred_net=%s is not provided by this package (the memory-attention heads are out of scope, DESIGN.md 7)" % pred_net


def _is_attn_head(net):
    nets = net.values() if isinstance(net, nn.ModuleDict) else (net,)
    return any(isinstance(n, _ATTN_HEADS) for n in nets)


def attn_ragged_ok(net, training):
    """Can the steps of this attention head run on ops.seg_attention?  The attentions as the heads build them: projected (hidden_dim
    != -1), no zero key, no input layer norms, no active dropout inside.  Anything else goes through the padded modules."""
    return all(a.weight_q is not None and a.weight_v is not None and not a.add_zero_attn and not a.pre_lnorm
               and a.score_func in ops.SEG_SCORES and not (training and a.drop.p > 0) for a in (net.p_attn, net.g_attn))


def attn_steps_ragged(net, p_rows, p_ptr, p_skip, Lp, g_rows, g_ptr, g_skip, Lg):
    """The inference steps of BaseAttnPredictNet on the ragged rows [Np, D] / [Ng, D] (skipped rows already zero): per step the graph
    rows attend to the pattern rows and then to themselves.  Returns the refined graph rows; skipped rows stay zero rows."""
    pa, ga = net.p_attn, net.g_attn
    pk, pv = _proj(p_rows, pa.weight_k), _proj(p_rows, pa.weight_v)
    g = g_rows
    for _ in range(net.infer_steps):
        a = ops.seg_attention(_proj(g, pa.weight_q), pk, pv, g_ptr, p_ptr, pa.num_heads, pa.scale, pa.score_func, g_skip, p_skip,
                              max_q=Lg, max_k=Lp)
        g = pa.close(g, _proj(a, pa.weight_o))
        a = ops.seg_attention(_proj(g, ga.weight_q), _proj(g, ga.weight_k), _proj(g, ga.weight_v), g_ptr, g_ptr, ga.num_heads,
                              ga.scale, ga.score_func, g_skip, g_skip, max_q=Lg, max_k=Lg)
        g = ga.close(g, _proj(a, ga.weight_o))
    return g


def diamnet_memory_ragged(net, p_rows, p_ptr, p_skip, Lp, g_rows, g_ptr, g_skip, Lg):
    """DIAMNet's memory on the ragged rows: the window pool of the graph rows, mem_layer, then infer_steps rounds with the mem_len
    memory rows of every pair as the queries.  Returns the flattened memory [B, mem_len * hidden]."""
    B, M = g_ptr.numel() - 1, net.mem_len
    mem, m_mask = ops.seg_window_pool(g_rows, g_ptr, g_skip, M, net.mem_init, max_len=Lg)
    m = ops.linear_any(mem, net.mem_layer.weight, net.mem_layer.bias)
    m_ptr = th.arange(0, (B + 1) * M, M, dtype=th.int32, device=m.device)
    m_skip = (~m_mask).reshape(-1).view(th.uint8)
    pa, ga = net.p_attn, net.g_attn
    pk, pv = _proj(p_rows, pa.weight_k), _proj(p_rows, pa.weight_v)
    gk, gv = _proj(g_rows, ga.weight_k), _proj(g_rows, ga.weight_v)
    for _ in range(net.infer_steps):
        a = ops.seg_attention(_proj(m, pa.weight_q), pk, pv, m_ptr, p_ptr, pa.num_heads, pa.scale, pa.score_func, m_skip, p_skip,
                              max_q=M, max_k=Lp)
        m = pa.close(m, _proj(a, pa.weight_o))
        a = ops.seg_attention(_proj(m, ga.weight_q), gk, gv, m_ptr, g_ptr, ga.num_heads, ga.scale, ga.score_func, m_skip, g_skip,
                              max_q=M, max_k=Lg)
        m = ga.close(m, _proj(a, ga.weight_o))
    return m.reshape(B, -1)


def _proj(x, w):
    """x @ w for a parameter stored [in, out] (the attention weights), on the any-width HIP product."""
    return ops.linear_any(x.contiguous(), w.t().contiguous())


def _zero_skipped(rows, skip):
    return rows if skip is None else rows.masked_fill(skip.reshape(-1, 1).bool(), 0)


def attn_head_ragged(net, p_rows, p_ptr, p_skip, Lp, p_count, g_rows, g_ptr, g_skip, Lg, g_count):
    """forward of an attention head or of DIAMNet (return_weights off, no dropout) on ragged rows: the steps on ops.seg_attention /
    ops.seg_window_pool, the closing pool on dn_si_pool_sum / dn_si_pool_max with the bias as the value of every padded position."""
    p_skip, g_skip = ops._u8_or_none(p_skip), ops._u8_or_none(g_skip)
    p_rows, g_rows = _zero_skipped(p_rows, p_skip).contiguous(), _zero_skipped(g_rows, g_skip).contiguous()
    dt = g_rows.dtype
    pl, gl = p_count.to(th.float32).view(-1, 1), g_count.to(th.float32).view(-1, 1)
    pl_inv, gl_inv = (1.0 / pl).to(dt), (1.0 / gl).to(dt)
    pl, gl = pl.to(dt), gl.to(dt)
    if isinstance(net, DIAMNet):
        m = diamnet_memory_ragged(net, p_rows, p_ptr, p_skip, Lp, g_rows, g_ptr, g_skip, Lg)
        return net.close_memory(m, pl, gl, pl_inv, gl_inv)
    g_rows = attn_steps_ragged(net, p_rows, p_ptr, p_skip, Lp, g_rows, g_ptr, g_skip, Lg)
    pooled = []
    for rows, fc, ptr, skip, L in ((p_rows, net.p_fc, p_ptr, p_skip, Lp), (g_rows, net.g_fc, g_ptr, g_skip, Lg)):
        if isinstance(net, MaxAttnPredictNet):
            pooled.append(ops.si_pool_max(ops.linear_any(rows.contiguous(), fc.weight, fc.bias), fc.bias, ptr, L, skip))
            continue
        S, _ = ops.si_pool_sum(rows.contiguous(), ptr, skip)
        y = th.addmm(fc.bias.float() * L, S, fc.weight.float().t())
        pooled.append((y / L if isinstance(net, MeanAttnPredictNet) else y).to(dt))
    p, g = pooled
    y = net.act(net.pred_fc1(th.cat([p, g, g - p, g * p, pl, gl, pl_inv, gl_inv], dim=1)))
    return net.pred_fc2(th.cat([y, pl, gl, pl_inv, gl_inv], dim=1))


# ------------------------------------------------------------------------------------------------ container.py:14-100
class OutputDict(OrderedDict):
    """The model output: an ordered dict of the 15 entries of basemodel.py:964-980 (None entries kept), readable by key, by
    attribute and by position (to_tuple)."""

    def __getattr__(self, name):
        try:
            return self[name]
        except KeyError:
            raise AttributeError(name)

    def __getitem__(self, k):
        if isinstance(k, str):
            return super().__getitem__(k)
        return self.to_tuple()[k]

    def __delitem__(self, *args, **kwargs):
        raise Exception("You cannot use ``__delitem__`` on a %s instance." % self.__class__.__name__)

    def setdefault(self, *args, **kwargs):
        raise Exception("You cannot use ``setdefault`` on a %s instance." % self.__class__.__name__)

    def pop(self, *args, **kwargs):
        raise Exception("You cannot use ``pop`` on a %s instance." % self.__class__.__name__)

    def update(self, *args, **kwargs):
        raise Exception("You cannot use ``update`` on a %s instance." % self.__class__.__name__)

    def to_tuple(self):
        return tuple(self[k] for k in self.keys())


# ------------------------------------------------------------------------------------------------ embed.py
def get_enc_len(x, base=10):
    """Digits of x in `base` (at least 1), embed.py:8-35."""
    n, cnt = int(x), 0
    while n > 0:
        n //= base
        cnt += 1
    return max(cnt, 1)


def int2multihot(x, len_x, base=10):
    """embed.py:70-101: per digit position a one-hot of the digit ([n, len_x * base], int64); leading zeros count as digit 0."""
    x = np.asarray(x, dtype=np.int64).reshape(-1)
    rep = np.zeros((len(x), len_x * base), dtype=np.int64)
    for i, n in enumerate(x):
        n = int(n) % base ** len_x
        idx = (len_x - 1) * base
        while n:
            rep[i, idx + n % base] = 1
            n //= base
            idx -= base
        while idx >= 0:
            rep[i, idx] = 1
            idx -= base
    return rep


class Embedding(nn.Embedding):
    """embed.py:105-121: a lookup for long input, a product with the weight for multi-hot float rows."""

    def forward(self, x):
        if x.dtype == th.long:
            return super().forward(x)
        if x.is_floating_point() and x.size(-1) == self.num_embeddings:
            return th.matmul(x.view(-1, x.size(-1)), self.weight).view(x.size()[:-1] + (self.embedding_dim,))
        raise NotImplementedError

    def get_output_dim(self):
        return self.embedding_dim


class NormalEmbedding(Embedding):
    def __init__(self, num_embeddings, embedding_dim, **kw):
        super().__init__(num_embeddings, embedding_dim, **kw)
        nn.init.normal_(self.weight, 0.0, 1.0)
        if self.padding_idx is not None:
            with th.no_grad():
                self.weight[self.padding_idx].fill_(0)


class UniformEmbedding(Embedding):
    def __init__(self, num_embeddings, embedding_dim, **kw):
        super().__init__(num_embeddings, embedding_dim, **kw)
        nn.init.uniform_(self.weight, -1.0, 1.0)
        if self.padding_idx is not None:
            with th.no_grad():
                self.weight[self.padding_idx].fill_(0)


class OrthogonalEmbedding(Embedding):
    def __init__(self, num_embeddings, embedding_dim, **kw):
        super().__init__(num_embeddings, embedding_dim, **kw)
        nn.init.orthogonal_(self.weight)
        if self.padding_idx is not None:
            with th.no_grad():
                self.weight[self.padding_idx].fill_(0)


class EquivariantEmbedding(Embedding):
    """embed.py:162-194, quirks kept: `weight` starts as the rolls of `row_vec` and then trains as a free matrix (the forward
    never reads row_vec, so row_vec gets no gradient; allow_forward is only cleared by an explicit call of .backward, which
    autograd never makes)."""

    def __init__(self, num_embeddings, embedding_dim, **kw):
        super().__init__(num_embeddings, embedding_dim, **kw)
        self.row_vec = nn.Parameter(th.Tensor(self.embedding_dim))
        self.allow_forward = True
        nn.init.normal_(self.row_vec, 0.0, 1.0)
        with th.no_grad():
            for i in range(num_embeddings):
                self.weight[i].data.copy_(th.roll(self.row_vec, i, 0))

    def refresh(self):
        if not self.allow_forward:
            with th.no_grad():
                for i in range(self.num_embeddings):
                    self.weight[i] = th.roll(self.row_vec, i, 0)
            self.allow_forward = True

    def forward(self, x):
        self.refresh()
        return super().forward(x)

    def backward(self, x):
        self.allow_forward = False
        return super().backward(x)


class MultihotEmbedding(Embedding):
    """embed.py:197-208: frozen table of the base-`base` multi-hot codes of 0 .. max_n - 1."""

    def __init__(self, max_n=1024, base=2):
        self.max_n = max_n
        self.base = base
        enc_len = get_enc_len(max_n - 1, base)
        super().__init__(max_n, 2 * enc_len)
        with th.no_grad():
            self.weight.data.copy_(th.from_numpy(int2multihot(np.arange(0, max_n), enc_len, base)).float())

    def extra_repr(self):
        return "base=%d, max_n=%d, enc_dim=%d" % (self.base, self.max_n, self.weight.shape[1])


class PositionEmbedding(Embedding):
    """embed.py:211-222: frozen sinusoid table."""

    def __init__(self, embedding_dim, max_len=512, scale=1):
        freq_seq = th.arange(0, embedding_dim, 2.0, dtype=th.float)
        inv_freq = th.pow(10000, (freq_seq / embedding_dim)).reciprocal()
        sinusoid_inp = th.outer(th.arange(0, max_len, 1.0), inv_freq)
        super().__init__(max_len, embedding_dim)
        with th.no_grad():
            self.weight.data.copy_(th.cat([th.sin(sinusoid_inp), th.cos(sinusoid_inp)], dim=-1) * scale)

    def extra_repr(self):
        return "embedding_dim=%d, max_len=%d" % (self.weight.shape[1], self.weight.shape[0])


# ------------------------------------------------------------------------------------------------ filter.py:6-16
class ScalarFilter(nn.Module):
    """gate[b, j] = g_x[b, j] occurs in p_x[b] (padded [bsz, l1] / [bsz, l2] inputs).  The model does not call it: its gate comes
    from dn_si_filter_meta on the ragged labels."""

    def forward(self, p_x, g_x):
        matrix = g_x.unsqueeze(2) - p_x.unsqueeze(1)
        return th.max(matrix == 0, dim=2)[0]


# ------------------------------------------------------------------------------------------------ utils/dl.py:157-191
def expand_dimensions(old_module, new_module, pre_pad=True):
    """Copy old parameters into the (larger) new ones, zeros elsewhere; pre_pad puts the old values at the END of every dim."""
    with th.no_grad():
        if isinstance(old_module, th.Tensor):
            nn.init.zeros_(new_module)
            size = old_module.size()
            if len(size) > 4:
                raise NotImplementedError
            sl = tuple(slice(-n, None) if pre_pad else slice(0, n) for n in size)
            new_module.data[sl].copy_(old_module)
            return
        old_params = dict(old_module.named_parameters())
        for name, p in new_module.named_parameters():
            if name in old_params:
                expand_dimensions(old_params[name], p, pre_pad)


def _i32(t):
    t = t.reshape(-1)
    return t if t.dtype == th.int32 else t.to(th.int32)


# ------------------------------------------------------------------------------------------------ basemodel.py
class GraphAdjModel(nn.Module):
    def __init__(self, **kw):
        super().__init__()
        self.add_node_id = kw.get("add_node_id", kw.get("gnn_add_node_id", False))
        self.max_ngv = kw["max_ngv"]
        self.max_ngvl = kw["max_ngvl"]
        self.max_nge = kw["max_nge"]
        self.max_ngel = kw["max_ngel"]
        self.max_npv = kw["max_npv"]
        self.max_npvl = kw["max_npvl"]
        self.max_npe = kw["max_npe"]
        self.max_npel = kw["max_npel"]
        self.base = kw.get("base", 2)                     # (sic: not enc_base, basemodel.py:33)
        self.hid_dim = kw.get("hid_dim", 64)
        self.share_emb_net = kw.get("share_emb_net", True)
        self.share_enc_net = kw.get("share_enc_net", True)
        self.share_rep_net = kw.get("share_rep_net", True)
        self.rep_residual = kw.get("rep_residual", True)
        self.pred_with_enc = kw.get("pred_with_enc", False)
        self.pred_with_deg = kw.get("pred_with_deg", False)

        self.g_enc_net = self.create_enc_net(type="graph", **kw)
        self.p_enc_net = self.create_enc_net(type="pattern", **kw)
        self.filter_net = self.create_filter_net(**kw)
        self.g_emb_net = self.create_emb_net(type="graph", **kw)
        self.p_emb_net = self.create_emb_net(type="pattern", **kw)
        self.g_rep_net = self.create_rep_net(type="graph", **kw)
        self.p_rep_net = self.create_rep_net(type="pattern", **kw)
        self.pred_net = self.create_pred_net(**kw)

    # ---- construction (basemodel.py:61-123, 634-828) ----
    def create_enc_net(self, type, **kw):
        enc_net = kw.get("enc_net", "Multihot")
        if type == "graph":
            nv, nvl = self.max_ngv, self.max_ngvl
        elif type == "pattern":
            if self.share_enc_net:
                return self.g_enc_net
            nv, nvl = self.max_npv, self.max_npvl
        else:
            raise ValueError
        if enc_net == "Multihot":
            enc = OrderedDict({"v": MultihotEmbedding(nv, self.base), "vl": MultihotEmbedding(nvl, self.base)})
        elif enc_net == "Position":
            enc = OrderedDict({"v": PositionEmbedding(get_enc_len(nv - 1, self.base) * self.base, nv),
                               "vl": PositionEmbedding(get_enc_len(nvl - 1, self.base) * self.base, nvl)})
        else:
            raise NotImplementedError(enc_net)
        for net in enc.values():
            net.weight.requires_grad = False
        return nn.ModuleDict(enc)

    def create_filter_net(self, **kw):
        filter_net = kw.get("filter_net", "None")
        if filter_net == "None":
            return None
        if filter_net == "ScalarFilter":
            return nn.ModuleDict({"vl": ScalarFilter()})
        raise ValueError(filter_net)

    def create_emb_net(self, type, **kw):
        emb_net = kw.get("emb_net", "Orthogonal")
        if type == "graph":
            dims = self.get_graph_enc_dims()
        elif type == "pattern":
            dims = self.get_pattern_enc_dims()
        else:
            raise ValueError
        classes = {"Orthogonal": OrthogonalEmbedding, "Normal": NormalEmbedding, "Uniform": UniformEmbedding,
                   "Equivariant": EquivariantEmbedding}
        if emb_net not in classes:
            raise ValueError(emb_net)
        return nn.ModuleDict(OrderedDict({k: classes[emb_net](v, self.hid_dim) for k, v in dims.items()}))

    def create_rep_net(self, type, **kw):
        raise NotImplementedError

    def create_pred_net(self, **kw):
        act_func = kw.get("pred_act_func", "relu")
        dropout = kw.get("pred_dropout", 0.0)
        pred_net = kw.get("pred_net", "SumPredictNet")
        hidden_dim = kw.get("pred_hid_dim", 64)
        return_weights = kw.get("pred_return_weights", "none")
        classes = {"MeanPredictNet": MeanPredictNet, "SumPredictNet": SumPredictNet, "MaxPredictNet": MaxPredictNet}
        if pred_net in classes:
            return classes[pred_net](self.get_rep_dim(), hidden_dim=hidden_dim, act_func=act_func, dropout=dropout,
                                     return_weights="node" in return_weights)
        if pred_net in _UNSUPPORTED_PRED_NETS:
            raise NotImplementedError(_constructor_refusal(pred_net))
        raise ValueError(pred_net)

    def set_pred_net(self, pred_net, **kw):
        """Replace self.pred_net by one of the attention heads or DIAMNet (attn_pred.py), built at get_rep_dim() from the keys of
        the reference's create_pred_net (pred_hid_dim, pred_act_func, pred_dropout, pred_return_weights, pred_num_heads,
        pred_infer_steps, pred_mem_len, pred_mem_init; same defaults).  The new head starts from its own fresh initial values, on
        the device and in the dtype of the head it replaces.  Returns the new head."""
        new = build_attn_pred_net(pred_net, self.get_rep_dim(), "node" in kw.get("pred_return_weights", "none"), **kw)
        old = next(self.pred_net.parameters())
        new = new.to(device=old.device, dtype=old.dtype)
        del self.pred_net
        self.pred_net = new
        return new

    def get_graph_enc_dims(self):
        return OrderedDict({"v": get_enc_len(self.max_ngv - 1, self.base) * self.base,
                            "vl": get_enc_len(self.max_ngvl - 1, self.base) * self.base})

    def get_pattern_enc_dims(self):
        if self.share_enc_net:
            return self.get_graph_enc_dims()
        return OrderedDict({"v": get_enc_len(self.max_npv - 1, self.base) * self.base,
                            "vl": get_enc_len(self.max_npvl - 1, self.base) * self.base})

    def get_graph_enc_dim(self):
        return sum(self.get_graph_enc_dims().values())

    def get_pattern_enc_dim(self):
        return sum(self.get_pattern_enc_dims().values())

    def get_rep_dim(self):
        rep_dim = self.hid_dim
        if self.pred_with_enc:
            rep_dim += self.get_graph_enc_dim()
        if self.pred_with_deg:
            rep_dim += 2
        return rep_dim

    def refine_node_weights(self, weights, use_max=False):
        return weights

    def refine_edge_weights(self, weights, use_max=False):
        return weights

    # ---- representation (implemented by RGIN / RGCN) ----
    def get_pattern_rep(self, pattern, p_emb, mask=None):
        raise NotImplementedError

    def get_graph_rep(self, graph, g_emb, mask=None, gate=None):
        raise NotImplementedError

    # ---- forward (basemodel.py:887-982) ----
    @staticmethod
    def _embed(emb_net, enc_net, ids, labels, add_node_id):
        """emb_net["vl"](enc_net["vl"](labels)) (+ the same for the ids): dn_si_embed_fwd, one launch."""
        for m in emb_net.values():
            if isinstance(m, EquivariantEmbedding):
                m.refresh()
        if add_node_id:
            return ops.si_embed(labels, enc_net["vl"].weight, emb_net["vl"].weight, ids, enc_net["v"].weight, emb_net["v"].weight)
        return ops.si_embed(labels, enc_net["vl"].weight, emb_net["vl"].weight)

    def forward(self, pattern, graph):
        bsz = pattern.batch_size
        if graph.batch_size != bsz:
            raise ValueError("pattern and graph batches differ in size: %d vs %d" % (bsz, graph.batch_size))
        p_ptr, g_ptr = pattern.node_ptr(), graph.node_ptr()
        p_id, p_vl = _i32(pattern.ndata[NODEID]), _i32(pattern.ndata[NODELABEL])
        g_id, g_vl = _i32(graph.ndata[NODEID]), _i32(graph.ndata[NODELABEL])
        dtype = self.g_emb_net["vl"].weight.dtype
        gated = self.filter_net is not None and len(self.filter_net) > 0
        meta, vl_gate = ops.si_filter_meta(
            p_ptr, p_vl, p_id, g_ptr, g_vl, g_id,
            (self.p_enc_net["vl"].num_embeddings, self.p_enc_net["v"].num_embeddings),
            (self.g_enc_net["vl"].num_embeddings, self.g_enc_net["v"].num_embeddings), dtype if gated else None)

        p_v_emb = self._embed(self.p_emb_net, self.p_enc_net, p_id, p_vl, self.add_node_id)
        g_v_emb = self._embed(self.g_emb_net, self.g_enc_net, g_id, g_vl, self.add_node_id)
        p_len, g_len = ops.si_read_meta(meta)               # the forward's one device-to-host read (raises on bad batches)

        p_v_rep = self.get_pattern_rep(pattern, p_v_emb)
        g_v_rep = self.get_graph_rep(graph, g_v_emb, gate=vl_gate)

        p_dummy, g_dummy = pattern.ndata.get(DUMMYFLAG), graph.ndata.get(DUMMYFLAG)
        p_v_mask = self.refine_node_weights(ops.si_len_mask(p_ptr, p_len, p_dummy))
        g_v_mask = self.refine_node_weights(ops.si_len_mask(g_ptr, g_len, g_dummy))

        p_side = (pattern, p_v_rep, p_ptr, p_id, p_vl, self.p_enc_net, p_dummy, p_len)
        g_side = (graph, g_v_rep, g_ptr, g_id, g_vl, self.g_enc_net, g_dummy, g_len)
        if self._ragged_head_applies():
            pred_c, pred_v = self._ragged_head(p_side, g_side, p_v_mask, g_v_mask), None
        else:
            pred_c, pred_v = ops.launch_tagged("si_head_padded", lambda: self._padded_head(p_side, g_side, p_v_mask, g_v_mask))

        return OutputDict(
            p_v_emb=p_v_emb, p_e_emb=None, g_v_emb=g_v_emb, g_e_emb=None,
            p_v_rep=p_v_rep, p_e_rep=None, g_v_rep=g_v_rep, g_e_rep=None,
            p_v_mask=p_v_mask, p_e_mask=None, g_v_mask=g_v_mask, g_e_mask=None,
            pred_c=pred_c, pred_v=pred_v, pred_e=None,
        )

    def _ragged_head_applies(self):
        net = self.pred_net
        return ((type(net) in (SumPredictNet, MeanPredictNet, MaxPredictNet)
                 or (isinstance(net, _ATTN_HEADS) and attn_ragged_ok(net, self.training)))
                and net.weight_fc1 is None and not (self.training and net.drop.p > 0)
                and type(self).refine_node_weights is GraphAdjModel.refine_node_weights)

    def _degrees(self, g):
        src, dst = g.all_edges()
        in_deg, out_deg = ops.degrees(_i32(src), _i32(dst), g.number_of_nodes())
        return out_deg, in_deg

    def _addfeat(self, side):
        """The per-row [enc_v | enc_vl | out_deg | in_deg] of basemodel.py:914-932 as dense tensors (Max and padded heads)."""
        g, rep, _, ids, labels, enc_net, _, _ = side
        feats = []
        if self.pred_with_enc:
            feats += [F.embedding(ids.long(), enc_net["v"].weight), F.embedding(labels.long(), enc_net["vl"].weight)]
        if self.pred_with_deg:
            feats += [d.to(rep.dtype).view(-1, 1) for d in self._degrees(g)]
        return feats

    def _ragged_head(self, p_side, g_side, p_v_mask, g_v_mask):
        """PredictNet.forward on the ragged rows.  Sum / Mean: fc is linear, so the padded sum of fc(row) is
        (sum of the unmasked rows) @ W^T + L * b (/ L for Mean).  Max: fc per row, then the per-graph max with b as the
        candidate of the masked positions."""
        net = self.pred_net
        if isinstance(net, _ATTN_HEADS):
            rows = [th.cat(self._addfeat(s) + [s[1]], dim=1) if (self.pred_with_enc or self.pred_with_deg) else s[1]
                    for s in (p_side, g_side)]
            return attn_head_ragged(net, rows[0], p_side[2], p_side[6], p_side[7], p_v_mask.sum(1),
                                    rows[1], g_side[2], g_side[6], g_side[7], g_v_mask.sum(1))
        pooled, counts = [], []
        for side, fc in ((p_side, net.p_fc), (g_side, net.g_fc)):
            g, rep, ptr, ids, labels, enc_net, dummy, L = side
            if isinstance(net, MaxPredictNet):
                rows = th.cat(self._addfeat(side) + [rep], dim=1) if (self.pred_with_enc or self.pred_with_deg) else rep
                y = ops.linear_any(rows.contiguous(), fc.weight, fc.bias)
                pooled.append(ops.si_pool_max(y, fc.bias, ptr, L, dummy))
                counts.append(None)
                continue
            deg = self._degrees(g) if self.pred_with_deg else (None, None)
            enc = (ids, enc_net["v"].weight, labels, enc_net["vl"].weight) if self.pred_with_enc else (None,) * 4
            S, cnt = ops.si_pool_sum(rep, ptr, dummy, *enc, *deg)
            # sum over the padded rows of fc(row): masked rows are zero rows, each gives the bias (pred.py agg_graph)
            p = th.addmm(fc.bias.float() * L, S, fc.weight.float().t())
            if isinstance(net, MeanPredictNet):
                p = p / L
            pooled.append(p.to(rep.dtype))
            counts.append(cnt)
        p, g = pooled
        if counts[0] is None:                                # (Max: no pooled sum carries the counts)
            counts = [p_v_mask.sum(1), g_v_mask.sum(1)]
        dt = p.dtype
        pl, gl = counts[0].to(th.float32).view(-1, 1), counts[1].to(th.float32).view(-1, 1)
        pl_inv, gl_inv = (1.0 / pl).to(dt), (1.0 / gl).to(dt)
        pl, gl = pl.to(dt), gl.to(dt)
        y = net.act(net.pred_fc1(th.cat([p, g, g - p, g * p, pl, gl, pl_inv, gl_inv], dim=1)))
        return net.pred_fc2(th.cat([y, pl, gl, pl_inv, gl_inv], dim=1))

    def _padded_head(self, p_side, g_side, p_v_mask, g_v_mask):
        """basemodel.py:914-962 as written: the concatenated rows padded per graph, masked, through the pred net."""
        outs = []
        for side, mask in ((p_side, p_v_mask), (g_side, g_v_mask)):
            g, rep = side[0], side[1]
            feats = self._addfeat(side)
            out = th.cat(feats + [rep], dim=-1) if feats else rep
            out = split_and_batchify_graph_feats(out, g.batch_num_nodes(), pre_pad=True)[0]
            outs.append(out.masked_fill(~mask.unsqueeze(-1), 0))
        pred_c, pred_v = self.pred_net(outs[0], p_v_mask, outs[1], g_v_mask)
        return pred_c, pred_v

    # ---- expand (basemodel.py:167-219) ----
    def expand(self, **kw):
        """Grow the vocabularies: max_* = max(kw, current); enc nets rebuilt, filter / emb / (pred_with_enc) pred nets rebuilt with
        the old weights copied in front-padded.  A rebuilt module is deleted and re-registered, as in the reference, so it moves to
        the end of the state_dict.  On failure the sizes AND the modules (and their order) are restored."""
        if "base" in kw and kw["base"] != self.base:
            raise ValueError("expand cannot change base (%s -> %s)" % (self.base, kw["base"]))
        if _is_attn_head(self.pred_net):
            raise NotImplementedError("expand: a model that carries an attention head or DIAMNet (set_pred_net) cannot be expanded; "
                                      "expand first, then attach the head")
        kw = dict(kw)
        names = ["max_npv", "max_npvl", "max_npe", "max_npel", "max_ngv", "max_ngvl", "max_nge", "max_ngel"]
        bak = {k: getattr(self, k) for k in names}
        bak_modules = OrderedDict(self._modules)
        bak_plain = {k: self.__dict__[k] for k in ("filter_net",) if k in self.__dict__}     # filter_net None is a plain attribute
        for k in names:
            setattr(self, k, max(kw.get(k, -1), bak[k]))
        try:
            new = self.create_enc_net(type="graph", **kw)
            del self.g_enc_net
            self.g_enc_net = new
            if self.share_enc_net:
                self.p_enc_net = self.g_enc_net
            else:
                new = self.create_enc_net(type="pattern", **kw)
                del self.p_enc_net
                self.p_enc_net = new
            new = self.create_filter_net(**kw)
            if self.filter_net is not None and new is not None:
                expand_dimensions(self.filter_net, new, pre_pad=True)
            del self.filter_net
            self.filter_net = new
            new = self.create_emb_net(type="graph", **kw)
            expand_dimensions(self.g_emb_net, new, pre_pad=True)
            del self.g_emb_net
            self.g_emb_net = new
            if self.share_emb_net:
                self.p_emb_net = self.g_emb_net
            else:
                new = self.create_emb_net(type="pattern", **kw)
                expand_dimensions(self.p_emb_net, new, pre_pad=True)
                del self.p_emb_net
                self.p_emb_net = new
            if self.pred_with_enc:
                new = self.create_pred_net(**kw)
                expand_dimensions(self.pred_net, new, pre_pad=True)
                del self.pred_net
                self.pred_net = new
        except Exception:
            for k, v in bak.items():
                setattr(self, k, v)
            self._modules.clear()
            self._modules.update(bak_modules)
            self.__dict__.update(bak_plain)
            raise


class RGIN(GraphAdjModel):
    """rgin.py:175-260 on RGINRepNet (state_dict g_rep_net.rgin.graph_rgin_(i).*)."""

    def create_rep_net(self, type, **kw):
        if type == "graph":
            num_layers, num_rels = kw.get("rep_num_graph_layers", 1), self.max_ngel
        elif type == "pattern":
            if self.share_rep_net:
                return self.g_rep_net
            num_layers, num_rels = kw.get("rep_num_pattern_layers", 1), self.max_npel
        else:
            raise ValueError
        return RGINRepNet(self.hid_dim, num_rels, num_layers=num_layers, rep_residual=self.rep_residual,
                          regularizer=kw.get("rep_rgin_regularizer", "basis"), num_bases=kw.get("rep_rgin_num_bases", -1),
                          num_mlp_layers=kw.get("rep_rgin_num_mlp_layers", 2), batch_norm=kw.get("rep_rgin_batch_norm", False),
                          act_func=kw.get("rep_act_func", "relu"), dropout=kw.get("rep_dropout", 0.0), name=type)

    def get_pattern_rep(self, pattern, p_emb, mask=None):
        return self.p_rep_net.get_pattern_rep(pattern, p_emb, mask=mask)

    def get_graph_rep(self, graph, g_emb, mask=None, gate=None):
        return self.g_rep_net.get_graph_rep(graph, g_emb, mask=mask, gate=gate)


class RGCN(GraphAdjModel):
    """rgcn.py:215-300 on RGCNRepNet (state_dict g_rep_net.rgcn.graph_rgcn_(i).*)."""

    def create_rep_net(self, type, **kw):
        if type == "graph":
            num_layers, num_rels = kw.get("rep_num_graph_layers", 1), self.max_ngel
        elif type == "pattern":
            if self.share_rep_net:
                return self.g_rep_net
            num_layers, num_rels = kw.get("rep_num_pattern_layers", 1), self.max_npel
        else:
            raise ValueError
        return RGCNRepNet(self.hid_dim, num_rels, num_layers=num_layers, rep_residual=self.rep_residual,
                          regularizer=kw.get("rep_rgcn_regularizer", "basis"), num_bases=kw.get("rep_rgcn_num_bases", -1),
                          edge_norm=kw.get("rep_rgcn_edge_norm", "in"), batch_norm=kw.get("rep_rgcn_batch_norm", False),
                          act_func=kw.get("rep_act_func", "relu"), dropout=kw.get("rep_dropout", 0.0), name=type)

    def get_pattern_rep(self, pattern, p_emb, mask=None):
        return self.p_rep_net.get_pattern_rep(pattern, p_emb, mask=mask)

    def get_graph_rep(self, graph, g_emb, mask=None, gate=None):
        return self.g_rep_net.get_graph_rep(graph, g_emb, mask=mask, gate=gate)
