"""The attention count heads and DIAMNet (the heads pred.py left out).

Mirror of subgraph_isomorphism/models/pred.py:240-640 (Attention, DotAttention, Mean / Sum / MaxAttnPredictNet) and :643-760,
:1043-1328 (init_mem for mean | sum | max, DIAMNet): same constructors, parameter names (`weight_q weight_k weight_v weight_o g_net`,
the layer norms, `p_attn g_attn m_attn mem_layer`), registration order -- hence the same state_dict order and, under one
torch.manual_seed, the same initial bits -- and the same `forward(p_rep, p_mask, g_rep, g_mask) -> (y, w)` on padded tensors.
This file is the plain-torch ("composed") path; the SI models run the same steps on the ragged rows through ops.seg_attention /
ops.seg_window_pool (graph_adj.py) where their conditions hold.

Quirks of the reference that are kept:

* `init_weight(<nn.Module>)` does nothing there, so `g_net.weight`, DIAMNet's `pred_fc1` / `weight_fc1` keep nn.Linear's own initial
  values (those lines are not repeated here: they draw nothing); `g_net.bias` is set to 1, and then EVERY parameter of p_attn / g_attn
  / m_attn -- g_net and its bias included -- is re-drawn by the identity init, in parameters() order;
* the heads sum / average / take the max over ALL padded positions;
* DIAMNet with return_weights feeds `weight_fc1` (built for mem_len * hidden + 2 inputs) 4 * hidden + 2 values: it only runs with
  mem_len = 4; without return_weights `p_fc`, `g_fc` and `m_attn` are never used and get no gradient;
* a masked row inside [start, end] of a DIAMNet window is a zero row: it counts in the mean and is a candidate of the max.

`mem_init` in attn | lstm | circular_* is refused with NotImplementedError."""
import torch as th
import torch.nn as nn

from .act import map_activation_str_to_layer
from .dl import batch_convert_mask_to_start_and_end
from .init import init_weight
from .pred import PredictNet

_INF = -1e30                                              # constants.py:7
MEM_INITS = ("mean", "sum", "max")
_REFUSED_MEM_INITS = ("attn", "lstm", "circular_mean", "circular_sum", "circular_max", "circular_attn", "circular_lstm")


class Attention(nn.Module):
    """pred.py:240-403.  query [bsz, qlen, query_dim], key / value [bsz, klen, key_dim / value_dim], masks [bsz, qlen] / [bsz, klen]."""

    def __init__(self, query_dim, key_dim, value_dim, hidden_dim, num_heads=1, scale=1, score_func="softmax", add_zero_attn=False,
                 add_gate=False, add_residual=False, pre_lnorm=False, post_lnorm=False, dropout=0.0):
        super().__init__()
        self.query_dim, self.key_dim, self.value_dim, self.hidden_dim = query_dim, key_dim, value_dim, hidden_dim
        if hidden_dim == -1 and query_dim % num_heads != 0:
            raise ValueError("Error: query_dim (%d) %% num_heads (%d) should be 0." % (query_dim, num_heads))
        if hidden_dim == -1 and key_dim % num_heads != 0:
            raise ValueError("Error: key_dim (%d) %% num_heads (%d) should be 0." % (key_dim, num_heads))
        if hidden_dim != -1 and hidden_dim % num_heads != 0:
            raise ValueError("Error: hidden_dim (%d) %% num_heads (%d) should be 0." % (hidden_dim, num_heads))
        self.num_heads = num_heads
        self.scale = scale
        self.score_func = score_func
        self.add_zero_attn = add_zero_attn
        self.add_residual = add_residual
        self.pre_lnorm = pre_lnorm
        self.post_lnorm = post_lnorm
        self.drop = nn.Dropout(dropout)
        if hidden_dim != -1:
            self.weight_v = nn.Parameter(th.Tensor(value_dim, hidden_dim))
            self.weight_o = nn.Parameter(th.Tensor(hidden_dim, query_dim))
        else:
            self.register_parameter("weight_v", None)
            self.register_parameter("weight_o", None)
        self.score_act = map_activation_str_to_layer(score_func)
        if hasattr(self.score_act, "dim"):
            self.score_act.dim = 2                        # the key axis of [bsz, qlen, klen, heads]
        self.g_net = nn.Linear(query_dim * 2, query_dim, bias=True) if add_gate else None
        if pre_lnorm:
            self.q_layer_norm = nn.LayerNorm(query_dim)
            self.k_layer_norm = nn.LayerNorm(key_dim)
            self.v_layer_norm = nn.LayerNorm(value_dim)
            self.o_layer_norm = None
        if post_lnorm:                                    # (sic: with both flags the three input norms are dropped again)
            self.q_layer_norm = None
            self.k_layer_norm = None
            self.v_layer_norm = None
            self.o_layer_norm = nn.LayerNorm(query_dim)
        if hidden_dim != -1:
            init_weight(self.weight_v, init="normal")
            init_weight(self.weight_o, init="normal")
        if add_gate:
            nn.init.constant_(self.g_net.bias, 1.0)

    def compute_score(self, query, key, key_mask=None):
        raise NotImplementedError

    def forward(self, query, key, value, query_mask=None, key_mask=None):
        bsz, qlen, vlen = query.size(0), query.size(1), value.size(1)
        original_query = query
        if self.add_zero_attn:
            key = th.cat([key, key.new_zeros((bsz, 1) + key.size()[2:])], dim=1)
            value = th.cat([value, value.new_zeros((bsz, 1) + value.size()[2:])], dim=1)
            vlen += 1
            if key_mask is not None:
                key_mask = th.cat([key_mask, key_mask.new_ones((bsz, 1))], dim=1)
        if self.pre_lnorm and self.q_layer_norm is not None:
            query, key, value = self.q_layer_norm(query), self.k_layer_norm(key), self.v_layer_norm(value)
        attn_score = self.drop(self.compute_score(query, key, key_mask))
        if self.weight_v is not None:
            value = th.matmul(value, self.weight_v)
        value = value.view(bsz, vlen, self.num_heads, -1)
        attn_vec = th.einsum("bijn,bjnd->bind", attn_score, value).contiguous().view(bsz, qlen, -1)
        if query_mask is not None:
            while query_mask.dim() < attn_vec.dim():
                query_mask = query_mask.unsqueeze(-1)
            attn_vec = attn_vec.masked_fill(query_mask == 0, 0)
        if self.weight_o is not None:
            attn_vec = th.matmul(attn_vec, self.weight_o)
        attn_vec = self.drop(attn_vec)
        return self.close(original_query, attn_vec)

    def close(self, original_query, attn_vec):
        """The gate, the residual and the output norm (pred.py:379-391); row-wise, so it serves padded and ragged rows alike."""
        if self.g_net is not None:
            g = th.sigmoid(self.g_net(th.cat([original_query, attn_vec], dim=-1)))
            attn_out = g * original_query + (1 - g) * attn_vec
        else:
            attn_out = attn_vec
        if self.add_residual:
            attn_out = original_query + attn_out
        if self.post_lnorm:
            attn_out = self.o_layer_norm(attn_out)
        return attn_out

    def get_output_dim(self):
        return self.query_dim


class DotAttention(Attention):
    """pred.py:411-487: scaled dot-product scores per head, masked keys at -1e30, softmax or sparsemax over the keys."""

    def __init__(self, query_dim, key_dim, value_dim, hidden_dim, num_heads=1, scale=1, score_func="softmax", add_zero_attn=False,
                 add_gate=False, add_residual=False, pre_lnorm=False, post_lnorm=False, dropout=0.0):
        super().__init__(query_dim, key_dim, value_dim, hidden_dim, num_heads=num_heads, scale=scale, score_func=score_func,
                         add_zero_attn=add_zero_attn, add_gate=add_gate, add_residual=add_residual, pre_lnorm=pre_lnorm,
                         post_lnorm=post_lnorm, dropout=dropout)
        if hidden_dim == -1 and (query_dim != key_dim or query_dim != value_dim):
            raise ValueError("Error: when hidden_dim equals -1, the query, key, and value need the same dimension!")
        if hidden_dim != -1:
            self.weight_q = nn.Parameter(th.Tensor(query_dim, hidden_dim))
            self.weight_k = nn.Parameter(th.Tensor(key_dim, hidden_dim))
            init_weight(self.weight_q, init="normal")
            init_weight(self.weight_k, init="normal")
        else:
            self.register_parameter("weight_q", None)
            self.register_parameter("weight_k", None)

    def compute_score(self, query, key, key_mask=None):
        bsz, qlen, klen = query.size(0), query.size(1), key.size(1)
        if self.weight_q is not None:
            query = th.matmul(query, self.weight_q)
            key = th.matmul(key, self.weight_k)
        query = query.view(bsz, qlen, self.num_heads, -1)
        key = key.view(bsz, klen, self.num_heads, -1)
        attn_score = th.einsum("bind,bjnd->bijn", query, key) * self.scale
        if key_mask is not None:
            attn_score = attn_score.masked_fill(key_mask.view(bsz, 1, klen, 1) == 0, _INF)
        if self.score_act is not None:
            attn_score = self.score_act(attn_score)
        return attn_score


def _head_attention(input_dim, query_dim, hidden_dim, num_heads):
    return DotAttention(query_dim=query_dim, key_dim=input_dim, value_dim=input_dim, hidden_dim=hidden_dim, num_heads=num_heads,
                        scale=1 / (hidden_dim / num_heads) ** 0.5, score_func="sparsemax", add_gate=True, add_residual=False,
                        pre_lnorm=False, post_lnorm=False)


def _identity_redraw(*attns):
    """pred.py:540-546: "make the attention should prefer to output the original"."""
    for attn in attns:
        for param in attn.parameters():
            if param.requires_grad:
                init_weight(param, init="identity")


class BaseAttnPredictNet(PredictNet):
    """pred.py:490-559: infer_steps rounds of (graph rows attend to the pattern rows, then to themselves), then PredictNet."""

    def __init__(self, input_dim, hidden_dim, num_heads=1, max_seq_len=512, infer_steps=3, act_func="relu", dropout=0.0,
                 return_weights=False):
        super().__init__(input_dim, hidden_dim, act_func=act_func, dropout=dropout, return_weights=return_weights)
        self.num_heads = num_heads
        self.infer_steps = infer_steps
        self.p_attn = _head_attention(input_dim, input_dim, hidden_dim, num_heads)
        self.g_attn = _head_attention(input_dim, input_dim, hidden_dim, num_heads)
        _identity_redraw(self.p_attn, self.g_attn)

    def infer_fn(self, g, p, g_mask, p_mask):
        g = self.p_attn(g, p, p, query_mask=g_mask, key_mask=p_mask)
        return self.g_attn(g, g, g, query_mask=g_mask, key_mask=g_mask)

    def forward(self, p_rep, p_mask, g_rep, g_mask):
        g = g_rep
        for _ in range(self.infer_steps):
            g = self.infer_fn(g, p_rep, g_mask, p_mask)
        return super().forward(p_rep, p_mask, g, g_mask)


class MeanAttnPredictNet(BaseAttnPredictNet):
    def agg_graph(self, g_rep, g_mask=None):
        return th.mean(g_rep, dim=1)


class SumAttnPredictNet(BaseAttnPredictNet):
    def agg_graph(self, g_rep, g_mask=None):
        return th.sum(g_rep, dim=1)


class MaxAttnPredictNet(BaseAttnPredictNet):
    def agg_graph(self, g_rep, g_mask=None):
        return th.max(g_rep, dim=1)[0]


def window_shape(seq_len, mem_len):
    """(stride, kernel) of init_mem's pooling windows for seq_len > mem_len (pred.py:714-715)."""
    stride = seq_len // mem_len
    return stride, seq_len - (mem_len - 1) * stride


def init_mem(x, x_mask=None, mem_len=4, mem_init="mean"):
    """pred.py:648-760 for mean | sum | max: x [bsz, L, dim] -> (mem [bsz, mem_len, dim], mem_mask [bsz, mem_len] or None)."""
    if mem_init not in MEM_INITS:
        raise NotImplementedError("mem_init=%s" % mem_init)
    bsz, seq_len = x.size(0), x.size(1)
    if seq_len <= mem_len:
        mem = th.cat([x.new_zeros((bsz, mem_len - seq_len, x.size(2))), x], dim=1)
        mem_mask = None if x_mask is None else th.cat([x_mask.new_zeros((bsz, mem_len - seq_len)), x_mask], dim=1)
        return mem, mem_mask
    stride, kernel = window_shape(seq_len, mem_len)
    win = x.unfold(1, kernel, stride)                     # [bsz, mem_len, dim, kernel]
    if mem_init == "max":
        mem = win.max(dim=-1)[0]
    elif mem_init == "sum":
        mem = win.mean(dim=-1) * kernel
    else:
        mem = win.mean(dim=-1)
    mem_mask = None if x_mask is None else x_mask.bool().unfold(1, kernel, stride).any(dim=-1)
    return mem, mem_mask


class DIAMNet(PredictNet):
    """pred.py:1043-1328 (Liu et al., "Neural Subgraph Isomorphism Counting", arXiv:1912.11589): a memory of mem_len rows pooled from
    the graph rows attends to the pattern and to the graph for infer_steps rounds and is read out flat."""

    def __init__(self, input_dim, hidden_dim, act_func="relu", num_heads=1, max_seq_len=512, infer_steps=1, mem_len=4,
                 mem_init="mean", dropout=0.0, return_weights=False):
        if mem_init not in MEM_INITS:
            if mem_init in _REFUSED_MEM_INITS:
                raise NotImplementedError("DIAMNet: mem_init=%s is not provided by this package (mean, sum and max are)" % mem_init)
            raise ValueError("DIAMNet: unknown mem_init=%s" % mem_init)
        super().__init__(input_dim, hidden_dim, act_func=act_func, dropout=dropout, return_weights=return_weights)
        self.num_heads = num_heads
        self.infer_steps = infer_steps
        self.mem_len = mem_len
        self.mem_init = mem_init
        mem_dim = hidden_dim
        self.mem_layer = nn.Linear(input_dim, mem_dim)
        self.p_attn = _head_attention(input_dim, mem_dim, hidden_dim, num_heads)
        self.g_attn = _head_attention(input_dim, mem_dim, hidden_dim, num_heads)
        self.m_attn = _head_attention(mem_dim, hidden_dim, hidden_dim, num_heads)
        if return_weights:
            del self.weight_fc1
            self.weight_fc1 = nn.Linear(mem_dim * mem_len + 2, hidden_dim)
        del self.pred_fc1
        self.pred_fc1 = nn.Linear(mem_dim * mem_len + 4, hidden_dim)
        _identity_redraw(self.p_attn, self.g_attn, self.m_attn)

    def agg_pattern(self, p_rep, p_mask=None):
        if self.mem_init == "max":
            return th.max(p_rep, dim=1)[0]
        if self.mem_init == "sum":
            return th.sum(p_rep, dim=1)
        return th.mean(p_rep, dim=1)

    def init_memory(self, x, x_mask=None):
        """pred.py:1183-1263.  The reference buckets the batch by (start, end) of the unmasked span so as to pool rows of one length
        together; per sample the result is init_mem of its own rows start .. end, which is what is computed here (one group per
        distinct span)."""
        if x_mask is None:
            mem, mem_mask = init_mem(x, None, self.mem_len, self.mem_init)
            return self.mem_layer(mem), mem_mask
        start, end = batch_convert_mask_to_start_and_end(x_mask)
        spans = th.stack([start, end + 1], dim=1)
        uniq, inv = th.unique(spans, dim=0, return_inverse=True)
        mem = x.new_zeros((x.size(0), self.mem_len, self.mem_layer.out_features))
        mem_mask = th.zeros((x.size(0), self.mem_len), dtype=th.bool, device=x.device)
        for i, (s, e) in enumerate(uniq.tolist()):
            rows = th.nonzero(inv == i).view(-1)
            m, mk = init_mem(x[rows, s:e], x_mask[rows, s:e], self.mem_len, self.mem_init)
            mem = mem.index_copy(0, rows, self.mem_layer(m))
            mem_mask = mem_mask.index_copy(0, rows, mk.bool())
        return mem, mem_mask

    def infer_fn(self, m, p, g, m_mask, p_mask, g_mask):
        m = self.p_attn(m, p, p, query_mask=m_mask, key_mask=p_mask)
        return self.g_attn(m, g, g, query_mask=m_mask, key_mask=g_mask)

    def forward(self, p_rep, p_mask, g_rep, g_mask):
        bsz, g_len = p_mask.size(0), g_mask.size(1)
        pl = p_mask.float().sum(dim=1).view(bsz, 1)
        gl = g_mask.float().sum(dim=1).view(bsz, 1)
        pl_inv, gl_inv = 1.0 / pl, 1.0 / gl
        m, m_mask = self.init_memory(g_rep, g_mask)
        for _ in range(self.infer_steps):
            m = self.infer_fn(m=m, g=g_rep, p=p_rep, m_mask=m_mask, g_mask=g_mask, p_mask=p_mask)
        w = None
        if self.weight_fc1 is not None:
            p = self.m_attn(self.p_fc(p_rep), m, m, p_mask, m_mask)
            p = self.agg_pattern(self.drop(p), p_mask).unsqueeze(1).expand(bsz, g_len, -1)
            g = self.drop(self.m_attn(self.g_fc(g_rep), m, m, g_mask, m_mask))
            ex = lambda t: t.expand(bsz, g_len).unsqueeze(-1)  # noqa: E731
            w = self.act(self.weight_fc1(th.cat([p, g, g - p, g * p, ex(pl), ex(pl_inv)], dim=2)))
            w = self.weight_fc2(th.cat([w, ex(pl), ex(pl_inv)], dim=2)).squeeze(-1)
        y = self.close_memory(m.reshape(bsz, -1), pl, gl, pl_inv, gl_inv)
        return y, w

    def close_memory(self, m_flat, pl, gl, pl_inv, gl_inv):
        y = self.act(self.pred_fc1(th.cat([m_flat, pl, gl, pl_inv, gl_inv], dim=1)))
        return self.pred_fc2(th.cat([y, pl, gl, pl_inv, gl_inv], dim=1))


ATTN_PRED_NETS = {"MeanAttnPredictNet": MeanAttnPredictNet, "SumAttnPredictNet": SumAttnPredictNet,
                  "MaxAttnPredictNet": MaxAttnPredictNet, "DIAMNet": DIAMNet}
REFUSED_PRED_NETS = ("MeanMemAttnPredictNet", "SumMemAttnPredictNet", "MaxMemAttnPredictNet")


def build_attn_pred_net(pred_net, input_dim, return_weights, **kw):
    """The head `pred_net` at input_dim from the keys of the reference's create_pred_net (basemodel.py:296-423), same defaults."""
    if pred_net in REFUSED_PRED_NETS:
        raise NotImplementedError("pred_net=%s is not provided by this package: its init_mem loops over the samples in Python and its "
                                  "attn branch reads an unbound name (DESIGN.md 7)" % pred_net)
    if pred_net not in ATTN_PRED_NETS:
        raise ValueError(pred_net)
    common = dict(hidden_dim=kw.get("pred_hid_dim", 64), act_func=kw.get("pred_act_func", "relu"),
                  num_heads=kw.get("pred_num_heads", 4), infer_steps=kw.get("pred_infer_steps", 1),
                  dropout=kw.get("pred_dropout", 0.0), return_weights=return_weights)
    if pred_net == "DIAMNet":
        common.update(mem_len=kw.get("pred_mem_len", 4), mem_init=kw.get("pred_mem_init", "mean"))
    return ATTN_PRED_NETS[pred_net](input_dim, **common)
