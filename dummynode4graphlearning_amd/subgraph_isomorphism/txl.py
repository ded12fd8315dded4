"""The TransformerXL count model on edge sequences (subgraph_isomorphism/models/txl.py): TXLFF, TXLAttn, TXLLayer and
TransformerXL(EdgeSeqModel).  DESIGN.md "SI count models: TXL".

A layer is relative-position multi-head attention over [memory | segment] (-> o_net -> residual -> LayerNorm, or LayerNorm first
under pre_lnorm) followed by a two-Linear feed-forward block of the same shape.  The model cuts a sequence into segments of seg_len
rows (the data padded on the RIGHT, the mask on the LEFT, as the reference's segment_data calls do), runs them in order with the last
mem_len rows of every layer's input kept, detached, as the next segment's memory, and returns the last L rows of the concatenation.

Quirks of the reference kept: ext_len = kw.get("seg_len", 0), so passing seg_len switches the memory off; the keys read are seg_len,
mem_len, clamp_len, num_heads, pre_lnorm, rep_dropout, rep_act_func and rep_num_{graph,pattern}_layers (the CLI's rep_txl_* keys are
accepted and ignored); the attention mask of encoder_forward is all ones, so rel_shift's wrapped entries and the padded key rows take
part in the softmax; rep_residual is not used.  decoder_forward / same_length are never reached by the model and are not built.  Any
layer count is allowed (the reference's torch stops at four).

state_dict: g_rep_net._module_dict.txl.graph_txl_(i).attn.{q,k,v,r}_net.weight, ...attn.o_net.{weight,bias}, ...attn.layer_norm.*,
...ff.{layer1,layer2,layer_norm}.*, g_rep_net._param_dict.{r_w_bias,r_r_bias} [heads, hid_dim // heads], pos_emb.weight (frozen).

composed: the segment loop in torch ops (any device and dtype, active dropout, every shape the kernels refuse).  fused: per layer over
the whole padded sequence -- the memory of segment s is rows of the layer's own input, so the loop is a block-banded attention --
with ops.txl_attention (dn_txl.hip) between torch's Linears; `with ops.eseq_fused(on)` picks the path, the TXL layers' own default is
ops.TXL_FUSED_DEFAULT."""
import torch as th
import torch.nn as nn
import torch.nn.functional as F

from .. import ops
from .act import map_activation_str_to_layer
from .edge_seq import EdgeSeqModel
from .graph_adj import PositionEmbedding
from .init import init_module, init_weight


def segment_data(data, max_len, pre_pad=False):
    """utils/dl.py:17-27: pad dimension 1 to a multiple of max_len (on the left when pre_pad) and split."""
    pad_len = max_len - data.size(1) % max_len
    if pad_len != max_len:
        size = list(data.size())
        size[1] = pad_len
        zero_pad = th.zeros(size, device=data.device, dtype=data.dtype)
        data = th.cat([zero_pad, data], dim=1) if pre_pad else th.cat([data, zero_pad], dim=1)
    return th.split(data, max_len, dim=1)


class MixtureDict(nn.Module):
    """The reference container's state_dict prefixes (models/container.py:279): modules under _module_dict, parameters under
    _param_dict; len() counts both."""

    def __init__(self, input=None):
        super().__init__()
        self._module_dict = nn.ModuleDict()
        self._param_dict = nn.ParameterDict()
        for k, v in (input or {}).items():
            self[k] = v

    def __setitem__(self, key, value):
        if isinstance(value, nn.Parameter):
            self._param_dict[key] = value
        else:
            self._module_dict[key] = value

    def __getitem__(self, key):
        if key in self._param_dict:
            return self._param_dict[key]
        if key in self._module_dict:
            return self._module_dict[key]
        raise KeyError(key)

    def __len__(self):
        return len(self._param_dict) + len(self._module_dict)


class TXLFF(nn.Module):
    def __init__(self, input_dim, hid_dim, act_func="relu", dropout=0.0, pre_lnorm=False):
        super().__init__()
        self.input_dim, self.hid_dim, self.pre_lnorm = input_dim, hid_dim, pre_lnorm
        self.layer1 = nn.Linear(input_dim, hid_dim)
        self.layer2 = nn.Linear(hid_dim, input_dim)
        self.act = map_activation_str_to_layer(act_func)
        self.drop = nn.Dropout(dropout)
        self.layer_norm = nn.LayerNorm(input_dim)
        init_module(self.layer1, activation=act_func, init="normal")
        init_module(self.layer2, init="normal")

    def forward(self, x):
        if self.pre_lnorm:
            x = self.layer_norm(x)
        o = self.drop(self.layer2(self.drop(self.act(self.layer1(x))))) + x
        return o if self.pre_lnorm else self.layer_norm(o)

    def get_output_dim(self):
        return self.input_dim


class TXLAttn(nn.Module):
    def __init__(self, input_dim, hid_dim, num_heads=1, dropout=0.0, seg_len=None, ext_len=None, mem_len=None, pre_lnorm=False):
        super().__init__()
        self.input_dim, self.hid_dim, self.num_heads, self.pre_lnorm = input_dim, hid_dim, num_heads, pre_lnorm
        self.scale = 1 / ((hid_dim / num_heads) ** 0.5)
        self.drop = nn.Dropout(dropout)
        self.q_net = nn.Linear(input_dim, hid_dim, bias=False)
        self.k_net = nn.Linear(input_dim, hid_dim, bias=False)
        self.v_net = nn.Linear(input_dim, hid_dim, bias=False)
        self.r_net = nn.Linear(input_dim, hid_dim, bias=False)
        self.o_net = nn.Linear(input_dim, hid_dim)
        self.layer_norm = nn.LayerNorm(input_dim)
        for net in (self.q_net, self.k_net, self.v_net, self.r_net, self.o_net):
            init_module(net, init="normal")

    rel_shift = staticmethod(ops.txl_rel_shift)

    def _close(self, attn_vec, w):
        out = self.drop(self.o_net(attn_vec)) + w
        return out if self.pre_lnorm else self.layer_norm(out)

    def forward(self, w, r, r_w_bias, r_r_bias, attn_mask=None, mems=None):
        """One segment (composed): w [B, qlen, H], r [1, klen, H] the position rows klen - 1 .. 0, mems [B, mlen, H] or None."""
        bsz, qlen, n = w.size(0), w.size(1), self.num_heads
        c = th.cat([mems, w], dim=1) if mems is not None else w
        klen = c.size(1)
        x = w
        if self.pre_lnorm:
            x, c = self.layer_norm(x), self.layer_norm(c)
        r_head_k = self.r_net(r).view(klen, n, -1)
        w_head_q = self.q_net(x).view(bsz, qlen, n, -1)
        w_head_k = self.k_net(c).view(bsz, klen, n, -1)
        w_head_v = self.v_net(c).view(bsz, klen, n, -1)
        AC = th.einsum("bind,bjnd->bijn", w_head_q + r_w_bias, w_head_k)
        BD = self.rel_shift(th.einsum("bind,jnd->bijn", w_head_q + r_r_bias, r_head_k))
        score = (AC + BD) * self.scale
        if attn_mask is not None:
            score = score.masked_fill(~(attn_mask.unsqueeze(-1) if attn_mask.dim() == 3 else attn_mask.unsqueeze(1).unsqueeze(-1)),
                                      float("-inf"))
        prob = self.drop(F.softmax(score, dim=2))
        attn_vec = th.einsum("bijn,bjnd->bind", prob, w_head_v).contiguous().view(bsz, qlen, self.hid_dim)
        return self._close(attn_vec, w)

    def forward_sequence(self, x, rtab, r_w_bias, r_r_bias, seg_len, mem_len):
        """Every segment at once (fused): x [B, Lp, H] the layer's input over the whole padded sequence, rtab [P, H] the position
        rows by relative position.  The memory rows are the input's own rows, detached as data but not as a function of the weights:
        they are projected a second time from x.detach(), so that their gradient reaches k_net, v_net (and layer_norm) and not x."""
        B, Lp, n = x.size(0), x.size(1), self.num_heads

        def _proj():
            xn = self.layer_norm(x) if self.pre_lnorm else x
            q, k, v = (net(xn).view(B, Lp, n, -1) for net in (self.q_net, self.k_net, self.v_net))
            km = vm = None
            if mem_len > 0:
                xd = x.detach()
                xd = self.layer_norm(xd) if self.pre_lnorm else xd
                km, vm = self.k_net(xd).view(B, Lp, n, -1), self.v_net(xd).view(B, Lp, n, -1)
            return q, k, v, km, vm, self.r_net(rtab).view(rtab.size(0), n, -1)

        q, k, v, km, vm, rk = ops.launch_tagged("txl_proj", _proj)
        attn_vec = ops.txl_attention(q, k, v, km, vm, rk, r_w_bias, r_r_bias, seg_len, mem_len, self.scale)
        return ops.launch_tagged("txl_close", lambda: self._close(attn_vec, x))

    def get_output_dim(self):
        return self.input_dim


class TXLLayer(nn.Module):
    def __init__(self, input_dim, hid_dim, num_heads, dropout=0.0, act_func="relu", pre_lnorm=False):
        super().__init__()
        self.attn = TXLAttn(input_dim, hid_dim, num_heads=num_heads, dropout=dropout, pre_lnorm=pre_lnorm)
        self.ff = TXLFF(input_dim, hid_dim, act_func=act_func, dropout=dropout, pre_lnorm=pre_lnorm)

    def forward(self, x, r, r_w_bias, r_r_bias, attn_mask=None, mems=None):
        return self.ff(self.attn(x, r, r_w_bias, r_r_bias, attn_mask=attn_mask, mems=mems))

    def forward_sequence(self, x, rtab, r_w_bias, r_r_bias, seg_len, mem_len):
        o = self.attn.forward_sequence(x, rtab, r_w_bias, r_r_bias, seg_len, mem_len)
        return ops.launch_tagged("txl_ff", lambda: self.ff(o))

    def fused_ok(self, x, seg_len, mem_len):
        """The kernels' predicate for this layer on input x [B, Lp, H] (no active dropout; ops.txl_attention_supported's shapes)."""
        a = self.attn
        d = a.hid_dim // a.num_heads
        return (not (self.training and a.drop.p > 0) and x.is_cuda and x.dtype == th.float32 and a.q_net.weight.dtype == th.float32
                and a.hid_dim == a.input_dim and d * a.num_heads == a.hid_dim and d in ops.TXL_HEAD_WIDTHS
                and seg_len % 16 == 0 and 16 <= seg_len <= ops.TXL_MAX_SEG and mem_len % 16 == 0
                and seg_len + mem_len <= ops.TXL_MAX_WINDOW and x.size(0) * x.size(1) * a.hid_dim * 2 < 2 ** 31)

    def get_output_dim(self):
        return self.ff.get_output_dim()


class TransformerXL(EdgeSeqModel):
    def __init__(self, **kw):
        self.seg_len = kw.get("seg_len", 64)
        self.ext_len = kw.get("seg_len", 0)                         # (sic: txl.py:215)
        self.mem_len = kw.get("mem_len", 64)
        self.clamp_len = kw.get("clamp_len", -1)
        self.max_len = self.seg_len + self.ext_len + self.mem_len
        self.same_length = False
        self.num_heads = kw.get("num_heads", 1)
        super().__init__(**kw)
        self.pos_emb = PositionEmbedding(self.hid_dim, max_len=max(self.clamp_len, self.max_len))
        self.pos_emb.weight.requires_grad = False
        self.drop = nn.Dropout(kw.get("rep_dropout", 0.0))

    def create_rep_net(self, type, **kw):
        if type == "graph":
            num_layers = kw.get("rep_num_graph_layers", 1)
        elif type == "pattern":
            if self.share_rep_net:
                return self.g_rep_net
            num_layers = kw.get("rep_num_pattern_layers", 1)
        else:
            raise ValueError
        num_heads = self.num_heads
        txl = nn.ModuleList()
        for i in range(num_layers):
            txl.add_module("%s_txl_(%d)" % (type, i), TXLLayer(
                self.hid_dim, self.hid_dim, num_heads=num_heads, dropout=kw.get("rep_dropout", 0.0),
                act_func=kw.get("rep_act_func", "relu"), pre_lnorm=kw.get("pre_lnorm", False)))
        r_w_bias = nn.Parameter(th.empty(num_heads, self.hid_dim // num_heads))
        r_r_bias = nn.Parameter(th.empty(num_heads, self.hid_dim // num_heads))
        init_weight(r_w_bias, init="normal")
        init_weight(r_r_bias, init="normal")
        return MixtureDict({"txl": txl, "r_w_bias": r_w_bias, "r_r_bias": r_r_bias})

    # ---- the memory (txl.py:258-288) ----
    def effective_mem_len(self):
        """The rows a segment really sees of its predecessors: update_mems keeps rows [.. - mem_len, mlen + max(0, qlen - ext_len)),
        which is empty whenever ext_len >= seg_len -- that is, whenever seg_len was passed."""
        return self.mem_len if self.mem_len > 0 and self.ext_len < self.seg_len else 0

    def init_mems(self, num_layers, x):
        if self.mem_len > 0:
            return [th.empty((x.size(0), 0, self.hid_dim), dtype=x.dtype, device=x.device) for _ in range(num_layers + 1)]
        return None

    def update_mems(self, hids, mems, mlen, qlen):
        if mems is None:
            return None
        end_idx = mlen + max(0, qlen - 0 - self.ext_len)
        beg_idx = max(0, end_idx - self.mem_len)
        new_mems = []
        for i in range(len(hids)):
            cat = hids[i] if mlen == 0 else th.cat([mems[i], hids[i]], dim=1)
            new_mems.append(cat[:, beg_idx:end_idx].detach())
        return new_mems

    def position_rows(self, n, device):
        """pos_emb at the relative positions 0 .. n - 1, clamped at clamp_len when that is positive: [n, H]."""
        pos = th.arange(n, dtype=th.long, device=device)
        if self.clamp_len > 0:
            pos = pos.clamp(max=self.clamp_len)
        return self.pos_emb(pos)

    def _forward(self, x, x_mask, net, attn_mask=None, mems=None):
        qlen = x.size(1)
        txl, r_w_bias, r_r_bias = net["txl"], net["r_w_bias"], net["r_r_bias"]
        mlen = mems[0].size(1) if mems is not None else 0
        klen = mlen + qlen
        r = self.position_rows(klen, x.device).flip(0).unsqueeze(0)
        x, r = self.drop(x), self.drop(r)
        outputs = [x]
        for i, layer in enumerate(txl):
            m = None if mems is None else mems[i]
            o = layer(outputs[-1], r, r_w_bias, r_r_bias, attn_mask=attn_mask, mems=m).masked_fill(~x_mask, 0.0)
            outputs.append(o)
        return outputs[-1], self.update_mems(outputs, mems, mlen, qlen)

    def encoder_forward(self, enc_inp, enc_mask, enc_net, mems=None):
        qlen = enc_inp.size(1)
        klen = (mems[0].size(1) if mems is not None else 0) + qlen
        attn_mask = th.ones((qlen, klen), dtype=th.bool, device=enc_inp.device).unsqueeze(0)
        return self._forward(enc_inp, enc_mask, enc_net, attn_mask=attn_mask, mems=mems)

    # ---- the two paths ----
    def _rep_composed(self, net, emb, mask):
        segments = segment_data(emb, self.seg_len)
        segmasks = segment_data(mask, self.seg_len, pre_pad=True)
        outputs, mems = [], None
        for i, (seg, m) in enumerate(zip(segments, segmasks)):
            if i == 0:
                mems = self.init_mems(len(net["txl"]), seg)
            o, mems = self.encoder_forward(seg, m, net, mems=mems)
            outputs.append(o)
        return th.cat(outputs, dim=1)[:, -emb.size(1):]

    def _rep_fused(self, net, emb, mask):
        seg, mem = self.seg_len, self.effective_mem_len()
        x = th.cat(segment_data(emb, seg), dim=1)
        m = th.cat(segment_data(mask, seg, pre_pad=True), dim=1)
        rtab = self.position_rows(seg + mem, emb.device)
        for layer in net["txl"]:
            x = layer.forward_sequence(x, rtab, net["r_w_bias"], net["r_r_bias"], seg, mem).masked_fill(~m, 0.0)
        return x[:, -emb.size(1):]

    def _rep(self, net, emb, mask):
        seg, mem = self.seg_len, self.effective_mem_len()
        Lp = -(-emb.size(1) // seg) * seg
        probe = emb.new_empty((emb.size(0), Lp, 0))
        if (ops.txl_fused_enabled() and not (self.training and self.drop.p > 0) and len(net["txl"]) > 0
                and all(layer.fused_ok(probe, seg, mem) for layer in net["txl"])):
            return self._rep_fused(net, emb, mask)
        return ops.launch_tagged("txl_composed", lambda: self._rep_composed(net, emb, mask))

    def get_pattern_rep(self, p_emb, mask=None, lens=None):
        if mask is None:
            mask = th.ones(p_emb.size()[:2] + (1,), dtype=th.bool, device=p_emb.device)
        else:
            p_emb = p_emb.masked_fill(~mask, 0.0)
        return self._rep(self.p_rep_net, p_emb, mask)

    def get_graph_rep(self, g_emb, mask=None, gate=None, lens=None):
        if mask is None:
            mask = th.ones(g_emb.size()[:2] + (1,), dtype=th.bool, device=g_emb.device)
        else:
            g_emb = g_emb.masked_fill(~mask, 0.0)
        if gate is not None:
            g_emb = g_emb * gate
        g_output = self._rep(self.g_rep_net, g_emb, mask)
        return g_output * gate if gate is not None else g_output
