"""The CNN count model on edge sequences (subgraph_isomorphism/models/cnn.py): CNNLayer and CNN(EdgeSeqModel).

A layer is Conv1d -> act -> MaxPool1d(k // stride, 1, padding) (-> BatchNorm1d) -> Dropout; the model gates the embeddings by
mask * filter gate, runs the layers, multiplies every layer's output by the gate pooled through the same two windows and adds the
layer's input when rep_residual and the length is kept.  In rows layout x [B, L, C] (DESIGN.md "SI count models: CNN", formula 1):

    conv[b, t]   = sum_j x0[b, t - p + j] @ W[:, :, j]^T + bias          (zero padding)         L1 = L + 2p - k + 1
    pooled[b, t] = max_j act(conv)[b, t - p + j]                         (-inf padding)         L2 = L1 + 2p - k // stride + 1
    gate'        = winmax(winmax(gate, k, stride, p), k // stride, 1, p)
    y            = pooled * gate'  (+ x0 when rep_residual and L2 == L)

Nothing is transposed to [B, C, L].  state_dict: g_rep_net.cnn.graph_cnn_(i).conv.{weight [C, C, k], bias}, .bn.*.

composed: these formulas in torch ops (CPU tensors too).  fused: ops.eseq_conv_pool, one launch per layer forward, where
ops.eseq_fused_supported holds (no BatchNorm, no active dropout, stride 1, ...); a layer outside it is composed as a whole."""
import torch as th
import torch.nn as nn
import torch.nn.functional as F

from .. import ops
from .act import map_activation_str_to_layer
from .edge_seq import EdgeSeqModel
from .init import calculate_gain, kaiming_normal_init


def _windows(x, k, stride, p, fill):
    """[B, L, D] -> the windows [B, (L + 2p - k) // stride + 1, D, k] along the sequence, `fill` outside it."""
    if x.shape[1] + 2 * p < k:
        raise RuntimeError("CNN: a window of %d positions does not fit a sequence of %d with padding %d" % (k, x.shape[1], p))
    return F.pad(x, (0, 0, p, p), value=fill).unfold(1, k, stride)


def win_max(x, k, stride, p):
    """max_pool1d(kernel k, stride, padding p) along dim 1 of [B, L, D]; ties go to the first slot, as in torch."""
    return _windows(x, k, stride, p, float("-inf")).max(dim=-1)[0]


def win_sum(x, k, stride, p):
    """k * avg_pool1d(kernel k, stride, padding p) along dim 1 of [B, L, D] (zeros outside)."""
    return _windows(x, k, stride, p, 0.0).sum(dim=-1)


def conv_rows(x, weight, bias, stride, p):
    """conv1d(weight [Co, Ci, k], stride, padding p) on rows layout [B, L, Ci] -> [B, L1, Co]."""
    return th.einsum("blcj,ocj->blo", _windows(x, weight.shape[2], stride, p, 0.0), weight) + bias


class CNNLayer(nn.Module):
    def __init__(self, in_channels, out_channels, kernel_size, padding=-1, stride=1, groups=1, dilation=1, batch_norm=True,
                 act_func="relu", dropout=0.0):
        super().__init__()
        self.in_channels, self.out_channels = in_channels, out_channels
        if padding == -1:
            padding = kernel_size // 2
        self.conv = nn.Conv1d(in_channels, out_channels, kernel_size=kernel_size, padding=padding, stride=stride, groups=groups,
                              dilation=dilation)
        self.act_func = act_func
        self.act = map_activation_str_to_layer(act_func, inplace=True)
        self.pool = nn.MaxPool1d(kernel_size=kernel_size // stride, stride=1, padding=padding)
        self.bn = nn.BatchNorm1d(out_channels) if batch_norm else None
        self.drop = nn.Dropout(dropout)
        kaiming_normal_init(self.conv.weight, gain=calculate_gain(act_func))        # init_module(conv, "normal", act_func)
        nn.init.zeros_(self.conv.bias)

    def geometry(self):
        """(k, stride, padding, pool window) as integers."""
        return self.conv.kernel_size[0], self.conv.stride[0], self.conv.padding[0], self.pool.kernel_size

    def fused_ok(self, x):
        k, stride, p, kp = self.geometry()
        return (self.bn is None and not (self.training and self.drop.p > 0)
                and ops.eseq_fused_supported(x, self.conv.weight, p, self.act_func, stride=stride, dilation=self.conv.dilation[0],
                                             groups=self.conv.groups))

    def forward(self, x):
        """The layer on rows layout [B, L, C] (composed)."""
        k, stride, p, kp = self.geometry()
        if self.conv.groups != 1 or self.conv.dilation[0] != 1:
            raise NotImplementedError("CNNLayer: groups / dilation other than 1")
        o = self.act(conv_rows(x, self.conv.weight, self.conv.bias, stride, p))
        o = win_max(o, kp, 1, p)
        if self.bn is not None:
            o = self.bn(o.reshape(-1, o.shape[-1])).view(o.shape)
        return self.drop(o)

    def pool_gate(self, gate, use_max=True):
        """A [B, L, D] tensor through the layer's two windows: max / max (the gate, the masks) or sum / max (the added features)."""
        k, stride, p, kp = self.geometry()
        gate = win_max(gate, k, stride, p) if use_max else win_sum(gate, k, stride, p)
        return win_max(gate, kp, 1, p)

    def get_output_dim(self):
        return self.out_channels


class CNN(EdgeSeqModel):
    def create_rep_net(self, type, **kw):
        if type == "graph":
            num_layers = kw.get("rep_num_graph_layers", 1)
        elif type == "pattern":
            if self.share_rep_net:
                return self.g_rep_net
            num_layers = kw.get("rep_num_pattern_layers", 1)
        else:
            raise ValueError
        geo = []
        for key, dflt in (("rep_cnn_kernel_sizes", 2), ("rep_cnn_paddings", -1), ("rep_cnn_strides", 1)):
            v = kw.get(key, dflt)
            geo.append([v] * num_layers if isinstance(v, int) else list(v))
        cnn = nn.ModuleList()
        for i in range(num_layers):
            cnn.add_module("%s_cnn_(%d)" % (type, i), CNNLayer(
                self.hid_dim, self.hid_dim, kernel_size=geo[0][i], padding=geo[1][i], stride=geo[2][i],
                batch_norm=kw.get("rep_cnn_batch_norm", True), act_func=kw.get("rep_act_func", "relu"), dropout=kw.get("rep_dropout", 0.0)))
        return nn.ModuleDict({"cnn": cnn})

    def _rep(self, net, emb, gate, lens):
        """cnn.py:112-190: emb [B, L, C], gate [B, L, 1] float, lens: the host lengths (every gate entry left of a sequence is 0)."""
        L = emb.shape[1]
        lens = [l if l > 0 else L for l in lens]
        x, gated = emb, False
        for layer in net["cnn"]:
            k, stride, p, kp = layer.geometry()
            if ops.eseq_fused_enabled() and layer.fused_ok(x):
                x, gate = ops.eseq_conv_pool(x, lens, layer.conv.weight, layer.conv.bias, gate, p, layer.act_func, self.rep_residual)
                lens = [min(x.shape[1], l + 2 * p) for l in lens]
                gated = True
                continue
            if not gated:
                x, gated = x * gate, True
            o, gate = ops.launch_tagged("eseq_layer_composed", lambda: (layer(x), layer.pool_gate(gate)))
            o = o * gate
            lens = [o.shape[1]] * len(lens)                                # (a composed layer keeps no support bound)
            x = x + o if self.rep_residual and o.size() == x.size() else o
        return x if gated else x * gate

    def get_pattern_rep(self, p_emb, mask=None, lens=None):
        return self._rep(self.p_rep_net, p_emb, mask.float(), lens)

    def get_graph_rep(self, g_emb, mask=None, gate=None, lens=None):
        return self._rep(self.g_rep_net, g_emb, mask.float() * gate, lens)

    def refine_edge_weights(self, weights, use_max=False):
        """cnn.py:192-237 on [B, L] / [B, L, D]: through every graph layer's two windows (max / max, or window sum / max)."""
        if weights is None:
            return None
        dim, dtype = weights.dim(), weights.dtype
        w = (weights.unsqueeze(-1) if dim == 2 else weights).float()
        for layer in self.g_rep_net["cnn"]:
            w = layer.pool_gate(w, use_max=use_max)
        return (w.squeeze(-1) if dim == 2 else w).to(dtype)
