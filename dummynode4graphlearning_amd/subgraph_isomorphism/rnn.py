"""The RNN count model on edge sequences (subgraph_isomorphism/models/rnn.py): RNNLayer and RNN(EdgeSeqModel).

A layer is nn.LSTM / nn.GRU / nn.RNN(batch_first=True, bidirectional) over the whole left-padded batch [B, L, H] (-> LayerNorm)
-> Dropout; hidden width per direction hid_dim // 2 when bidirectional.  The model (DESIGN.md "SI count models: RNN"):

    graph side     x0 = emb * gate, gate = mask * filter gate;  per layer  o = layer(x) * gate,  x = x + o when rep_residual and the
                   widths agree, else x = o
    pattern side   x0 = emb.masked_fill(~mask, 0);  per layer  x = layer(x).masked_fill(~mask, 0)      (the reference always passes a
                   mask, so the pattern side never gets the residual)

Lengths are kept, so refine_edge_weights is EdgeSeqModel's identity.  Pad positions are NOT dead for the recurrence: the biases drive
the state through the left padding and the first live step sees it -- both paths compute them.  rep_rnn_layer_norm is accepted and
ignored (the reference never passes it on to RNNLayer).  state_dict: g_rep_net.rnn.graph_rnn_(i).layer.{weight_ih_l0, weight_hh_l0,
bias_ih_l0, bias_hh_l0} (+ the _reverse set), p_rep_net.rnn.pattern_rnn_(i)....

composed: torch's own module (CPU tensors too).  fused: ops.eseq_rnn (dn_eseq_rnn.hip), one launch per layer forward behind the input
projection, where ops.eseq_rnn_supported holds and the layer has no LayerNorm and no active dropout; `with ops.eseq_fused(on)` picks
the path, the RNN layers' own default is ops.ESEQ_RNN_FUSED_DEFAULT."""
import torch as th
import torch.nn as nn

from .. import ops
from .edge_seq import EdgeSeqModel
from .init import xavier_uniform_init

_RNNS = {"LSTM": nn.LSTM, "GRU": nn.GRU, "RNN": nn.RNN}


class RNNLayer(nn.Module):
    def __init__(self, rep_rnn_type, input_dim, hid_dim, layer_norm=False, bidirectional=False, dropout=0.0):
        super().__init__()
        if rep_rnn_type not in _RNNS:
            raise ValueError("rep_rnn_type must be LSTM, GRU or RNN (got %r)" % (rep_rnn_type,))
        self.rnn_type, self.input_dim, self.hid_dim, self.bidirectional = rep_rnn_type, input_dim, hid_dim, bool(bidirectional)
        self.layer = _RNNS[rep_rnn_type](input_dim, hid_dim // 2 if bidirectional else hid_dim, bidirectional=bidirectional,
                                        batch_first=True)
        self.ln = nn.LayerNorm(hid_dim) if layer_norm else None
        self.drop = nn.Dropout(dropout)
        for names in self.layer._all_weights:                       # init_module(self.layer): utils/init.py:184-190
            for n in names:
                if "weight" in n:
                    xavier_uniform_init(getattr(self.layer, n))
                elif "bias" in n:
                    nn.init.zeros_(getattr(self.layer, n))

    def params(self):
        """The torch module's tensors by name (what ops.eseq_rnn takes)."""
        return {n: getattr(self.layer, n) for names in self.layer._all_weights for n in names}

    def fused_ok(self, x):
        return (self.ln is None and not (self.training and self.drop.p > 0)
                and ops.eseq_rnn_supported(x, self.params(), self.rnn_type, self.bidirectional))

    def forward(self, x):
        """The layer on [B, L, H] (composed: torch's module).  On the GPU the module runs on ops.eseq_rnn_composed_backend(); in
        eval mode with gradients wanted it runs on torch's native kernels whatever that says, because torch refuses MIOpen's RNN
        backward outside training mode."""
        native = None
        if not x.is_cuda:
            native = False
        elif not self.training and th.is_grad_enabled():
            native = True
        with ops.eseq_rnn_composed_backend(native):
            o = self.layer(x)[0]
        if self.ln is not None:
            o = self.ln(o)
        return self.drop(o)

    def get_output_dim(self):
        return self.hid_dim - self.hid_dim % 2


class RNN(EdgeSeqModel):
    def create_rep_net(self, type, **kw):
        if type == "graph":
            num_layers = kw.get("rep_num_graph_layers", 1)
        elif type == "pattern":
            if self.share_rep_net:
                return self.g_rep_net
            num_layers = kw.get("rep_num_pattern_layers", 1)
        else:
            raise ValueError
        rnn = nn.ModuleList()
        for i in range(num_layers):
            rnn.add_module("%s_rnn_(%d)" % (type, i), RNNLayer(
                kw.get("rep_rnn_type", "LSTM"), self.hid_dim, self.hid_dim, bidirectional=kw.get("rep_rnn_bidirectional", False),
                dropout=kw.get("rep_dropout", 0.0)))
        return nn.ModuleDict({"rnn": rnn})

    def _rep(self, net, emb, gate, lens, residual):
        """rnn.py:86-124: emb [B, L, H], gate [B, L, 1] float, lens: the host lengths (every gate entry left of a sequence is 0)."""
        L = emb.shape[1]
        lens = [l if l > 0 else L for l in lens]
        x, gated = emb, False
        for layer in net["rnn"]:
            if ops.eseq_rnn_fused_enabled() and layer.fused_ok(x):
                x = ops.eseq_rnn(x, lens, layer.params(), gate, layer.rnn_type, layer.bidirectional, residual)
                gated = True                                        # (x * gate * gate == x * gate: the op gates its input itself)
                continue
            if not gated:
                x, gated = x * gate, True
            o = ops.launch_tagged("eseq_rnn_composed", lambda: layer(x)) * gate
            x = x + o if residual and o.size() == x.size() else o
        return x if gated else x * gate

    def get_pattern_rep(self, p_emb, mask=None, lens=None):
        return self._rep(self.p_rep_net, p_emb, mask.float(), lens, False)

    def get_graph_rep(self, g_emb, mask=None, gate=None, lens=None):
        return self._rep(self.g_rep_net, g_emb, mask.float() * gate, lens, self.rep_residual)
