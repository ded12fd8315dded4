"""EdgeSeqModel: the shared part of the SI count models on edge sequences (CNN in cnn.py, RNN in rnn.py, TransformerXL in txl.py).

Same constructor keys, state_dict names / shapes, RNG order, forward(pattern, graph) -> OutputDict (p_e_emb, g_e_emb, p_e_rep,
g_e_rep, p_e_mask, g_e_mask, pred_c, pred_e) and expand(**kw) as subgraph_isomorphism/models/basemodel.py:222-626.  pattern / graph
are EdgeSeq batches (edgeseq.py).  What the model shares with GraphAdjModel -- the embedding classes, create_emb_net, get_rep_dim,
expand, the pooling heads -- is inherited from it; the five-code encoders, the three-label filter, the head's "edge" weights and
the forward are its own.  All tensors stay in rows layout [B, L, C].

Two paths behind `with ops.eseq_fused(on)` (default ops.ESEQ_FUSED_DEFAULT): composed = the reference's arithmetic in torch ops (CPU
tensors too, and every case the kernels refuse); fused = dn_eseq.hip (filter gate, the CNN layers) / dn_eseq_rnn.hip (the RNN layers,
whose own default is ops.ESEQ_RNN_FUSED_DEFAULT) / dn_txl.hip (the TXL layers, ops.TXL_FUSED_DEFAULT) + ops.si_embed.

Quirks of the reference kept: ScalarFilter compares against the pattern's PADDED zeros too (label 0 passes for every pattern shorter
than the longest of the batch); a sequence of length 0 gets an all-ones mask (batch_convert_len_to_mask's `mask[i, :-0]`); the
head sums over all padded positions.  filter_net="None" constructs but its forward raises (basemodel.py:521 dereferences None);
a DUMMYFLAG entry in tdata raises NotImplementedError (basemodel.py:532-539 reads the unbound name p_mask)."""
from collections import OrderedDict

import torch as th
import torch.nn as nn
import torch.nn.functional as F

from .. import ops
from ..edgeseq import DUMMYFLAG, REVFLAG
from .attn_pred import build_attn_pred_net
from .graph_adj import (EquivariantEmbedding, GraphAdjModel, MultihotEmbedding, OutputDict, PositionEmbedding, ScalarFilter,
                        _constructor_refusal, _UNSUPPORTED_PRED_NETS, get_enc_len)
from .pred import MaxPredictNet, MeanPredictNet, SumPredictNet

CODES = ("u", "v", "ul", "el", "vl")


def len_mask(lens, L, device):
    """batch_convert_len_to_mask(lens, pre_pad=True) as [B, L] bool (utils/dl.py:113-127; length 0 -> all ones, as there)."""
    ln = th.as_tensor([l if l > 0 else L for l in lens], dtype=th.long, device=device)
    return th.arange(L, device=device).view(1, L) >= (L - ln).view(-1, 1)


class EdgeSeqModel(GraphAdjModel):
    # ---- construction (basemodel.py:226-450) ----
    def create_enc_net(self, type, **kw):
        enc_net = kw.get("enc_net", "Multihot")
        if type == "graph":
            sizes = (self.max_ngv, self.max_ngv, self.max_ngvl, self.max_ngel, self.max_ngvl)
        elif type == "pattern":
            if self.share_enc_net:
                return self.g_enc_net
            sizes = (self.max_npv, self.max_npv, self.max_npvl, self.max_npel, self.max_npvl)
        else:
            raise ValueError
        if enc_net == "Multihot":
            enc = OrderedDict((k, MultihotEmbedding(n, self.base)) for k, n in zip(CODES, sizes))
        elif enc_net == "Position":
            enc = OrderedDict((k, PositionEmbedding(get_enc_len(n - 1, self.base) * self.base, n)) for k, n in zip(CODES, sizes))
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
            return nn.ModuleDict({k: ScalarFilter() for k in ["ul", "el", "vl"]})
        raise ValueError(filter_net)

    def create_pred_net(self, **kw):
        pred_net = kw.get("pred_net", "SumPredictNet")
        classes = {"MeanPredictNet": MeanPredictNet, "SumPredictNet": SumPredictNet, "MaxPredictNet": MaxPredictNet}
        if pred_net in classes:
            return classes[pred_net](self.get_rep_dim(), hidden_dim=kw.get("pred_hid_dim", 64), act_func=kw.get("pred_act_func", "relu"),
                                     dropout=kw.get("pred_dropout", 0.0), return_weights="edge" in kw.get("pred_return_weights", "none"))
        if pred_net in _UNSUPPORTED_PRED_NETS:
            raise NotImplementedError(_constructor_refusal(pred_net))
        raise ValueError(pred_net)

    def set_pred_net(self, pred_net, **kw):
        """GraphAdjModel.set_pred_net with the sequence models' weights key ("edge" in pred_return_weights)."""
        new = build_attn_pred_net(pred_net, self.get_rep_dim(), "edge" in kw.get("pred_return_weights", "none"), **kw)
        old = next(self.pred_net.parameters())
        new = new.to(device=old.device, dtype=old.dtype)
        del self.pred_net
        self.pred_net = new
        return new

    def _enc_dims(self, sizes):
        return OrderedDict((k, get_enc_len(n - 1, self.base) * self.base) for k, n in zip(CODES, sizes))

    def get_graph_enc_dims(self):
        return self._enc_dims((self.max_ngv, self.max_ngv, self.max_ngvl, self.max_ngel, self.max_ngvl))

    def get_pattern_enc_dims(self):
        if self.share_enc_net:
            return self.get_graph_enc_dims()
        return self._enc_dims((self.max_npv, self.max_npv, self.max_npvl, self.max_npel, self.max_npvl))

    # ---- the pieces of forward ----
    def get_filter_gate(self, pattern, graph):
        """(ul_gate & vl_gate) & el_gate, [B, Lg] bool, or None without a filter (basemodel.py:452-460)."""
        if self.filter_net is None or len(self.filter_net) == 0:
            return None
        labels = (pattern.ul, pattern.el, pattern.vl, graph.ul, graph.el, graph.vl)
        if ops.eseq_fused_enabled() and ops.eseq_filter_supported(*labels, num_labels=max(self.max_ngvl, self.max_ngel,
                                                                                         self.max_npvl, self.max_npel)):
            return ops.eseq_filter_gate(*labels)
        return ops.eseq_filter_gate_composed(*labels)

    def _embed(self, emb_net, enc_net, seq, fused):
        """(enc dict or None, emb [B, L, hid]): the sum over the five codes of emb_net[k](enc_net[k](code_k)) (basemodel.py:462-500)."""
        for m in emb_net.values():
            if isinstance(m, EquivariantEmbedding):
                m.refresh()
        B, L = seq.u.shape
        if fused:
            seq.check_codes(tuple(enc_net[k].num_embeddings for k in CODES))
            keys = [seq.tdata[k].reshape(-1).to(th.int32) for k in CODES]
            t = [(keys[i], enc_net[k].weight, emb_net[k].weight) for i, k in enumerate(CODES)]
            emb = ops.si_embed(*t[0], *t[1]) + ops.si_embed(*t[2], *t[3]) + ops.si_embed(*t[4])
            return None, emb.view(B, L, -1)
        enc = OrderedDict((k, enc_net[k](seq.tdata[k])) for k in CODES)
        emb = emb_net["u"](enc["u"]) + emb_net["v"](enc["v"]) + emb_net["ul"](enc["ul"]) + emb_net["el"](enc["el"]) + \
            emb_net["vl"](enc["vl"])
        return enc, emb

    def get_pattern_rep(self, p_emb, mask=None, lens=None):
        raise NotImplementedError

    def get_graph_rep(self, g_emb, mask=None, gate=None, lens=None):
        raise NotImplementedError

    def _addfeat(self, seq, enc, enc_net, mask):
        """[enc_u | enc_v | enc_ul | enc_el | enc_vl | out_deg[u] | in_deg[v]] of basemodel.py:547-590, masked and refined."""
        feats = []
        if self.pred_with_enc:
            feats += [enc[k] if enc is not None else F.embedding(seq.tdata[k], enc_net[k].weight) for k in CODES]
        if self.pred_with_deg:
            num_v = seq.batch_num_nodes().view(-1, 1)
            shift = num_v.max() - num_v
            feats.append(th.gather(seq.out_degrees().float(), 1, seq.u + shift).unsqueeze(-1))
            feats.append(th.gather(seq.in_degrees().float(), 1, seq.v + shift).unsqueeze(-1))
        if not feats:
            return None
        feat = th.cat(feats, dim=-1).masked_fill(~mask, 0)
        return self.refine_edge_weights(feat)

    def forward(self, pattern, graph):
        bsz = pattern.batch_size
        if graph.batch_size != bsz:
            raise ValueError("pattern and graph batches differ in size: %d vs %d" % (bsz, graph.batch_size))
        for name, seq in (("pattern", pattern), ("graph", graph)):
            if DUMMYFLAG in seq.tdata:
                raise NotImplementedError("%s.tdata carries %r: the reference's EdgeSeqModel.forward reads an unbound name there "
                                          "(basemodel.py:534 / 538, `p_mask` / `g_mask`)" % (name, DUMMYFLAG))
        if self.filter_net is None or len(self.filter_net) == 0:
            raise ValueError("the edge-sequence models need filter_net=\"ScalarFilter\": the reference's forward dereferences the "
                             "missing gate (basemodel.py:521)")
        dev = graph.device
        fused = ops.eseq_fused_enabled() and dev.type == "cuda" and self.g_emb_net["u"].weight.dtype in ops.MFMA_DTYPES
        p_lens = pattern.lens if pattern.lens is not None else [pattern.number_of_tuples()]
        g_lens = graph.lens if graph.lens is not None else [graph.number_of_tuples()]
        p_e_mask = len_mask(p_lens, pattern.u.shape[-1], dev).view(bsz, -1, 1)
        g_e_mask = len_mask(g_lens, graph.u.shape[-1], dev).view(bsz, -1, 1)
        el_gate = ops.launch_tagged("eseq_filter", lambda: self.get_filter_gate(pattern, graph)).view(bsz, -1, 1).float()

        p_enc, p_e_emb = ops.launch_tagged("eseq_embed", lambda: self._embed(self.p_emb_net, self.p_enc_net, pattern, fused))
        g_enc, g_e_emb = ops.launch_tagged("eseq_embed", lambda: self._embed(self.g_emb_net, self.g_enc_net, graph, fused))
        p_e_rep = self.get_pattern_rep(p_e_emb, mask=p_e_mask, lens=p_lens)
        g_e_rep = self.get_graph_rep(g_e_emb, mask=g_e_mask, gate=el_gate, lens=g_lens)

        def _tail(p_e_mask, g_e_mask):
            if REVFLAG in pattern.tdata:
                p_e_mask = p_e_mask.masked_fill(pattern.tdata[REVFLAG].view(bsz, -1, 1).bool(), 0)
            if REVFLAG in graph.tdata:
                g_e_mask = g_e_mask.masked_fill(graph.tdata[REVFLAG].view(bsz, -1, 1).bool(), 0)
            p_feat = self._addfeat(pattern, p_enc, self.p_enc_net, p_e_mask)
            g_feat = self._addfeat(graph, g_enc, self.g_enc_net, g_e_mask)
            p_e_mask = self.refine_edge_weights(p_e_mask.float(), use_max=True).bool().view(bsz, -1)
            g_e_mask = self.refine_edge_weights(g_e_mask.float(), use_max=True).bool().view(bsz, -1)
            return p_feat, g_feat, p_e_mask, g_e_mask

        p_feat, g_feat, p_e_mask, g_e_mask = ops.launch_tagged("eseq_mask_refine", lambda: _tail(p_e_mask, g_e_mask))
        p_out = p_e_rep if p_feat is None else th.cat([p_feat, p_e_rep], dim=-1)
        g_out = g_e_rep if g_feat is None else th.cat([g_feat, g_e_rep], dim=-1)
        pred_c, pred_e = ops.launch_tagged("si_head_padded", lambda: self.pred_net(p_out, p_e_mask, g_out, g_e_mask))
        return OutputDict(
            p_v_emb=None, p_e_emb=p_e_emb, g_v_emb=None, g_e_emb=g_e_emb,
            p_v_rep=None, p_e_rep=p_e_rep, g_v_rep=None, g_e_rep=g_e_rep,
            p_v_mask=None, p_e_mask=p_e_mask, g_v_mask=None, g_e_mask=g_e_mask,
            pred_c=pred_c, pred_v=None, pred_e=pred_e,
        )
