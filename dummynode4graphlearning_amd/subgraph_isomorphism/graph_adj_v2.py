"""The SI count models CompGCN / DMPNN (SURVEY.md 8b "SI model", the dual half): GraphAdjModelV2 with node AND edge
representations, two heads and their length-weighted mix.

Same constructor (the **kw dict of train.py:84-105 build_model), state_dict keys / shapes, initial values under a given
torch.manual_seed, forward(pattern, graph) -> OutputDict and expand(**kw) as subgraph_isomorphism/models/basemodel.py:985-1703,
compgcn.py:289-385 and dmpnn.py:178-277.  The rep stacks are this package's CompGCNLayer / DMPLayer (dual.py, on dn_dual.hip);
the glue around them reuses graph_adj.py's kernels on both sides of the graph:

* dn_si_filter_meta once on the node labels (node_ptr) and once on the edge labels (edge_ptr): gates, padded lengths and the
  id / label checks, both read back in ONE copy per forward;
* code embedding enc[key] @ W per side (dn_si_embed_fwd), with add_edge_id the ids read through src / dst;
* the Sum / Mean head on the ragged rows: node rows as in GraphAdjModel, edge rows
  [enc_v[u] | enc_v[v] | enc_vl[u] | enc_el[e] | enc_vl[v] | out_deg[u] | in_deg[v] | rep] pooled per graph by dn_sie_pool_sum
  without building the concatenation (rows with is_dummy | is_reversed skipped); Max on dn_si_pool_max.

forward has no CPU path; construction, state_dict and expand work on the CPU."""
from collections import OrderedDict

import torch as th
import torch.nn as nn
import torch.nn.functional as F

from .. import ops
from .._lib import DnHipError
from .dl import split_and_batchify_graph_feats
from .dual import CompGCNLayer, DMPLayer
from .attn_pred import build_attn_pred_net
from .graph_adj import (_ATTN_HEADS, _UNSUPPORTED_PRED_NETS, _constructor_refusal, attn_head_ragged, attn_ragged_ok, DUMMYFLAG, EDGELABEL, NODEID, NODELABEL, EquivariantEmbedding, GraphAdjModel,
                        MultihotEmbedding, NormalEmbedding, OrthogonalEmbedding, OutputDict, PositionEmbedding, ScalarFilter,
                        UniformEmbedding, _i32, get_enc_len)
from .pred import MaxPredictNet, MeanPredictNet, SumPredictNet

REVFLAG = "is_reversed"


class GraphAdjModelV2(GraphAdjModel):
    def __init__(self, **kw):
        self.add_edge_id = kw.get("add_edge_id", kw.get("gnn_add_edge_id", False))
        self.node_pred = kw.get("node_pred", True)
        self.edge_pred = kw.get("edge_pred", True)
        super().__init__(**kw)

    # ---- construction (basemodel.py:993-1412) ----
    def create_enc_net(self, type, **kw):
        enc_net = kw.get("enc_net", "Multihot")
        if type == "graph":
            nv, nvl, nel = self.max_ngv, self.max_ngvl, self.max_ngel
        elif type == "pattern":
            if self.share_enc_net:
                return self.g_enc_net
            nv, nvl, nel = self.max_npv, self.max_npvl, self.max_npel
        else:
            raise ValueError
        sizes = OrderedDict((("v", nv), ("vl", nvl), ("el", nel)))
        if enc_net == "Multihot":
            enc = OrderedDict((k, MultihotEmbedding(n, self.base)) for k, n in sizes.items())
        elif enc_net == "Position":
            enc = OrderedDict((k, PositionEmbedding(get_enc_len(n - 1, self.base) * self.base, n)) for k, n in sizes.items())
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
            return nn.ModuleDict({"vl": ScalarFilter(), "el": ScalarFilter()})
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
        net = nn.ModuleDict(OrderedDict((k, classes[emb_net](dims[k], self.hid_dim)) for k in ("v", "vl", "el")))
        with th.no_grad():                              # "rescale because of multi-hot or multi-sinusoid", basemodel.py:1086-1090
            for k in net:
                net[k].weight.div_(dims[k] // self.base)
        return net

    def create_pred_net(self, **kw):
        act_func = kw.get("pred_act_func", "relu")
        dropout = kw.get("pred_dropout", 0.0)
        pred_net = kw.get("pred_net", "SumPredictNet")
        hidden_dim = kw.get("pred_hid_dim", 64)
        return_weights = kw.get("pred_return_weights", "none")
        rep_v_dim, rep_e_dim = self.get_rep_dim()
        classes = {"MeanPredictNet": MeanPredictNet, "SumPredictNet": SumPredictNet, "MaxPredictNet": MaxPredictNet}
        if pred_net in classes:
            cls = classes[pred_net]
            return nn.ModuleDict({
                "v": cls(rep_v_dim, hidden_dim=hidden_dim, act_func=act_func, dropout=dropout,
                         return_weights="node" in return_weights) if self.node_pred else None,
                "e": cls(rep_e_dim, hidden_dim=hidden_dim, act_func=act_func, dropout=dropout,
                         return_weights="edge" in return_weights) if self.edge_pred else None})
        if pred_net in _UNSUPPORTED_PRED_NETS:
            raise NotImplementedError(_constructor_refusal(pred_net))
        raise ValueError(pred_net)

    def set_pred_net(self, pred_net, **kw):
        """GraphAdjModel.set_pred_net for the {"v", "e"} pair of heads (a switched-off side stays a None entry)."""
        return_weights = kw.get("pred_return_weights", "none")
        rep_v_dim, rep_e_dim = self.get_rep_dim()
        new = nn.ModuleDict({
            "v": build_attn_pred_net(pred_net, rep_v_dim, "node" in return_weights, **kw) if self.node_pred else None,
            "e": build_attn_pred_net(pred_net, rep_e_dim, "edge" in return_weights, **kw) if self.edge_pred else None})
        old = next(self.pred_net.parameters())
        new = new.to(device=old.device, dtype=old.dtype)
        del self.pred_net
        self.pred_net = new
        return new

    def get_graph_enc_dims(self):
        return OrderedDict({"v": get_enc_len(self.max_ngv - 1, self.base) * self.base,
                            "vl": get_enc_len(self.max_ngvl - 1, self.base) * self.base,
                            "el": get_enc_len(self.max_ngel - 1, self.base) * self.base})

    def get_pattern_enc_dims(self):
        if self.share_enc_net:
            return self.get_graph_enc_dims()
        return OrderedDict({"v": get_enc_len(self.max_npv - 1, self.base) * self.base,
                            "vl": get_enc_len(self.max_npvl - 1, self.base) * self.base,
                            "el": get_enc_len(self.max_npel - 1, self.base) * self.base})

    @staticmethod
    def _enc_dim(d):
        return d["v"] + d["vl"], (d["v"] + d["vl"]) * 2 + d["el"]

    def get_graph_enc_dim(self):
        return self._enc_dim(self.get_graph_enc_dims())

    def get_pattern_enc_dim(self):
        return self._enc_dim(self.get_pattern_enc_dims())

    def get_rep_dim(self):
        rep_v_dim, rep_e_dim = self.hid_dim, self.hid_dim
        if self.pred_with_enc:
            enc_v_dim, enc_e_dim = self.get_graph_enc_dim()
            rep_v_dim += enc_v_dim
            rep_e_dim += enc_e_dim
        if self.pred_with_deg:
            rep_v_dim += 2
            rep_e_dim += 2
        return rep_v_dim, rep_e_dim

    # ---- representation (CompGCN / DMPNN) ----
    def _layers(self, type):
        raise NotImplementedError

    def get_pattern_rep(self, pattern, p_v_emb, p_e_emb, v_mask=None, e_mask=None):
        v_zero = ~v_mask if v_mask is not None else None
        e_zero = ~e_mask if e_mask is not None else None
        v_out = p_v_emb if v_zero is None else p_v_emb.masked_fill(v_zero, 0.0)
        e_out = p_e_emb if e_zero is None else p_e_emb.masked_fill(e_zero, 0.0)
        for layer in self._layers("pattern"):
            v, e = layer(pattern, v_out, e_out)
            if v_zero is not None:
                v = v.masked_fill(v_zero, 0.0)
            if e_zero is not None:
                e = e.masked_fill(e_zero, 0.0)
            if self.rep_residual and v_out.size() == v.size() and e_out.size() == e.size():
                v_out, e_out = v_out + v, e_out + e
            else:
                v_out, e_out = v, e
        return v_out, e_out

    def get_graph_rep(self, graph, g_v_emb, g_e_emb, v_mask=None, e_mask=None, v_gate=None, e_gate=None):
        if v_mask is not None:
            v_gate = v_mask.to(g_v_emb.dtype) if v_gate is None else v_mask.to(g_v_emb.dtype) * v_gate
        if e_mask is not None:
            e_gate = e_mask.to(g_e_emb.dtype) if e_gate is None else e_mask.to(g_e_emb.dtype) * e_gate
        v_out = g_v_emb if v_gate is None else g_v_emb * v_gate
        e_out = g_e_emb if e_gate is None else g_e_emb * e_gate
        for layer in self._layers("graph"):
            v, e = layer(graph, v_out, e_out)
            if v_gate is not None:
                v = v * v_gate
            if e_gate is not None:
                e = e * e_gate
            if self.rep_residual and v_out.size() == v.size() and e_out.size() == e.size():
                v_out, e_out = v_out + v, e_out + e
            else:
                v_out, e_out = v, e
        return v_out, e_out

    # ---- forward (basemodel.py:1520-1703) ----
    def _embed_edges(self, emb_net, enc_net, el, id_src, id_dst):
        """emb_el(enc_el[label]) (+ emb_v(enc_v[id[src]]) + emb_v(enc_v[id[dst]]) with add_edge_id)."""
        if not self.add_edge_id:
            return ops.si_embed(el, enc_net["el"].weight, emb_net["el"].weight)
        e = ops.si_embed(el, enc_net["el"].weight, emb_net["el"].weight, id_src, enc_net["v"].weight, emb_net["v"].weight)
        return e + ops.si_embed(id_dst, enc_net["v"].weight, emb_net["v"].weight)

    @staticmethod
    def _edge_keys(ids, src, dst):
        """(id[src_e], id[dst_e]) as int32 [E] each: the node-id keys of the edge embedding and of the edge head rows."""
        return ids.index_select(0, src.long()), ids.index_select(0, dst.long())

    @staticmethod
    def _edge_skip(g):
        """is_dummy | is_reversed of the edges as uint8 [E] (None when the batch carries neither flag)."""
        d, r = g.edata.get(DUMMYFLAG), g.edata.get(REVFLAG)
        flags = [t.reshape(-1).bool() for t in (d, r) if t is not None]
        if not flags:
            return None
        return (flags[0] if len(flags) == 1 else flags[0] | flags[1]).view(th.uint8)

    def forward(self, pattern, graph):
        bsz = pattern.batch_size
        if graph.batch_size != bsz:
            raise ValueError("pattern and graph batches differ in size: %d vs %d" % (bsz, graph.batch_size))
        if self.edge_pred and (pattern.number_of_edges() == 0 or graph.number_of_edges() == 0):
            raise ValueError("SI model batch: a batch without edges (edge_pred is on)")
        sides = []
        for g, enc in ((pattern, self.p_enc_net), (graph, self.g_enc_net)):
            src, dst = g.all_edges()
            s = dict(g=g, enc=enc, ptr=g.node_ptr(), eptr=g.edge_ptr(), id=_i32(g.ndata[NODEID]), vl=_i32(g.ndata[NODELABEL]),
                     el=_i32(g.edata[EDGELABEL]), src=_i32(src).contiguous(), dst=_i32(dst).contiguous(),
                     dummy=g.ndata.get(DUMMYFLAG), skip=self._edge_skip(g))
            if s["el"].numel() != s["src"].numel() or s["vl"].numel() != g.number_of_nodes():
                raise DnHipError("SI model batch: one label per node and per edge expected")
            sides.append(s)
        P, G = sides
        dtype = self.g_emb_net["vl"].weight.dtype
        gated = self.filter_net is not None and len(self.filter_net) > 0
        meta_v, vl_gate = ops.si_filter_meta(
            P["ptr"], P["vl"], P["id"], G["ptr"], G["vl"], G["id"],
            (self.p_enc_net["vl"].num_embeddings, self.p_enc_net["v"].num_embeddings),
            (self.g_enc_net["vl"].num_embeddings, self.g_enc_net["v"].num_embeddings), dtype if gated else None)
        # the same rule on the edge labels with the edge lengths (basemodel.py:1434-1442); the "id" slot re-checks the label
        n_pel, n_gel = self.p_enc_net["el"].num_embeddings, self.g_enc_net["el"].num_embeddings
        meta_e, el_gate = ops.si_filter_meta(P["eptr"], P["el"], P["el"], G["eptr"], G["el"], G["el"], (n_pel, n_pel), (n_gel, n_gel),
                                             dtype if gated else None)

        need_ids = self.add_edge_id or (self.edge_pred and self.pred_with_enc)
        for s in sides:
            s["id_src"], s["id_dst"] = self._edge_keys(s["id"], s["src"], s["dst"]) if need_ids else (None, None)
        p_v_emb = self._embed(self.p_emb_net, self.p_enc_net, P["id"], P["vl"], self.add_node_id)
        p_e_emb = self._embed_edges(self.p_emb_net, self.p_enc_net, P["el"], P["id_src"], P["id_dst"])
        g_v_emb = self._embed(self.g_emb_net, self.g_enc_net, G["id"], G["vl"], self.add_node_id)
        g_e_emb = self._embed_edges(self.g_emb_net, self.g_enc_net, G["el"], G["id_src"], G["id_dst"])
        # the forward's one device-to-host read (raises on bad batches)
        (P["L"], G["L"]), (P["Le"], G["Le"]) = ops.si_read_meta_pair(meta_v, meta_e, need_edges=self.edge_pred)

        p_v_rep, p_e_rep = self.get_pattern_rep(pattern, p_v_emb, p_e_emb)
        g_v_rep, g_e_rep = self.get_graph_rep(graph, g_v_emb, g_e_emb, v_gate=vl_gate, e_gate=el_gate)
        P["v_rep"], P["e_rep"], G["v_rep"], G["e_rep"] = p_v_rep, p_e_rep, g_v_rep, g_e_rep

        for s in sides:
            s["v_mask"] = self.refine_node_weights(ops.si_len_mask(s["ptr"], s["L"], s["dummy"]))
            s["e_mask"] = self.refine_edge_weights(ops.si_len_mask(s["eptr"], s["Le"], s["skip"]))
            if self.pred_with_deg:
                s["in_deg"], s["out_deg"] = ops.degrees(s["src"], s["dst"], s["g"].number_of_nodes())

        pred_cv = pred_ce = pred_v = pred_e = None
        if self.node_pred:
            pred_cv, pred_v = self._head("v", P, G)
        if self.edge_pred:
            pred_ce, pred_e = self._head("e", P, G)
        if self.node_pred and self.edge_pred:
            g_v_len = G["v_mask"].float().sum(dim=1).view(-1, 1)
            g_e_len = G["e_mask"].float().sum(dim=1).view(-1, 1)
            g_len = g_v_len + g_e_len
            pred_c = (g_v_len / g_len).to(pred_cv.dtype) * pred_cv + (g_e_len / g_len).to(pred_ce.dtype) * pred_ce
        elif self.node_pred:
            pred_c = pred_cv
        elif self.edge_pred:
            pred_c = pred_ce
        else:
            raise ValueError("node_pred and edge_pred are both off")

        return OutputDict(
            p_v_emb=p_v_emb, p_e_emb=p_e_emb, g_v_emb=g_v_emb, g_e_emb=g_e_emb,
            p_v_rep=p_v_rep, p_e_rep=p_e_rep, g_v_rep=g_v_rep, g_e_rep=g_e_rep,
            p_v_mask=P["v_mask"], p_e_mask=P["e_mask"], g_v_mask=G["v_mask"], g_e_mask=G["e_mask"],
            pred_c=pred_c, pred_v=pred_v, pred_e=pred_e,
        )

    # ---- heads ----
    def _ragged_applies(self, net):
        return ((type(net) in (SumPredictNet, MeanPredictNet, MaxPredictNet)
                 or (isinstance(net, _ATTN_HEADS) and attn_ragged_ok(net, self.training)))
                and net.weight_fc1 is None and not (self.training and net.drop.p > 0)
                and type(self).refine_node_weights is GraphAdjModel.refine_node_weights
                and type(self).refine_edge_weights is GraphAdjModel.refine_edge_weights)

    def _head(self, kind, P, G):
        net = self.pred_net[kind]
        if self._ragged_applies(net):
            return self._ragged(kind, net, P, G), None
        return ops.launch_tagged("si_head_padded", lambda: self._padded(kind, net, P, G))

    def _rows(self, kind, s):
        """The head rows of one side as a dense tensor (Max and padded heads): basemodel.py:1580-1660."""
        rep = s[kind + "_rep"]
        enc = s["enc"]
        feats = []
        if kind == "v":
            if self.pred_with_enc:
                feats += [F.embedding(s["id"].long(), enc["v"].weight), F.embedding(s["vl"].long(), enc["vl"].weight)]
            if self.pred_with_deg:
                feats += [s["out_deg"].to(rep.dtype).view(-1, 1), s["in_deg"].to(rep.dtype).view(-1, 1)]
        else:
            u, v = s["src"].long(), s["dst"].long()
            if self.pred_with_enc:
                vl = s["vl"].long()
                feats += [F.embedding(s["id_src"].long(), enc["v"].weight), F.embedding(s["id_dst"].long(), enc["v"].weight),
                          F.embedding(vl[u], enc["vl"].weight), F.embedding(s["el"].long(), enc["el"].weight),
                          F.embedding(vl[v], enc["vl"].weight)]
            if self.pred_with_deg:
                feats += [s["out_deg"].long()[u].to(rep.dtype).view(-1, 1), s["in_deg"].long()[v].to(rep.dtype).view(-1, 1)]
        return th.cat(feats + [rep], dim=1) if feats else rep

    def _pool_sum(self, kind, s):
        rep, enc = s[kind + "_rep"], s["enc"]
        deg = (s["out_deg"], s["in_deg"]) if self.pred_with_deg else (None, None)
        if kind == "v":
            e = (s["id"], enc["v"].weight, s["vl"], enc["vl"].weight) if self.pred_with_enc else (None,) * 4
            return ops.si_pool_sum(rep, s["ptr"], s["dummy"], *e, *deg)
        e = (s["id"], enc["v"].weight, s["vl"], enc["vl"].weight, s["el"], enc["el"].weight) if self.pred_with_enc else (None,) * 6
        return ops.sie_pool_sum(rep, s["eptr"], s["skip"], s["src"], s["dst"], *e, *deg)

    def _ragged(self, kind, net, P, G):
        """PredictNet.forward on the ragged rows (see GraphAdjModel._ragged_head): Sum / Mean pool the rows first (fc is linear),
        Max applies fc per row and takes the per-graph max with the bias as the candidate of the masked positions."""
        if isinstance(net, _ATTN_HEADS):
            a = []
            for s in (P, G):
                ptr, skip, L = (s["ptr"], s["dummy"], s["L"]) if kind == "v" else (s["eptr"], s["skip"], s["Le"])
                a += [self._rows(kind, s), ptr, skip, L, s[kind + "_mask"].sum(1)]
            return attn_head_ragged(net, *a)
        pooled, counts = [], []
        for s, fc in ((P, net.p_fc), (G, net.g_fc)):
            ptr, skip, L = (s["ptr"], s["dummy"], s["L"]) if kind == "v" else (s["eptr"], s["skip"], s["Le"])
            if isinstance(net, MaxPredictNet):
                y = ops.linear_any(self._rows(kind, s).contiguous(), fc.weight, fc.bias)
                pooled.append(ops.si_pool_max(y, fc.bias, ptr, L, skip))
                counts.append(s[kind + "_mask"].sum(1))
                continue
            S, cnt = self._pool_sum(kind, s)
            p = th.addmm(fc.bias.float() * L, S, fc.weight.float().t())
            if isinstance(net, MeanPredictNet):
                p = p / L
            pooled.append(p.to(s[kind + "_rep"].dtype))
            counts.append(cnt)
        p, g = pooled
        dt = p.dtype
        pl, gl = counts[0].to(th.float32).view(-1, 1), counts[1].to(th.float32).view(-1, 1)
        pl_inv, gl_inv = (1.0 / pl).to(dt), (1.0 / gl).to(dt)
        pl, gl = pl.to(dt), gl.to(dt)
        y = net.act(net.pred_fc1(th.cat([p, g, g - p, g * p, pl, gl, pl_inv, gl_inv], dim=1)))
        return net.pred_fc2(th.cat([y, pl, gl, pl_inv, gl_inv], dim=1))

    def _padded(self, kind, net, P, G):
        """basemodel.py:1597-1667 as written: the concatenated rows padded per graph, masked, through the pred net."""
        outs = []
        for s in (P, G):
            lens = s["g"].batch_num_nodes() if kind == "v" else s["g"].batch_num_edges()
            out = split_and_batchify_graph_feats(self._rows(kind, s), lens, pre_pad=True)[0]
            outs.append(out.masked_fill(~s[kind + "_mask"].unsqueeze(-1), 0))
        return net(outs[0], P[kind + "_mask"], outs[1], G[kind + "_mask"])


class CompGCN(GraphAdjModelV2):
    """compgcn.py:289-385 on CompGCNLayer (state_dict g_rep_net.compgcn.graph_compgcn_(i).*)."""

    def create_rep_net(self, type, **kw):
        if type == "graph":
            num_layers = kw.get("rep_num_graph_layers", 1)
        elif type == "pattern":
            if self.share_rep_net:
                return self.g_rep_net
            num_layers = kw.get("rep_num_pattern_layers", 1)
        else:
            raise ValueError
        layers = nn.ModuleList()
        for i in range(num_layers):
            layers.add_module("%s_compgcn_(%d)" % (type, i), CompGCNLayer(
                self.hid_dim, self.hid_dim, comp_opt=kw.get("rep_compgcn_comp_opt", "mult"),
                edge_norm=kw.get("rep_compgcn_edge_norm", "none"), batch_norm=kw.get("rep_compgcn_batch_norm", False),
                act_func=kw.get("rep_act_func", "relu"), dropout=kw.get("rep_dropout", 0.0)))
        return nn.ModuleDict({"compgcn": layers})

    def _layers(self, type):
        return (self.p_rep_net if type == "pattern" else self.g_rep_net)["compgcn"]


class DMPNN(GraphAdjModelV2):
    """dmpnn.py:178-277 on DMPLayer (state_dict g_rep_net.dmpnn.graph_dmpnn_(i).*)."""

    def create_rep_net(self, type, **kw):
        if type == "graph":
            num_layers = kw.get("rep_num_graph_layers", 1)
        elif type == "pattern":
            if self.share_rep_net:
                return self.g_rep_net
            num_layers = kw.get("rep_num_pattern_layers", 1)
        else:
            raise ValueError
        layers = nn.ModuleList()
        for i in range(num_layers):
            layers.add_module("%s_dmpnn_(%d)" % (type, i), DMPLayer(
                self.hid_dim, self.hid_dim, init_neigenv=kw.get("init_neigenv", 4.0), init_eeigenv=kw.get("init_eeigenv", 4.0),
                num_mlp_layers=kw.get("rep_dmpnn_num_mlp_layers", 2), batch_norm=kw.get("rep_dmpnn_batch_norm", False),
                act_func=kw.get("rep_act_func", "relu"), dropout=kw.get("rep_dropout", 0.0)))
        return nn.ModuleDict({"dmpnn": layers})

    def _layers(self, type):
        return (self.p_rep_net if type == "pattern" else self.g_rep_net)["dmpnn"]
