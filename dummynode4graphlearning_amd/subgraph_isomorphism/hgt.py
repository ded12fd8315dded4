"""The SI count model HGT (heterogeneous graph transformer) on the MI355X kernels.

Mirrors of  DecompMultiTransform   subgraph_isomorphism/models/hgt.py:18-122  (weights: utils/decomp.py:8-43)
            HeteroGraphTransLayer  subgraph_isomorphism/models/hgt.py:125-364
            HGT                    subgraph_isomorphism/models/hgt.py:367-438
(constructor arguments, parameter names, creation order and initial values under a given torch.manual_seed, state_dict keys
`g_rep_net.hgt.graph_hgt_(i).*`, forward(pattern, graph) -> OutputDict).  Reference behaviour that is kept, not fixed:

* DecompMultiTransform turns num_bases <= 0 into regularizer "none", so the default config (`rep_hgt_regularizer="diag"`,
  `rep_hgt_num_bases=-1`) has dense per-node-type q / k / v weights [num_node_types, D * D];
* a_transform is built (it draws from the RNG) and never used: its gradients stay None;
* the node type is ndata["node_type"] if present, else ndata["label"]; the edge type of the logits is edata["edge_type"] if
  present, else edata["label"]; the edge type of the messages is looked up with the NODE data's keys (hgt.py:317-322) and ends
  up as edata["label"] too, because both label keys are the string "label";
* only the single-canonical-etype branch exists for BatchedGraph.

The reference gathers a [d_k, d_k] matrix per edge and head twice (logit, message).  Here the matrices are applied on the
destination side, once per (destination, edge type) PAIR that has an edge (docs/LAB_NOTES.md "SI count models: HGT"):

    logit_e  = <q_dst[h] att[et]^T, k_src[h]> pri[et, h] scale        Qp[pair] = q_dst @ blockdiag(att[r])^T: ONE relation-grouped product
    agg_dst  = sum_r (sum_{e of type r} a_e v_src) @ blockdiag(msg[r])   U[pair] from the attention, ONE grouped product + a segment sum

the q | k | v | loop products are one typed row product (ops.typed_linear: the rows grouped by node label, the regularisers
densified to [T, D, D] as rgin.dense_relation_weights does for relations), and the attention in between -- logits, max-subtracted
softmax over all in-edges of a destination, weighted sums per relation -- is ops.hgt_attention: one launch of dn_hgt.hip forward and
two deterministic launches backward (the default: it measured faster than the spread), or, under `with ops.hgt_fused(False):` and for
other dtypes and widths, torch scatter ops over the same factorisation (the A/B partner).  BatchNorm, activation and dropout stay torch.  GPU only for forward."""
import torch as th
import torch.nn as nn

from .. import ops
from .act import map_activation_str_to_layer
from .graph_adj import GraphAdjModel
from .init import init_weight

NODETYPE, EDGETYPE, NODELABEL, EDGELABEL = "node_type", "edge_type", "label", "label"          # constants.py:22-29
REGULARIZERS = ("none", "basis", "bdd", "diag", "scalar")


def create_decomposed_weights(regularizer, input_dim, output_dim, num_transforms, num_bases=-1):
    """utils/decomp.py:8-43: the parameters of one decomposed transform, created and initialised in the reference's order."""
    assert regularizer in REGULARIZERS
    if num_bases <= 0:
        regularizer = "none"
    if regularizer == "none":
        weights = {"weight": nn.Parameter(th.empty(num_transforms, input_dim * output_dim))}
    elif regularizer == "basis":
        weights = {"w_comp": nn.Parameter(th.empty(num_transforms, num_bases)),
                   "weight": nn.Parameter(th.empty(num_bases, input_dim * output_dim))}
    elif regularizer == "bdd":
        if input_dim % num_bases != 0 or output_dim % num_bases != 0:
            raise ValueError("Feature size must be a multiplier of num_bases (%d)." % num_bases)
        weights = {"weight": nn.Parameter(th.empty(num_transforms, input_dim * output_dim // num_bases))}
    else:
        if input_dim != output_dim:
            raise ValueError("Input size must equal to output size.")
        weights = {"w_comp": nn.Parameter(th.empty(num_transforms, num_bases)),
                   "weight": nn.Parameter(th.empty(num_bases, input_dim if regularizer == "diag" else 1))}
    for w in weights.values():
        init_weight(w, init="uniform")
    return weights


class DecompMultiTransform(nn.Module):
    def __init__(self, input_dim, output_dim, num_transforms, regularizer="basis", num_bases=-1, bias=False):
        super().__init__()
        assert regularizer in REGULARIZERS
        if num_bases <= 0:
            regularizer, num_bases = "none", -1
        self.input_dim, self.output_dim, self.num_transforms = input_dim, output_dim, num_transforms
        self.regularizer, self.num_bases = regularizer, num_bases
        weights = create_decomposed_weights(regularizer, input_dim, output_dim, num_transforms, num_bases)
        if bias:
            self.bias = nn.Parameter(th.empty(output_dim))
            nn.init.zeros_(self.bias)
        else:
            self.register_parameter("bias", None)
        self.weights = nn.ParameterDict(weights)

    def dense_weights(self):
        """[num_transforms, input_dim, output_dim]: the matrix forward() applies to a row of every type."""
        T, I, O = self.num_transforms, self.input_dim, self.output_dim
        w = self.weights["weight"]
        if self.regularizer == "none":
            return w.view(T, I, O)
        if self.regularizer == "basis":
            return th.matmul(self.weights["w_comp"], w).view(T, I, O)
        if self.regularizer == "bdd":
            return ops.block_diag_dense(w.view(T, self.num_bases, I // self.num_bases, O // self.num_bases))
        d = th.matmul(self.weights["w_comp"], w)                             # diag: [T, I]; scalar: [T, 1]
        return th.diag_embed(d.expand(T, I))

    def forward(self, x, xtype):
        if xtype.dtype != th.long and xtype.dtype != th.int32:
            raise NotImplementedError("DecompMultiTransform: integer types expected (soft type mixtures are not built)")
        size = x.size()
        y = ops.typed_linear(x.reshape(-1, self.input_dim), self.dense_weights().to(x.dtype), xtype.reshape(-1))
        y = y.view(size[:-1] + (-1,))
        return y if self.bias is None else y + self.bias

    def get_output_dim(self):
        return self.output_dim

    def extra_repr(self):
        return "\n".join(["in=%d, out=%d, num_transforms=%s," % (self.input_dim, self.output_dim, self.num_transforms),
                          "regularizer=%s, num_bases=%d," % (self.regularizer, self.num_bases)])


class HeteroGraphTransLayer(nn.Module):
    def __init__(self, input_dim, hidden_dim, num_node_types=1, num_edge_types=1, regularizer="basis", num_bases=-1, num_heads=1,
                 self_loop=True, bias=True, batch_norm=False, act_func="relu", dropout=0.0):
        super().__init__()
        self.input_dim, self.hidden_dim = input_dim, hidden_dim
        self.num_node_types, self.num_edge_types = num_node_types, num_edge_types
        self.total_rel = num_node_types * num_edge_types * num_node_types
        self.regularizer, self.num_heads, self.self_loop = regularizer, num_heads, self_loop
        self.scale = (hidden_dim / num_heads) ** -0.5
        if regularizer == "none":
            self.num_bases = -1
        elif regularizer in ("diag", "scalar"):
            self.num_bases = 1
        else:
            self.num_bases = num_bases
        if hidden_dim % num_heads != 0:
            raise ValueError("hidden_dim (%d) must be a multiple of num_heads (%d)" % (hidden_dim, num_heads))
        # creation order as hgt.py:160-194 (the RNG stream: k, q, v, a, then att, msg, loop)
        self.k_transform = DecompMultiTransform(input_dim, hidden_dim, num_node_types, regularizer, num_bases, False)
        self.q_transform = DecompMultiTransform(input_dim, hidden_dim, num_node_types, regularizer, num_bases, False)
        self.v_transform = DecompMultiTransform(input_dim, hidden_dim, num_node_types, regularizer, num_bases, False)
        self.a_transform = DecompMultiTransform(input_dim, hidden_dim, num_node_types, regularizer, num_bases, False)
        d_k = hidden_dim // num_heads
        self.relation_pri = nn.Parameter(th.ones(num_edge_types, num_heads))
        self.relation_att = nn.Parameter(th.empty(num_edge_types, num_heads, d_k, d_k))
        self.relation_msg = nn.Parameter(th.empty(num_edge_types, num_heads, d_k, d_k))
        if self_loop:
            self.loop_weight = nn.Parameter(th.empty(input_dim, hidden_dim))
        else:
            self.register_parameter("loop_weight", None)
        if bias:
            self.bias = nn.Parameter(th.empty(hidden_dim))
        else:
            self.register_parameter("bias", None)
        self.bn = nn.BatchNorm1d(hidden_dim) if batch_norm else None
        self.act = map_activation_str_to_layer(act_func)
        self.drop = nn.Dropout(dropout)
        init_weight(self.relation_att, activation=act_func, init="uniform")
        init_weight(self.relation_msg, activation=act_func, init="uniform")
        if self_loop:
            init_weight(self.loop_weight, activation=act_func, init="uniform")
        if bias:
            nn.init.zeros_(self.bias)

    # ---- the reference's key lookups (hgt.py:220-226, 244-250, 316-322) ----
    @staticmethod
    def _node_type_key(graph):
        return NODETYPE if NODETYPE in graph.ndata else (NODELABEL if NODELABEL in graph.ndata else NODETYPE)

    @staticmethod
    def _edge_type_keys(graph):
        att = EDGETYPE if EDGETYPE in graph.edata else (EDGELABEL if EDGELABEL in graph.edata else EDGETYPE)
        msg = EDGETYPE if EDGETYPE in graph.ndata else (EDGELABEL if EDGELABEL in graph.ndata else EDGETYPE)       # (sic: ndata)
        return att, msg

    def typed_weights(self, dtype=None):
        """[T, in, 3 H (+ H)]: q | k | v (| loop_weight for every type) densified, the operand of the layer's one typed product."""
        parts = [t.dense_weights() for t in (self.q_transform, self.k_transform, self.v_transform)]
        if self.self_loop:
            parts.append(self.loop_weight.unsqueeze(0).expand(self.num_node_types, -1, -1))
        W = th.cat(parts, dim=2)
        return W if dtype is None else W.to(dtype)

    def forward(self, graph, node_feat, edge_feat=None):
        if not isinstance(node_feat, th.Tensor):
            raise NotImplementedError("HeteroGraphTransLayer: a node feature tensor expected (per-type dicts are not built)")
        att_key, msg_key = self._edge_type_keys(graph)
        if att_key != msg_key:
            raise NotImplementedError("HeteroGraphTransLayer: logits typed by edata[%r] but messages by edata[%r]" % (att_key, msg_key))
        nt, et = graph.ndata[self._node_type_key(graph)], graph.edata[att_key]
        H, R, heads = self.hidden_dim, self.num_edge_types, self.num_heads
        tix = graph.type_index(nt, self.num_node_types) if node_feat.is_cuda and hasattr(graph, "type_index") else None
        if hasattr(graph, "hgt_index"):
            index = graph.hgt_index(et, R)
        else:
            src, dst = graph.all_edges()
            index = ops.HgtIndex(src, dst, et, graph.number_of_nodes(), R)
        x = node_feat.contiguous()
        qkvl = ops.typed_linear(x, self.typed_weights(x.dtype), nt, tix)                   # [N, 3 H (+ H)]
        q, k, v = (qkvl[:, i * H:(i + 1) * H].contiguous() for i in range(3))
        dt = x.dtype
        out = ops.hgt_message_pass(q, k, v, self.relation_att.to(dt), self.relation_msg.to(dt), self.relation_pri.to(dt), index, self.scale)
        if self.self_loop:
            out = out + qkvl[:, 3 * H:]
        if self.bias is not None:
            out = out + self.bias
        if self.bn is not None:
            out = self.bn(out)
        return self.drop(self.act(out))

    def extra_repr(self):
        return "\n".join(["in=%d, out=%d," % (self.input_dim, self.hidden_dim),
                          "num_node_types=%d, num_edge_types=%d," % (self.num_node_types, self.num_edge_types),
                          "regularizer=%s, num_bases=%d, num_heads=%d," % (self.regularizer, self.num_bases, self.num_heads),
                          "self_loop=%s, bias=%s," % (self.self_loop, self.bias is not None)])

    def get_output_dim(self):
        return self.hidden_dim


class HGT(GraphAdjModel):
    """hgt.py:367-438 on HeteroGraphTransLayer (state_dict g_rep_net.hgt.graph_hgt_(i).*)."""

    def create_rep_net(self, type, **kw):
        if type == "graph":
            num_layers, num_node_types, num_edge_types = kw.get("rep_num_graph_layers", 1), self.max_ngvl, self.max_ngel
        elif type == "pattern":
            if self.share_rep_net:
                return self.g_rep_net
            num_layers, num_node_types, num_edge_types = kw.get("rep_num_pattern_layers", 1), self.max_npvl, self.max_npel
        else:
            raise ValueError
        layers = nn.ModuleList()
        for i in range(num_layers):
            layers.add_module("%s_hgt_(%d)" % (type, i), HeteroGraphTransLayer(
                self.hid_dim, self.hid_dim, num_node_types=num_node_types, num_edge_types=num_edge_types,
                regularizer=kw.get("rep_hgt_regularizer", "diag"), num_bases=kw.get("rep_hgt_num_bases", -1),
                num_heads=kw.get("rep_hgt_num_heads", 4), batch_norm=kw.get("rep_hgt_batch_norm", False),
                act_func=kw.get("rep_act_func", "relu"), dropout=kw.get("rep_dropout", 0.0)))
        return nn.ModuleDict({"hgt": layers})

    # hgt.py:406-438: no residual; the pattern side is zero-masked only when a mask is given, the graph side is gated every layer
    def get_pattern_rep(self, pattern, p_emb, mask=None):
        zero = ~mask if mask is not None else None
        out = p_emb if zero is None else p_emb.masked_fill(zero, 0.0)
        for layer in self.p_rep_net["hgt"]:
            out = layer(pattern, out)
            if zero is not None:
                out = out.masked_fill(zero, 0.0)
        return out

    def get_graph_rep(self, graph, g_emb, mask=None, gate=None):
        if mask is not None:
            gate = mask.to(g_emb.dtype) if gate is None else mask.to(g_emb.dtype) * gate
        out = g_emb if gate is None else g_emb * gate
        for layer in self.g_rep_net["hgt"]:
            out = layer(graph, out)
            if gate is not None:
                out = out * gate
        return out
