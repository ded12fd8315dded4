"""The SI count model LRP (local relational pooling) on the MI355X kernels.

Mirrors of  LRPLayer  subgraph_isomorphism/models/lrp.py:18-96
            LRP       subgraph_isomorphism/models/lrp.py:99-419
(constructor arguments, parameter names, creation order and initial values under a given torch.manual_seed, state_dict keys
`g_rep_net.lrp.graph_lrp_(i).*`).  The reference feeds every layer three sparse matrices that LRPDataset builds on the host
(dataset.py:1750-1886): node_to_perm / edge_to_perm scatter rows into a dense [P L^2, in] tensor (P = all ordered selections of up
to L - 1 out-neighbours of every node), the einsum with weight [in, hid, L^2] contracts it, a third product pools the sequences
of a node.  Here the index is built from the graph on the device (ops.LrpIndex, cached on the batch) and the layer is
ops.lrp_pool: the weight row-factorised into a node table and an edge table on the Linear kernels, then either the composed path
(gather_segsum over the materialised index + the segment mean: the default, it measured faster on small egos) or one workgroup
per node that enumerates the node's sequences in the kernel and stores nothing of their number (dn_lrp.hip:
`with ops.lrp_fused():`, and by itself when the sequence list is too long to materialise).  The degree
net, BatchNorm, the optional mlp and dropout stay torch.  fp32, GPU only for forward."""
import torch as th
import torch.nn as nn

from .. import ops
from .act import map_activation_str_to_layer
from .graph_adj_v2 import GraphAdjModelV2
from .init import init_module, init_weight

INDEGREE = "in_deg"
_POOL_ACTS = ("relu", "leaky_relu", "none")


def _check_seq_len(lrp_seq_len):
    if int(lrp_seq_len) not in ops.LRP_SEQ_LENS:
        raise ValueError("lrp_seq_len must be one of %s (got %s)" % (ops.LRP_SEQ_LENS, lrp_seq_len))
    return int(lrp_seq_len)


def _check_matrix(m):
    """A matrix position of the reference's call: None, or an index object of this package; a torch sparse matrix is refused."""
    if isinstance(m, th.Tensor) or (isinstance(m, (tuple, list)) and any(isinstance(t, th.Tensor) for t in m)):
        raise TypeError("LRP takes no permutation matrices: the ego-net index is built from the graph on the device "
                        "(pass None, or the batch's ops.LrpIndex)")
    if m is not None and not isinstance(m, (ops.LrpIndex, ops.LrpPermIndex)):
        raise TypeError("LRP: None or an ops.LrpIndex expected in the matrix positions (got %s)" % type(m).__name__)
    return m if isinstance(m, ops.LrpIndex) else None


class LRPLayer(nn.Module):
    def __init__(self, input_dim=2, hidden_dim=128, lrp_seq_len=4, bias=True, act_func="relu", batch_norm=False, mlp=False,
                 dropout=0.0):
        super().__init__()
        self.lrp_seq_len = _check_seq_len(lrp_seq_len)
        self.input_dim, self.hidden_dim, self.act_func = input_dim, hidden_dim, act_func
        self.weight = nn.Parameter(th.empty(input_dim, hidden_dim, self.lrp_seq_len * self.lrp_seq_len))
        self.degnet_0 = nn.Linear(1, 2 * hidden_dim)
        self.degnet_1 = nn.Linear(2 * hidden_dim, hidden_dim)
        if bias:
            self.bias = nn.Parameter(th.empty(hidden_dim))
        else:
            self.register_parameter("bias", None)
        self.act = map_activation_str_to_layer(act_func)
        if batch_norm:
            self.bn = nn.BatchNorm1d(hidden_dim)
        else:
            self.register_parameter("bn", None)
        if mlp:
            self.mlp = nn.Linear(hidden_dim, hidden_dim)
        else:
            self.register_parameter("mlp", None)
        self.drop = nn.Dropout(dropout)
        init_weight(self.weight, activation=act_func, init="uniform")
        init_module(self.degnet_0, activation=act_func, init="uniform")
        init_module(self.degnet_1, activation=act_func, init="uniform")
        if bias:
            nn.init.zeros_(self.bias)
        if mlp:
            init_module(self.mlp, activation=act_func, init="uniform")

    def forward(self, graph, node_feat, edge_feat, pooling_matrix=None, node_to_perm_matrix=None, edge_to_perm_matrix=None):
        index = None
        for m in (pooling_matrix, node_to_perm_matrix, edge_to_perm_matrix):
            index = _check_matrix(m) or index
        if self.act_func not in _POOL_ACTS:
            raise NotImplementedError("LRPLayer: act_func=%s (the pooling kernels take relu, leaky_relu and none)" % self.act_func)
        if INDEGREE not in graph.ndata:
            graph.ndata[INDEGREE] = graph.in_degrees()
        factor = self.degnet_1(self.act(self.degnet_0(graph.ndata[INDEGREE].float().unsqueeze(1))))
        node_out = ops.lrp_pool(node_feat, edge_feat, self.weight, self.bias, factor, index if index is not None else graph,
                                self.lrp_seq_len, act=self.act_func, pool="mean")
        if self.bn is not None:
            node_out = self.bn(node_out)
        if self.mlp is not None:
            node_out = self.act(self.mlp(node_out))
        return self.drop(node_out), edge_feat

    def extra_repr(self):
        return "\n".join(["in=%s, out=%s" % (self.input_dim, self.hidden_dim), "lrp_seq_len=%s" % self.lrp_seq_len])

    def get_output_dim(self):
        return self.hidden_dim


class LRP(GraphAdjModelV2):
    """lrp.py:99-419 on LRPLayer.  forward(pattern, graph) is the native call; the reference's eight-argument call
    forward(pattern, p_perm_pool, p_n_perm_matrix, p_e_perm_matrix, graph, g_perm_pool, g_n_perm_matrix, g_e_perm_matrix) is
    accepted with None or an ops.LrpIndex in the six matrix positions."""

    def __init__(self, **kw):
        _check_seq_len(kw.get("lrp_seq_len", 4))
        super().__init__(**kw)

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
            layers.add_module("%s_lrp_(%d)" % (type, i), LRPLayer(
                self.hid_dim, self.hid_dim, lrp_seq_len=kw.get("lrp_seq_len", 4), batch_norm=kw.get("rep_lrp_batch_norm", False),
                act_func=kw.get("rep_act_func", "relu"), dropout=kw.get("rep_dropout", 0.0)))
        return nn.ModuleDict({"lrp": layers})

    def _layers(self, type):
        return (self.p_rep_net if type == "pattern" else self.g_rep_net)["lrp"]

    # lrp.py:130-214: the gates as in the other V2 models, but both branches of the rep_residual test append the layer's output
    # as it is (no residual sum), and the edge representation is the (gated) edge embedding every layer passes through
    def get_pattern_rep(self, pattern, p_v_emb, p_e_emb, v_mask=None, e_mask=None, index=None):
        v_zero = ~v_mask if v_mask is not None else None
        e_zero = ~e_mask if e_mask is not None else None
        v_out = p_v_emb if v_zero is None else p_v_emb.masked_fill(v_zero, 0.0)
        e_out = p_e_emb if e_zero is None else p_e_emb.masked_fill(e_zero, 0.0)
        for layer in self._layers("pattern"):
            v_out, e_out = layer(pattern, v_out, e_out, index)
            if v_zero is not None:
                v_out = v_out.masked_fill(v_zero, 0.0)
            if e_zero is not None:
                e_out = e_out.masked_fill(e_zero, 0.0)
        return v_out, e_out

    def get_graph_rep(self, graph, g_v_emb, g_e_emb, v_mask=None, e_mask=None, v_gate=None, e_gate=None, index=None):
        if v_mask is not None:
            v_gate = v_mask.to(g_v_emb.dtype) if v_gate is None else v_mask.to(g_v_emb.dtype) * v_gate
        if e_mask is not None:
            e_gate = e_mask.to(g_e_emb.dtype) if e_gate is None else e_mask.to(g_e_emb.dtype) * e_gate
        v_out = g_v_emb if v_gate is None else g_v_emb * v_gate
        e_out = g_e_emb if e_gate is None else g_e_emb * e_gate
        for layer in self._layers("graph"):
            v_out, e_out = layer(graph, v_out, e_out, index)
            if v_gate is not None:
                v_out = v_out * v_gate
            if e_gate is not None:
                e_out = e_out * e_gate
        return v_out, e_out

    def forward(self, pattern, *args):
        if len(args) == 1:
            return super().forward(pattern, args[0])
        if len(args) != 7:
            raise TypeError("LRP.forward(pattern, graph) or the reference's eight-argument form expected (got %d arguments)"
                            % (len(args) + 1))
        graph = args[3]
        for side, mats in ((pattern, args[0:3]), (graph, args[4:7])):
            for m in mats:
                ix = _check_matrix(m)
                if ix is not None:                                  # a caller-built index: the layers find it on the batch
                    side._cache._lrp[ix.seq_len] = ix
        return super().forward(pattern, graph)
