"""The SI count model DMPLRP (dual message passing + local relational pooling) on the MI355X kernels.

Mirrors of  DMPLRPPoolLayer  subgraph_isomorphism/models/dmplrp.py:19-198
            DMPLRP           subgraph_isomorphism/models/dmplrp.py:201-532
(constructor arguments, parameter names, creation order and initial values under a given torch.manual_seed, state_dict keys
`g_rep_net.DMPLRP.graph_DMPLRP_(i).*`).  A layer is the dual message pass of DMPLayer (dual.py, composed and `ops.dual_fused`
forms) followed by the pooling of LRPLayer over the ego-net sequences of every node -- but with nothing non-linear between the
contraction with lrp_weight and the mean over a node's sequences (dmplrp.py:180-185: no activation, no degree factor).  The mean
is then a weighted sum of table rows, and ops.lrp_pool_linear takes it in one weighted gather-segment-sum over the collapsed index
(ops.LrpIndex.collapsed: per node the distinct rows its sequences touch with their occurrence counts, built on the device from
closed forms; nothing is sized by the number of sequences).  `with ops.lrp_collapsed(False):` pools through
ops.lrp_pool(act="none", factor=None) instead.  The reference's three sparse matrices are not taken: the index is built from the
graph and cached on the batch.  fp32, GPU only for forward."""
import torch as th
import torch.nn as nn

from .. import ops
from .dual import DMPLayer
from .graph_adj_v2 import GraphAdjModelV2
from .init import init_weight
from .lrp import _check_matrix, _check_seq_len


class DMPLRPPoolLayer(DMPLayer):
    def __init__(self, input_dim, hidden_dim, init_neigenv=4.0, init_eeigenv=4.0, lrp_seq_len=4, bias=True, num_mlp_layers=2,
                 batch_norm=True, act_func="relu", dropout=0.0):
        if input_dim != hidden_dim:
            # dmplrp.py:181 views the [P L^2, hidden] rows of the message pass as [P, L^2, input]
            raise ValueError("DMPLRPPoolLayer: input_dim == hidden_dim expected (got %s, %s)" % (input_dim, hidden_dim))
        object.__setattr__(self, "_seq_len", _check_seq_len(lrp_seq_len))          # the hooks below run inside DMPLayer.__init__
        super().__init__(input_dim, hidden_dim, init_neigenv=init_neigenv, init_eeigenv=init_eeigenv, bias=bias,
                         num_mlp_layers=num_mlp_layers, batch_norm=batch_norm, act_func=act_func, dropout=dropout)
        self.lrp_seq_len = self._seq_len
        self.num_rels = 3

    # dmplrp.py:39-53, 75-89: lrp_weight after the six DMP weights, lrp_bias after nbias / ebias, lrp_weight initialised between
    # eloop_weight and the MLPs
    def _create_extra_weights(self):
        self.lrp_weight = nn.Parameter(th.empty(self.input_dim, self.hidden_dim, self._seq_len * self._seq_len))

    def _create_extra_bias(self, bias):
        if bias:
            self.lrp_bias = nn.Parameter(th.zeros(self.hidden_dim))
        else:
            self.register_parameter("lrp_bias", None)

    def _init_extra_weights(self):
        init_weight(self.lrp_weight, init="uniform")

    def forward(self, graph, node_feat, edge_feat, pooling_matrix=None, node_to_perm_matrix=None, edge_to_perm_matrix=None):
        index = None
        for m in (pooling_matrix, node_to_perm_matrix, edge_to_perm_matrix):
            index = _check_matrix(m) or index
        node_out, edge_out = super().forward(graph, node_feat, edge_feat)
        node_out = ops.lrp_pool_linear(node_out, edge_out, self.lrp_weight, self.lrp_bias, index if index is not None else graph,
                                       self.lrp_seq_len, pool="mean")
        return node_out, edge_out

    def extra_repr(self):
        return "\n".join(["in=%s, out=%s" % (self.input_dim, self.hidden_dim), "lrp_seq_len=%s" % self.lrp_seq_len])


class DMPLRP(GraphAdjModelV2):
    """dmplrp.py:201-532 on DMPLRPPoolLayer.  forward(pattern, graph) is the native call; the reference's eight-argument call
    forward(pattern, p_perm_pool, p_n_perm_matrix, p_e_perm_matrix, graph, g_perm_pool, g_n_perm_matrix, g_e_perm_matrix) is
    accepted with None or an ops.LrpIndex in the six matrix positions.  The inherited rep stacks apply the residual of
    dmplrp.py:272-277 / 320-325."""

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
            layers.add_module("%s_DMPLRP_(%d)" % (type, i), DMPLRPPoolLayer(
                self.hid_dim, self.hid_dim, init_neigenv=kw.get("init_neigenv", 4.0), init_eeigenv=kw.get("init_eeigenv", 4.0),
                lrp_seq_len=kw.get("lrp_seq_len", 4), num_mlp_layers=kw.get("rep_dmpnn_num_mlp_layers", 2),
                batch_norm=kw.get("rep_dmpnn_batch_norm", False), act_func=kw.get("rep_act_func", "relu"),
                dropout=kw.get("rep_dropout", 0.0)))
        return nn.ModuleDict({"DMPLRP": layers})

    def _layers(self, type):
        return (self.p_rep_net if type == "pattern" else self.g_rep_net)["DMPLRP"]

    def forward(self, pattern, *args):
        if len(args) == 1:
            return super().forward(pattern, args[0])
        if len(args) != 7:
            raise TypeError("DMPLRP.forward(pattern, graph) or the reference's eight-argument form expected (got %d arguments)"
                            % (len(args) + 1))
        graph = args[3]
        for side, mats in ((pattern, args[0:3]), (graph, args[4:7])):
            for m in mats:
                ix = _check_matrix(m)
                if ix is not None:                                  # a caller-built index: the layers find it on the batch
                    side._cache._lrp[ix.seq_len] = ix
        return super().forward(pattern, graph)
