from .rgcn import RGCNLayer, RGCNRepNet  # noqa: F401
from .rgin import RGINLayer, RGINRepNet  # noqa: F401
from . import bookkeeping  # noqa: F401
from .dual import CompGCNLayer, DMPLayer  # noqa: F401
from .pred import MaxPredictNet, MeanPredictNet, PredictNet, SumPredictNet, mask_dummy_nodes  # noqa: F401
from .dl import batch_convert_mask_to_start_and_end, split_and_batchify_graph_feats  # noqa: F401
from .act import Sparsemax  # noqa: F401
from .attn_pred import (Attention, DIAMNet, DotAttention, MaxAttnPredictNet, MeanAttnPredictNet,  # noqa: F401
                        SumAttnPredictNet, init_mem)
from .graph_adj import (EquivariantEmbedding, GraphAdjModel, MultihotEmbedding, NormalEmbedding, OrthogonalEmbedding,  # noqa: F401
                        OutputDict, PositionEmbedding, RGCN, RGIN, ScalarFilter, UniformEmbedding)
from .graph_adj_v2 import CompGCN, DMPNN, GraphAdjModelV2  # noqa: F401
from .lrp import LRP, LRPLayer  # noqa: F401
from .dmplrp import DMPLRP, DMPLRPPoolLayer  # noqa: F401
from .hgt import HGT, DecompMultiTransform, HeteroGraphTransLayer  # noqa: F401
from .edge_seq import EdgeSeqModel  # noqa: F401
from .cnn import CNN, CNNLayer  # noqa: F401
from .rnn import RNN, RNNLayer  # noqa: F401
from .txl import TXLFF, MixtureDict, TransformerXL, TXLAttn, TXLLayer  # noqa: F401
from .objective import SIEvalMeter, SIObjective, SITrainMeter, anneal_fn, cyclical_fn, schedule_value  # noqa: F401
