from .conv import GCNConv, GINConv, RGCNConv, SAGEConv, global_add_pool, global_max_pool, global_mean_pool  # noqa: F401
from .models import GCN, GIN, RGCN, RGIN, GCN_concat_readout, GraphSAGE  # noqa: F401
from .diffpool import DenseSAGEConv, DiffPool, DiffPoolLayer, SAGEConvolutions, dense_diff_pool  # noqa: F401
from . import hgpsl  # noqa: F401  (hgpsl.GCN is the conv of models/hgpsl.py; the package's GCN is the classifier of models.py)
from .hgpsl import HGPSLPool, Sparsemax  # noqa: F401
