"""MI355X-native hot path of HKUST-KnowComp/DummyNode4GraphLearning: dummy-node / edge-to-vertex index builds and
GIN / RGCN / RGIN message passing as hand-written gfx950 HIP kernels behind a C ABI (libdn_hip.so), exposed
through the reference's nn.Module surface.  GPU only -- importing is cheap, every operator raises without the
built library or with CPU tensors."""
from . import graph, ops, transforms, tu_io  # noqa: F401
from .graph import BatchedGraph, GraphBatch  # noqa: F401
from .edgeseq import EdgeSeq  # noqa: F401
from .hipgraph import StepGraph  # noqa: F401
from .loader import BatchLoader, PackedGraphs  # noqa: F401

__version__ = "0.1.0"

_GRAPH_KERNELS = ("GraphKernelData", "wl_colors", "wl_features", "wl_gram_matrices", "normalize_gram", "write_libsvm", "dataset_flags")
_GRAPH_KERNELS_SPGR = ("sp_features", "gr_features", "sp_gram_matrix", "gr_gram_matrix")
_GRAPH_KERNELS_KWL = ("kwl_colors", "kwl_features", "kwl_gram_matrices")
_GRAPH_KERNELS_K3WL = ("k3wl_colors", "k3wl_features", "k3wl_gram_matrices")
_GRAPH_KERNELS_SVM = ("read_gram", "normalize_gram_svm", "split_indices", "kernel_svm_evaluation", "evaluate_dataset", "format_table")


def __getattr__(name):
    # graph_kernels is also a command line (python -m dummynode4graphlearning_amd.graph_kernels): imported on first use, so that
    # runpy does not find the module loaded before it runs it
    if name == "graph_kernels" or name in _GRAPH_KERNELS:
        import importlib
        mod = importlib.import_module(".graph_kernels", __name__)
        return mod if name == "graph_kernels" else getattr(mod, name)
    if name == "graph_kernels_spgr" or name in _GRAPH_KERNELS_SPGR:                # (a command line too)
        import importlib
        mod = importlib.import_module(".graph_kernels_spgr", __name__)
        return mod if name == "graph_kernels_spgr" else getattr(mod, name)
    if name == "graph_kernels_kwl" or name in _GRAPH_KERNELS_KWL:                  # (a command line too)
        import importlib
        mod = importlib.import_module(".graph_kernels_kwl", __name__)
        return mod if name == "graph_kernels_kwl" else getattr(mod, name)
    if name == "graph_kernels_k3wl" or name in _GRAPH_KERNELS_K3WL:                # (a command line too)
        import importlib
        mod = importlib.import_module(".graph_kernels_k3wl", __name__)
        return mod if name == "graph_kernels_k3wl" else getattr(mod, name)
    if name == "graph_kernels_svm" or name in _GRAPH_KERNELS_SVM:                  # (a command line too)
        import importlib
        mod = importlib.import_module(".graph_kernels_svm", __name__)
        return mod if name == "graph_kernels_svm" else getattr(mod, name)
    raise AttributeError("module %r has no attribute %r" % (__name__, name))
