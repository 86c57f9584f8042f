"""ngnn — MI355X-native GraphSAGE / GCN sampled-subgraph aggregation path.

Drop-in for the reference's ``SAGE`` / ``SAGEH`` / ``SAGEPL`` / ``SimpleGCN`` (hhilsber/noise-GNN
``src/models/layers/sage.py``, ``sageH.py``, ``sagePL.py``, ``convolution.py``) and the PyG ``SAGEConv`` /
``GCNConv`` they call, backed by hand-written HIP kernels for gfx950 behind the
C ABI in ``include/ngnn.h``.  GPU only: there is no CPU fallback.
"""
from . import _lib, metrics
from .block import Block, get_block
from .metrics import EpochMeter, split_accuracy
from .models import NGNN, SAGE, SAGEH, SAGEPL, SimpleGCN
from .nn import GCNConv, Linear, SAGEConv
from .noise import flip_label, noise_matrix
from .ops import add_node_noise, batch_norm_act, segment_aggregate, shuffle_pos, topk_rewire

__all__ = ["Block", "get_block", "NGNN", "SAGE", "SAGEH", "SAGEPL", "SimpleGCN", "GCNConv", "Linear", "SAGEConv",
           "add_node_noise", "batch_norm_act", "segment_aggregate", "shuffle_pos", "topk_rewire", "flip_label", "noise_matrix",
           "EpochMeter", "split_accuracy", "metrics", "_lib"]
