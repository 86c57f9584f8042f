"""Drop-in conv layers: ``SAGEConv`` and ``GCNConv``.

Same constructor signatures, forward(x, edge_index), reset_parameters(),
sub-module names and state-dict keys as PyG 2.5.1's classes the reference
imports (``sage.py:4``, ``convolution.py:4``):

* SAGEConv: ``lin_l.weight [out,in]``, ``lin_l.bias [out]``, ``lin_r.weight [out,in]``
  out = lin_l(aggr_{j->i} x_j) + lin_r(x_i)          (sage.py:16-19, :34)
* GCNConv(normalize=False): ``lin.weight [out,in]`` (glorot), ``bias [out]`` (zeros)
  out = sum_{j->i} (x W^T)_j + bias                  (convolution.py:19-23, :31)
* GCNConv(normalize=True): same parameters,
  out = D^-1/2 (A + I) D^-1/2 x W^T + bias           (PyG gcn_norm [ext])

``forward`` also accepts a prebuilt :class:`ngnn.block.Block` in place of
``edge_index`` (the model wrappers build one per mini-batch).  On the GPU
(float32 / bfloat16) each conv is ONE autograd node over the hand-written
kernels (ngnn.fused: a one-layer fused stack), so a reference wrapper that
imports these classes instead of PyG's trains without library GEMMs.
"""
from __future__ import annotations

import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from .block import get_block
from .ops import segment_aggregate


class Linear(nn.Module):
    """PyG ``Linear`` init contract [ext]: kaiming_uniform(fan=in, a=sqrt(5))
    weight (or glorot), bias U(+-1/sqrt(in)).  Forward is F.linear."""

    def __init__(self, in_channels: int, out_channels: int, bias: bool = True,
                 weight_initializer: str | None = None):
        super().__init__()
        self.in_channels, self.out_channels = in_channels, out_channels
        self.weight_initializer = weight_initializer
        self.weight = nn.Parameter(torch.empty(out_channels, in_channels))
        if bias:
            self.bias = nn.Parameter(torch.empty(out_channels))
        else:
            self.register_parameter("bias", None)
        self.reset_parameters()

    def reset_parameters(self):
        if self.weight_initializer == "glorot":
            a = math.sqrt(6.0 / (self.weight.size(-2) + self.weight.size(-1)))
            self.weight.data.uniform_(-a, a)
        else:
            bound = math.sqrt(6.0 / ((1 + 5.0) * self.in_channels))
            self.weight.data.uniform_(-bound, bound)
        if self.bias is not None:
            bound = 1.0 / math.sqrt(self.in_channels)
            self.bias.data.uniform_(-bound, bound)

    def forward(self, x):
        return F.linear(x, self.weight, self.bias)

    def extra_repr(self):
        return f"{self.in_channels}, {self.out_channels}, bias={self.bias is not None}"


class SAGEConv(nn.Module):
    def __init__(self, in_channels: int, out_channels: int, aggr: str = "mean",
                 normalize: bool = False, root_weight: bool = True, project: bool = False,
                 bias: bool = True):
        super().__init__()
        if normalize or project or not root_weight or not bias:
            raise NotImplementedError(
                "the reference only uses SAGEConv(in, out) defaults (sage.py:16-19)")
        if aggr not in ("mean", "max", "sum", "add"):
            raise ValueError(f"unsupported aggr {aggr!r}")
        self.in_channels, self.out_channels, self.aggr = in_channels, out_channels, aggr
        self.lin_l = Linear(in_channels, out_channels, bias=True)
        self.lin_r = Linear(in_channels, out_channels, bias=False)

    def reset_parameters(self):
        self.lin_l.reset_parameters()
        self.lin_r.reset_parameters()

    def forward(self, x: torch.Tensor, edge_index) -> torch.Tensor:
        block = get_block(edge_index, x.size(0))
        from . import fused
        needs_grad = torch.is_grad_enabled() and (
            x.requires_grad or any(p.requires_grad for p in self.parameters()))
        if (not needs_grad and x.is_cuda and x.dtype == torch.float32 and x.dim() == 2
                and self.lin_l.weight.dtype == torch.float32):
            # inference (e.g. SAGE.inference, sage.py:52): one fused launch
            aggr = "sum" if self.aggr == "add" else self.aggr
            xc = x if x.stride(1) == 1 else x.contiguous()
            return fused.sage_layer_fwd(xc, block, aggr, self.lin_l.weight, self.lin_l.bias,
                                        self.lin_r.weight, relu=False, p_drop=0.0, seed=0)
        if fused.conv_supported(self, x):
            # the per-conv drop-in (INTEGRATION.md option A: the reference's own
            # wrapper, sage.py:33-39, with this class in place of PyG's): one
            # autograd node on the hand-written kernels -- fused gather +
            # split-bf16 MFMA forward, MFMA weight gradient, narrow-space input
            # gradient -- no library GEMM; relu / dropout stay the wrapper's
            return fused.sage_conv(self, x, block)
        out = self.lin_l(segment_aggregate(x, block, self.aggr))
        return out + self.lin_r(x)

    def __repr__(self):
        return (f"{self.__class__.__name__}({self.in_channels}, {self.out_channels}, "
                f"aggr={self.aggr})")


class GCNConv(nn.Module):
    """PyG 2.5.1 ``GCNConv`` [ext] for a Tensor ``edge_index``.

    ``normalize=False`` (this class's default -- PyG's is ``True``; the
    reference's ``SimpleGCN`` passes ``False`` and existing models rely on
    it): ``out = sum_{j->i} (x W^T)_j + b`` on the fused kernels.
    ``normalize=True``: the Kipf-Welling layer ``D^-1/2 (A + I) D^-1/2 x W^T +
    b`` with ``gcn_norm``'s self-loop rewrite (``add_self_loops=None`` means
    ``= normalize``), degrees counted on the edges passed in.  ``forward``
    takes an optional ``edge_weight`` (fp32 ``[E]``, no gradient) in either
    mode.  The normalised / weighted path is fp32 only and runs eagerly
    (``ngnn.ops.gcn_norm`` + the weighted aggregate kernel, the linear part
    on the hand-written GEMM kernels: no library GEMM)."""

    def __init__(self, in_channels: int, out_channels: int, normalize: bool = False,
                 add_self_loops: bool | None = None, bias: bool = True, improved: bool = False,
                 cached: bool = False, **kwargs):
        super().__init__()
        if add_self_loops is None:
            add_self_loops = bool(normalize)
        if (add_self_loops and not normalize) or not bias:
            raise NotImplementedError(
                "GCNConv: add_self_loops needs normalize=True, and bias=False is not implemented "
                "(the reference uses GCNConv(in, out, normalize=False), convolution.py:19-23)")
        if normalize and improved:
            raise NotImplementedError("GCNConv(normalize=True, improved=True) is not implemented")
        if normalize and cached:
            raise NotImplementedError("GCNConv(normalize=True, cached=True) is not implemented "
                                      "(the norm record is cached per block instead)")
        self.in_channels, self.out_channels = in_channels, out_channels
        self.normalize, self.add_self_loops = bool(normalize), bool(add_self_loops)
        self.lin = Linear(in_channels, out_channels, bias=False, weight_initializer="glorot")
        self.bias = nn.Parameter(torch.zeros(out_channels))

    def reset_parameters(self):
        self.lin.reset_parameters()
        self.bias.data.zero_()

    def forward(self, x: torch.Tensor, edge_index, edge_weight=None) -> torch.Tensor:
        weighted = self.normalize or edge_weight is not None
        if weighted:  # (refused before anything touches the device)
            for name, t in (("x", x), ("lin.weight", self.lin.weight), ("bias", self.bias)):
                if t.dtype != torch.float32:
                    raise TypeError("GCNConv: the normalised / weighted path is float32 only, "
                                    f"{name} is {t.dtype}")
        block = get_block(edge_index, x.size(0))
        from . import fused
        if weighted:
            return self._forward_weighted(x, block, edge_weight)
        if fused.conv_supported(self, x):
            # per-conv drop-in (convolution.py:29-35 with this class in place of
            # PyG's): one autograd node on the hand-written kernels
            return fused.gcn_conv(self, x, block)
        h = self.lin(x)
        return segment_aggregate(h, block, "sum") + self.bias

    def _forward_weighted(self, x, block, edge_weight):
        from . import fused
        from .ops import _gcn_record
        if not x.is_cuda:
            raise RuntimeError("ngnn runs on the GPU only: x is on the CPU")
        if x.dim() != 2:
            raise ValueError(f"x must be 2-D [N, F], got shape {tuple(x.shape)}")
        if x.size(0) != block.n_src:
            raise ValueError(f"x has {x.size(0)} rows but the block has {block.n_src} nodes")
        norm = _gcn_record(block, edge_weight, self.add_self_loops, self.normalize)
        return fused.gcn_weighted_conv(self, x, block, norm)

    def __repr__(self):
        extra = ", normalize=True" if self.normalize else ""
        return f"{self.__class__.__name__}({self.in_channels}, {self.out_channels}{extra})"
