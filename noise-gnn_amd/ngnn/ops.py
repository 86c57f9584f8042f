"""Autograd ops over libngnn (no CPU fallback).

``segment_aggregate(x, block, reduce)`` is the drop-in for PyG 2.5.1's
``MessagePassing.propagate`` with ``message = x_j`` and ``aggr`` in
{'mean', 'sum'/'add', 'max'} over a ``Tensor`` edge_index [ext] — the call the
reference makes inside every conv (``sage.py:34``, ``convolution.py:31``).

Forward: ``ngnn_seg_agg_fwd`` over the target-grouped CSR.
Backward: ``ngnn_seg_agg_bwd`` over the source-grouped CSR (a gather, no
atomics), reproducing torch autograd of ``index_select`` + ``scatter_add_``
(and of ``scatter_reduce_(amax)``: even split over ties, the zero ``self``
counting as a tie when the maximum is 0).
"""
from __future__ import annotations

import weakref

import torch

from . import _lib, _timing
from ._common import device_counter, read_counter, rows_ld
from .block import Block


def _check_features(x: torch.Tensor, name: str = "x") -> torch.Tensor:
    if not x.is_cuda:
        raise RuntimeError(f"ngnn runs on the GPU only: {name} is on the CPU")
    if x.dim() != 2:
        raise ValueError(f"{name} must be 2-D [N, F], got shape {tuple(x.shape)}")
    if x.dtype != torch.float32:
        raise TypeError(f"{name}: only float32 is supported on this path, got {x.dtype}")
    if x.stride(1) != 1 or x.stride(0) < x.size(1):
        x = x.contiguous()
    return x


class _SegmentAggregate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, block: Block, reduce: str):
        x = _check_features(x)
        if x.size(0) != block.n_src:
            raise ValueError(f"x has {x.size(0)} rows but the block has {block.n_src} nodes")
        F = x.size(1)
        out = torch.empty(block.n_dst, F, dtype=x.dtype, device=x.device)
        red = _lib.REDUCE[reduce]
        # algorithmic bytes: gathered rows + col + rowptr + output rows
        nbytes = block.E * (F * 4 + 4) + (block.n_dst + 1) * 4 + block.n_dst * F * 4
        with _timing.span("seg_agg_fwd", nbytes):
            rc = _lib.load().ngnn_seg_agg_fwd(
                _lib.ptr(x), x.stride(0), F, _lib.ptr(block.rowptr), _lib.ptr(block.col),
                block.n_dst, red, _lib.F32, _lib.ptr(out), out.stride(0),
                _lib.stream_handle(x.device))
        _lib.check(rc, "ngnn_seg_agg_fwd")
        ctx.block, ctx.red = block, red
        if red == _lib.REDUCE["max"]:
            ctx.save_for_backward(x, out)
        return out

    @staticmethod
    def backward(ctx, g):
        if not ctx.needs_input_grad[0]:
            return None, None, None
        block, red = ctx.block, ctx.red
        g = _check_features(g, "grad")
        F = g.size(1)
        t = block.transposed()
        gx = torch.empty(block.n_src, F, dtype=g.dtype, device=g.device)
        lib = _lib.load()
        x = agg = ws = None
        ws_bytes = 0
        if red == _lib.REDUCE["max"]:
            x, agg = ctx.saved_tensors
            ws_bytes = lib.ngnn_seg_agg_bwd_workspace_bytes(block.n_dst, F, red)
            ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=g.device)
        # algorithmic bytes: gathered grad rows + col_t + degree lookups + rowptr_t + grad_x
        nbytes = block.E * (F * 4 + 4 + 8) + (block.n_src + 1) * 4 + block.n_src * F * 4
        with _timing.span("seg_agg_bwd", nbytes):
            rc = lib.ngnn_seg_agg_bwd(
                _lib.ptr(g), g.stride(0), F, _lib.ptr(block.rowptr), _lib.ptr(block.col),
                block.n_dst, _lib.ptr(t.rowptr), _lib.ptr(t.col), block.n_src, red, _lib.F32,
                _lib.ptr(x), x.stride(0) if x is not None else F,
                _lib.ptr(agg), agg.stride(0) if agg is not None else F,
                _lib.ptr(gx), gx.stride(0), _lib.ptr(ws), ws_bytes, _lib.stream_handle(g.device))
        _lib.check(rc, "ngnn_seg_agg_bwd")
        return gx, None, None


def segment_aggregate(x: torch.Tensor, block: Block, reduce: str = "mean") -> torch.Tensor:
    if reduce not in _lib.REDUCE:
        raise ValueError(f"unsupported aggregation {reduce!r} (expected mean, sum/add or max)")
    return _SegmentAggregate.apply(x, block, reduce)


# ---- symmetric-normalised GCN: gcn_norm and the weighted aggregate ----

class GCNNorm:
    """What ``gcn_norm`` returns: ``dinv`` / ``loop_w`` (fp32 ``[N]``; None
    when the record normalises nothing / replaces no self-loops), ``w`` (the
    edge weights in target-grouped CSR order, None = ones) and ``w_t()`` (the
    same in source-grouped order, built at its first use: the backward's).
    ``edge_weight`` is the caller's tensor, kept for the cache's identity
    check alone; both orders are built from ``_ew``, its dense copy (the
    kernels read ``E`` consecutive floats).  The block is held weakly: the
    block's cache holds the record, and a strong reference back would keep
    the device arrays until the cycle collector runs."""
    __slots__ = ("_block", "add_self_loops", "normalize", "edge_weight", "_ew", "dinv", "loop_w", "w", "_w_t")

    def __init__(self, block, add_self_loops, normalize, edge_weight, ew, dinv, loop_w, w):
        self._block = weakref.ref(block)
        self.add_self_loops, self.normalize = add_self_loops, normalize
        self.edge_weight, self._ew, self.dinv, self.loop_w, self.w = edge_weight, ew, dinv, loop_w, w
        self._w_t = False

    @property
    def block(self):
        return self._block()

    def w_t(self):
        if self._w_t is False:
            if self._ew is None:
                self._w_t = None
            else:
                block = self.block
                if block is None:
                    raise RuntimeError("gcn_norm: the record's block is gone")
                order = block.edge_order(transposed=True)
                self._w_t = self._ew if order is None else self._ew.index_select(0, order)
        return self._w_t


def _check_edge_weight(edge_weight, block: Block) -> torch.Tensor:
    if not isinstance(edge_weight, torch.Tensor):
        raise TypeError("edge_weight must be a torch.Tensor")
    if not edge_weight.is_cuda:
        raise RuntimeError("ngnn runs on the GPU only: edge_weight is on the CPU")
    if edge_weight.dtype != torch.float32:
        raise TypeError(f"edge_weight: only float32 is supported, got {edge_weight.dtype}")
    if edge_weight.dim() != 1 or edge_weight.numel() != block.E:
        raise ValueError(f"edge_weight must be 1-D with one weight per edge ({block.E}), "
                         f"got shape {tuple(edge_weight.shape)}")
    if edge_weight.device != block.device:
        raise ValueError(f"edge_weight on {edge_weight.device}, the block on {block.device}")
    if edge_weight.requires_grad:
        raise NotImplementedError("edge_weight.requires_grad: there is no gradient to the edge weights")
    return edge_weight


def _gcn_record(block: Block, edge_weight, add_self_loops: bool, normalize: bool) -> GCNNorm:
    """The block's cached record for (add_self_loops, normalize, edge_weight
    identity and version): one ``ngnn_gcn_norm`` launch per block and key."""
    if block.n_src != block.n_dst:
        raise ValueError("gcn_norm needs a square block (sources == targets)")
    ew = None if edge_weight is None else _check_edge_weight(edge_weight, block)
    key = (bool(add_self_loops), bool(normalize), None if ew is None else (id(ew), ew._version))
    hit = block._gcn_norm.get(key)
    if hit is not None and hit.edge_weight is ew:  # (the record holds ew: its id cannot be reused)
        return hit
    w = None
    if ew is not None:
        ew = ew.contiguous()  # (a column of edge_attr: the kernels read consecutive floats)
        order = block.edge_order()
        w = ew if order is None else ew.index_select(0, order)
    dinv = loop_w = None
    N = block.n_dst
    if normalize:
        dinv = torch.empty(N, dtype=torch.float32, device=block.device)
        if add_self_loops:
            loop_w = torch.empty(N, dtype=torch.float32, device=block.device)
        with _timing.span("gcn_norm", block.E * (8 if w is not None else 4) + N * 16):
            rc = _lib.load().ngnn_gcn_norm(_lib.ptr(block.rowptr), _lib.ptr(block.col), _lib.ptr(w), N,
                                           int(bool(add_self_loops)), _lib.ptr(dinv), _lib.ptr(loop_w),
                                           _lib.stream_handle(block.device))
        _lib.check(rc, "ngnn_gcn_norm")
    rec = GCNNorm(block, bool(add_self_loops), bool(normalize), edge_weight, ew, dinv, loop_w, w)
    if len(block._gcn_norm) >= 4:
        block._gcn_norm.clear()
    block._gcn_norm[key] = rec
    return rec


def gcn_norm(block_or_edge_index, edge_weight=None, num_nodes=None, add_self_loops=True) -> GCNNorm:
    """PyG 2.5.1's ``gcn_norm`` [ext] for a Tensor ``edge_index`` (flow source
    -> target) as a record of per-node arrays instead of a rewritten edge
    list: with ``add_self_loops`` every self-loop edge is dropped and every
    node gets one loop (weight 1, or the weight of its existing self-loop
    edge -- the last in edge order when it has several, where PyG is
    unspecified); ``deg`` = the weights into each node, ``dinv = deg^-1/2``
    (0 where ``deg == 0``).  An edge's coefficient is ``dinv[s] * w * dinv[t]``.
    One launch (``ngnn_gcn_norm``), cached on the block: every layer of a
    forward and the backward share it.  ``edge_weight``: fp32 ``[E]`` on the
    block's device, no gradient.  ``num_nodes`` is needed with a raw
    ``edge_index``."""
    from .block import get_block
    if isinstance(block_or_edge_index, Block):
        block = block_or_edge_index
    else:
        if num_nodes is None:
            raise ValueError("gcn_norm: pass num_nodes with a raw edge_index")
        block = get_block(block_or_edge_index, int(num_nodes))
    return _gcn_record(block, edge_weight, bool(add_self_loops), True)


def _wagg(z, ldz, F, csr, w, norm: GCNNorm, bias, n_rows, out):
    # algorithmic bytes: E (4F + 8 [+4 weighted]) + N (8F + 12)  
    nbytes = csr.nnz * (4 * F + 8 + (4 if w is not None else 0)) + n_rows * (8 * F + 12)
    with _timing.span("gcn_wagg", nbytes):
        rc = _lib.load().ngnn_gcn_wagg(
            _lib.ptr(z), ldz, F, _lib.ptr(csr.rowptr), _lib.ptr(csr.col), _lib.ptr(w),
            _lib.ptr(norm.dinv), _lib.ptr(norm.loop_w), _lib.ptr(bias), n_rows, _lib.ptr(out),
            out.stride(0) if out.size(0) > 1 else max(F, 1), _lib.stream_handle(z.device))
    _lib.check(rc, "ngnn_gcn_wagg")
    return out


def wagg_fwd(z: torch.Tensor, block: Block, norm: GCNNorm, bias=None, out=None) -> torch.Tensor:
    """``ngnn_gcn_wagg`` over the target-grouped CSR, no autograd."""
    zs, ldz = rows_ld(z)
    N, F = block.n_dst, zs.size(1)
    if out is None:
        out = torch.empty(N, F, dtype=torch.float32, device=zs.device)
    return _wagg(zs, ldz, F, block.csr, norm.w, norm, bias, N, out)


def wagg_bwd(g: torch.Tensor, block: Block, norm: GCNNorm) -> torch.Tensor:
    """The input gradient of ``wagg_fwd``: the same entry on the
    source-grouped CSR (an edge's coefficient is symmetric in its ends)."""
    gs, ldg = rows_ld(g)
    N, F = block.n_src, gs.size(1)
    out = torch.empty(N, F, dtype=torch.float32, device=gs.device)
    return _wagg(gs, ldg, F, block.transposed(), norm.w_t(), norm, None, N, out)


class _GCNPropagate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z, block: Block, norm: GCNNorm, bias):
        ctx.block, ctx.norm = block, norm
        return wagg_fwd(z, block, norm, bias)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        dz = wagg_bwd(g, ctx.block, ctx.norm) if ctx.needs_input_grad[0] else None
        db = g.sum(0) if ctx.needs_input_grad[3] else None
        return dz, None, None, db


def gcn_propagate(z: torch.Tensor, block: Block, norm: GCNNorm, bias=None) -> torch.Tensor:
    """``out_i = bias + sum over edges e into i of dinv[s_e] w_e dinv[i]
    z[s_e]`` (+ the node's loop term when ``norm`` replaced the self-loops):
    PyG's ``GCNConv.propagate`` on ``gcn_norm``'s output, without the ``[E,
    F]`` message tensor.  fp32, GPU only; ``z`` passes through its leading
    dimension.  The forward and the gradient with respect to ``z`` (the same
    kernel on ``block.transposed()``) sum in a fixed order: bitwise
    reproducible.  The bias gradient is torch's column sum ``g.sum(0)``, not
    one of this library's fixed-order sums (``GCNConv`` does not take it from
    here: its ``db`` comes from ``ngnn_sage_wgrad``)."""
    z = _check_features(z, "z")
    if z.size(0) != block.n_src:
        raise ValueError(f"z has {z.size(0)} rows but the block has {block.n_src} nodes")
    if norm.block is not block:
        raise ValueError("gcn_propagate: norm was computed for another block")
    if bias is not None and (not bias.is_cuda or bias.dtype != torch.float32 or bias.numel() != z.size(1)):
        raise TypeError("gcn_propagate: bias must be a float32 CUDA tensor with one value per column")
    return _GCNPropagate.apply(z, block, norm, bias)


def sample_seed_rows(graph, fanout: int, batch_size: int, seed0: int, seed_stride: int, r0: int,
                     n_rows: int, seeds=None):
    """The hop-0 draws of loader positions ``r0 .. r0 + n_rows - 1`` of a pass
    with ``batch_size`` seeds per batch, without building a block
    (``ngnn_infer_draw``): position ``p`` is seed ``i = p % batch_size`` of
    batch ``b = p // batch_size``, whose block seed is ``seed0 + b *
    seed_stride`` (``NeighborLoader.batch_seed``); its node is ``seeds[p]``
    (``p`` itself without ``seeds``).  Returns the target-grouped CSR
    ``(rowptr int32[n_rows + 1], col int32[nnz])`` of GLOBAL neighbour ids in
    draw order -- bitwise the in-edges the loader's block gives that seed row.
    ``r0`` must be a multiple of ``batch_size``.  One host read (nnz)."""
    from .infer import seed_rows
    rowptr, col = seed_rows(graph, int(fanout), int(batch_size), seed0, seed_stride, int(r0), int(n_rows), seeds)
    return rowptr, col[:int(rowptr[-1])]


# ---- SAGEPL's per-node input noise (ngnn_node_noise_fwd / _bwd) ----

def node_noise_bad_ids(device=None, reset: bool = False) -> int:
    """How many rows ``add_node_noise``'s forward met on ``device`` with an id
    outside the table (those rows pass ``x`` through and train nothing).
    Debugging only: reading the device counter synchronises."""
    return read_counter("bad-id", device, "add_node_noise", reset)


class _AddNodeNoise(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, noise, n_id, rate: float, sign: bool):
        (xs, ldx), (tab, ldt) = rows_ld(x), rows_ld(noise)
        n_rows, F = xs.shape
        out = torch.empty(n_rows, F, dtype=xs.dtype, device=xs.device)
        flags = _lib.NOISE_SIGN if sign else 0
        bad = device_counter("bad-id", xs.device, "add_node_noise")
        # algorithmic bytes: x rows + table rows + out rows (+ the ids)
        nbytes = 3 * n_rows * F * 4 + (0 if n_id is None else n_rows * 8)
        with _timing.span("node_noise_fwd", nbytes):
            rc = _lib.load().ngnn_node_noise_fwd(
                _lib.ptr(xs), ldx, _lib.ptr(tab), ldt, tab.size(0), _lib.ptr(n_id), n_rows, F,
                rate, flags, _lib.ptr(out), F, _lib.ptr(bad), _lib.stream_handle(xs.device))
        _lib.check(rc, "ngnn_node_noise_fwd")
        ctx.rate, ctx.flags, ctx.ld = rate, flags, (ldx, ldt)
        ctx.save_for_backward(xs if sign else None, tab, n_id)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        xs, tab, n_id = ctx.saved_tensors
        dx = g if ctx.needs_input_grad[0] else None  # d out / d x = 1: the same tensor, no copy
        if not ctx.needs_input_grad[1]:
            return dx, None, None, None, None
        gs, ldg = rows_ld(g)
        n_rows, F = gs.shape
        n_nodes = tab.size(0)
        # no id list: row i is table row i -- stored, nothing to zero or to add up
        scatter = n_id is not None and not torch.are_deterministic_algorithms_enabled()
        if scatter:
            dst = dnoise = torch.zeros(n_nodes, F, dtype=gs.dtype, device=gs.device)
        else:
            dst = torch.empty(n_rows, F, dtype=gs.dtype, device=gs.device)
        # algorithmic bytes: grad rows + table rows read, one row of adds / stores each
        nbytes = 3 * n_rows * F * 4 + (0 if n_id is None else n_rows * 8)
        with _timing.span("node_noise_bwd", nbytes):
            rc = _lib.load().ngnn_node_noise_bwd(
                _lib.ptr(gs), ldg, _lib.ptr(xs), ctx.ld[0] if xs is not None else F, _lib.ptr(tab),
                ctx.ld[1], n_nodes, _lib.ptr(n_id), int(scatter), n_rows, F, ctx.rate, ctx.flags,
                _lib.ptr(dst), F, None, _lib.stream_handle(gs.device))
        _lib.check(rc, "ngnn_node_noise_bwd")
        if n_id is None:
            dnoise = dst
        elif not scatter:
            # deterministic: the per-row gradients summed by torch's deterministic
            # index_add_ (an id outside the table stored a zero row: any row takes it)
            dnoise = torch.zeros(n_nodes, F, dtype=gs.dtype, device=gs.device)
            dnoise.index_add_(0, n_id.clamp(0, max(n_nodes - 1, 0)), dst)
        return dx, dnoise, None, None, None


def add_node_noise(x: torch.Tensor, noise: torch.Tensor, n_id: torch.Tensor | None = None,
                   rate: float = 0.1, sign: bool = False) -> torch.Tensor:
    """``x + [sign(x) *] F.normalize(noise[n_id]) * rate`` as a new tensor --
    the reference's ``SAGEPL.adding_noise`` (sagePL.py:41-49: ``x.clone()``,
    the table gather, the row normalisation, the scale and the add) in one
    launch; ``n_id=None`` takes the table's rows in order (``x`` must then
    have one row per table row; the reference's branch there sets ``sign``).

    Backward: ``dx`` is the incoming gradient itself; ``dnoise`` is dense
    ``[nbr_nodes, F]`` (the reference's optimizer sees a dense gradient: Adam
    moves every row's moments) -- a zero fill and one launch of float atomics,
    duplicates accumulating as ``index_add_``.  Under
    ``torch.use_deterministic_algorithms(True)`` the kernel stores one
    gradient row per input row and torch's deterministic ``index_add_`` sums
    them.  fp32, GPU only; an id outside the table passes its row of ``x``
    through, trains nothing and is counted (``node_noise_bad_ids``)."""
    for name, t in (("x", x), ("noise", noise)):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise ValueError(f"add_node_noise: {name} must be a CUDA tensor (no CPU fallback)")
        if t.dtype != torch.float32:
            raise ValueError(f"add_node_noise: {name} must be float32, got {t.dtype}")
        if t.dim() != 2:
            raise ValueError(f"add_node_noise: {name} must be 2-D, got shape {tuple(t.shape)}")
    if x.device != noise.device:
        raise ValueError(f"add_node_noise: x on {x.device}, noise on {noise.device}")
    if x.size(1) != noise.size(1):
        raise ValueError(f"add_node_noise: x is {x.size(1)} wide, the table {noise.size(1)}")
    if n_id is None:
        if x.size(0) != noise.size(0):
            raise ValueError(f"add_node_noise: without n_id, x needs the table's {noise.size(0)} rows, "
                             f"got {x.size(0)}")
    else:
        if not isinstance(n_id, torch.Tensor) or not n_id.is_cuda or n_id.dtype != torch.int64 \
                or n_id.dim() != 1 or n_id.numel() != x.size(0) or n_id.device != x.device:
            raise ValueError("add_node_noise: n_id must be an int64 CUDA tensor with one id per row of x")
        n_id = n_id.contiguous()
    return _AddNodeNoise.apply(x, noise, n_id, float(rate), bool(sign))


# ---- similarity top-k edge rewiring (ngnn_topk_rewire) ----

def rewire_bad_endpoints(device=None, reset: bool = False) -> int:
    """How many edges ``topk_rewire`` met on ``device`` with an endpoint
    outside ``[0, N)`` (they are ignored).  Debugging only: reading the device
    counter synchronises."""
    return read_counter("bad-endpoint", device, "topk_rewire", reset)


def topk_rewire(h: torch.Tensor, edge_index: torch.Tensor, device=None, k_percent: float = 0.1,
                directed: bool = False, *, return_selections: bool = False):
    """The reference's ``topk_rewire(h, edge_index, device, k_percent,
    directed=False)`` (``src/utils/augmentation.py:36-86``) -> ``(pos_edge,
    neg_edge)``, contiguous int64 ``[2, M]`` on ``h``'s device, sorted by (row,
    column) without duplicates as ``torch.nonzero`` lists them -- with no
    ``N x N`` tensor anywhere: the cosine similarities are computed tile by
    tile on the matrix cores and selected as they come (``ngnn_topk_rewire``).

    With ``k2 = 2 * int(N * k_percent)``: the ``k2`` least similar entries by
    the reference's key leave the positive graph and the ``k2`` most similar
    non-edges join it; the ``k2`` most similar edges leave the negative graph
    and the ``k2`` least similar entries join it (the keys, quirks included:
    include/ngnn.h).  Equal keys are taken in ascending flat index ``i * N +
    j``; the result is bitwise reproducible.  ``h`` is detached (the
    reference's result carries no gradient); ``device`` is accepted for the
    reference's signature and ignored.  One host read (the two output
    lengths), where ``torch.nonzero`` synchronises in the reference.

    ``return_selections=True`` also returns the four selections' flat indices
    (int64 ``[4, k2]``, best key first).  ``directed=True`` is refused (the
    reference's branch raises ``UnboundLocalError``).  fp32, GPU only,
    ``N <= 65535``; an edge with an endpoint outside ``[0, N)`` is ignored and
    counted (``rewire_bad_endpoints``)."""
    if directed:
        raise NotImplementedError("topk_rewire: directed=True returns nothing in the reference "
                                  "(UnboundLocalError); only directed=False is implemented")
    if not isinstance(h, torch.Tensor) or not h.is_cuda:
        raise RuntimeError("ngnn runs on the GPU only: topk_rewire's h is on the CPU")
    if h.dim() != 2:
        raise ValueError(f"topk_rewire: h must be 2-D [N, F], got shape {tuple(h.shape)}")
    if h.dtype != torch.float32:
        raise TypeError(f"topk_rewire: only float32 h is supported, got {h.dtype}")
    if not isinstance(edge_index, torch.Tensor) or edge_index.dim() != 2 or edge_index.size(0) != 2 \
            or edge_index.dtype != torch.int64:
        raise ValueError("topk_rewire: edge_index must be an int64 tensor of shape [2, E]")
    dev = h.device
    hs, ldh = rows_ld(h.detach())
    ei = edge_index.to(dev).contiguous()
    N, F = hs.shape
    E = ei.size(1)
    k2 = 2 * int(N * k_percent)
    if k2 < 0:
        raise ValueError(f"topk_rewire: k_percent must not be negative, got {k_percent}")
    lib = _lib.load()
    cap = E + k2
    if N == 0:
        empty = torch.empty(2, 0, dtype=torch.int64, device=dev)
        sel = torch.empty(4, 0, dtype=torch.int64, device=dev)
        return (empty, empty.clone(), sel) if return_selections else (empty, empty.clone())
    ws_bytes = lib.ngnn_topk_rewire_workspace_bytes(N, F, E, k2)
    ws = pos = neg = counts = sel = None
    if ws_bytes:  # (0: sizes the entry refuses -- it reports which, before anything is read)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        pos = torch.empty(2, cap, dtype=torch.int64, device=dev)
        neg = torch.empty(2, cap, dtype=torch.int64, device=dev)
        counts = torch.zeros(3, dtype=torch.int32, device=dev)
        if return_selections:
            sel = torch.empty(4, k2, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        bad = device_counter("bad-endpoint", dev, "topk_rewire") if ws_bytes else None
        # algorithmic bytes: h once, the edges, the outputs (the similarity tiles stay on chip)
        with _timing.span("topk_rewire", N * F * 4 + E * 16 + 2 * cap * 16):
            rc = lib.ngnn_topk_rewire(
                _lib.ptr(hs), ldh, N, F, _lib.ptr(ei[0]) if E else None, _lib.ptr(ei[1]) if E else None,
                E, k2, _lib.ptr(pos), cap, _lib.ptr(neg), cap, _lib.ptr(counts), _lib.ptr(bad),
                _lib.ptr(sel), _lib.ptr(ws), ws_bytes, _lib.stream_handle(dev))
    _lib.check(rc, "ngnn_topk_rewire")
    n_pos, n_neg, overflow = counts.tolist()
    if overflow:
        raise _lib.NGNNError("topk_rewire: a candidate list filled up -- more than 2^20 entries tie at the "
                             "similarity of a selection's threshold (include/ngnn.h)")
    out = (pos[:, :n_pos].contiguous(), neg[:, :n_neg].contiguous())
    return out + (sel,) if return_selections else out


# ---- per-row partial feature shuffle (ngnn_shuffle_rows) ----

def shuffle_pos(features: torch.Tensor, device=None, prob: float = 0.1, seed: int | None = None) -> torch.Tensor:
    """The reference's ``shuffle_pos(features, device, prob)``
    (``src/utils/augmentation.py:88-102``): in every row, ``m = int(F * prob)``
    columns drawn uniformly at random trade their values by a uniform random
    permutation; the other columns are copied.  One launch
    (``ngnn_shuffle_rows``) instead of a Python loop of two ``torch.randperm``
    and an indexed write per row.  Returns a new detached tensor, as the
    reference's ``clone().detach()``; row-strided views are read in place.

    The draw is this library's own (include/ngnn.h), a pure function of
    ``(seed, row, F, m)`` -- the reference's depends on torch's global CPU
    generator and cannot be reproduced.  ``seed=None`` draws a 62-bit seed
    from torch's default CPU generator (a host-only call, no device sync), so
    ``torch.manual_seed`` makes a run repeatable.  A captured graph bakes in
    the seed it was captured with: every replay shuffles the same way.
    ``device`` is accepted for the reference's signature and ignored (the
    result stays on ``features``' device).  fp32, GPU only."""
    if not isinstance(features, torch.Tensor) or not features.is_cuda:
        raise RuntimeError("ngnn runs on the GPU only: shuffle_pos's features are on the CPU")
    if features.dim() != 2:
        raise ValueError(f"shuffle_pos: features must be 2-D [N, F], got shape {tuple(features.shape)}")
    if features.dtype != torch.float32:
        raise TypeError(f"shuffle_pos: only float32 features are supported, got {features.dtype}")
    x, ldx = rows_ld(features.detach())
    N, F = x.shape
    m = int(F * prob)  # augmentation.py:94, same float arithmetic
    if not 0 <= m <= F:
        raise ValueError(f"shuffle_pos: prob {prob} moves {m} of {F} columns")
    if seed is None:
        seed = int(torch.randint(0, 1 << 62, (1,)).item())
    out = torch.empty(N, F, dtype=torch.float32, device=x.device)
    with _timing.span("shuffle_pos", 2 * N * F * 4):
        rc = _lib.load().ngnn_shuffle_rows(_lib.ptr(x), ldx, N, F, m, int(seed) & 0xFFFFFFFFFFFFFFFF,
                                           _lib.ptr(out), F, _lib.stream_handle(x.device))
    _lib.check(rc, "ngnn_shuffle_rows")
    return out


# ---- fused ReLU - BatchNorm1d - dropout (ngnn_bn_fwd_train / _fwd_eval / _bwd) ----

class _BatchNormAct(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, bn, relu: bool, p: float, training: bool, seed: int, seed_dev):
        xs, ldx = rows_ld(x)
        n_rows, F = xs.shape
        out = torch.empty(n_rows, F, dtype=xs.dtype, device=xs.device)
        lib, st = _lib.load(), _lib.stream_handle(xs.device)
        if not training:
            with _timing.span("bn_fwd_eval", 2 * n_rows * F * 4):
                rc = lib.ngnn_bn_fwd_eval(_lib.ptr(xs), ldx, n_rows, F, int(relu), _lib.ptr(weight), _lib.ptr(bias),
                                          bn.eps, _lib.ptr(bn.running_mean), _lib.ptr(bn.running_var),
                                          _lib.ptr(out), F, st)
            _lib.check(rc, "ngnn_bn_fwd_eval")
            return out
        # rows: the batch mean, its fp32 rounding residual, invstd
        stats = torch.empty(3, F, dtype=torch.float32, device=xs.device)
        ws_bytes = lib.ngnn_bn_workspace_bytes(n_rows, F)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=xs.device)
        momentum = -1.0 if bn.momentum is None else float(bn.momentum)
        # algorithmic bytes: x twice (statistics, apply) + out
        with _timing.span("bn_fwd_train", 3 * n_rows * F * 4):
            rc = lib.ngnn_bn_fwd_train(_lib.ptr(xs), ldx, n_rows, F, int(relu), _lib.ptr(weight), _lib.ptr(bias),
                                       bn.eps, momentum, _lib.ptr(bn.running_mean), _lib.ptr(bn.running_var),
                                       _lib.ptr(bn.num_batches_tracked), p, seed, _lib.ptr(seed_dev),
                                       _lib.ptr(out), F, _lib.ptr(stats[0]), _lib.ptr(stats[1]), _lib.ptr(stats[2]),
                                       _lib.ptr(ws), ws_bytes, st)
        _lib.check(rc, "ngnn_bn_fwd_train")
        ctx.relu, ctx.p, ctx.seed, ctx.ldx = relu, p, seed, ldx
        ctx.save_for_backward(xs, weight, stats, seed_dev)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        xs, weight, stats, seed_dev = ctx.saved_tensors
        gs, ldg = rows_ld(g)
        n_rows, F = xs.shape
        dgamma, dbeta = torch.empty_like(stats[0]), torch.empty_like(stats[0])
        # the input that needs no gradient (bn1 on batch.x): no dx pass at all
        dx = torch.empty(n_rows, F, dtype=xs.dtype, device=xs.device) if ctx.needs_input_grad[0] else None
        lib = _lib.load()
        ws_bytes = lib.ngnn_bn_workspace_bytes(n_rows, F)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=xs.device)
        # algorithmic bytes: dout and x for the sums, again (+ dx) for the dx pass
        with _timing.span("bn_bwd", (2 if dx is None else 5) * n_rows * F * 4):
            rc = lib.ngnn_bn_bwd(_lib.ptr(gs), ldg, _lib.ptr(xs), ctx.ldx, n_rows, F, int(ctx.relu),
                                 _lib.ptr(weight), _lib.ptr(stats[0]), _lib.ptr(stats[1]), _lib.ptr(stats[2]),
                                 ctx.p, ctx.seed,
                                 _lib.ptr(seed_dev), _lib.ptr(dgamma), _lib.ptr(dbeta), _lib.ptr(dx), F,
                                 _lib.ptr(ws), ws_bytes, _lib.stream_handle(xs.device))
        _lib.check(rc, "ngnn_bn_bwd")
        return dx, dgamma, dbeta, None, None, None, None, None, None


def batch_norm_act_supported(x: torch.Tensor, bn: torch.nn.BatchNorm1d, training: bool) -> bool:
    """Whether ``batch_norm_act`` runs on the HIP kernels: a 2-D fp32 CUDA
    ``x``, an affine ``bn`` with fp32 parameters that tracks its running
    statistics, no stream capture in progress (a graph slot's padded rows
    would enter the statistics), and, in eval mode, nothing to differentiate
    (the kernels have no eval-mode backward)."""
    if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 2):
        return False
    if bn.weight is None or bn.bias is None or bn.running_mean is None or bn.running_var is None \
            or bn.num_batches_tracked is None:
        return False
    if any(t.dtype != torch.float32 or t.device != x.device
           for t in (bn.weight, bn.bias, bn.running_mean, bn.running_var)):
        return False
    if x.size(1) != bn.num_features or torch.cuda.is_current_stream_capturing():
        return False
    if not training and torch.is_grad_enabled() and (x.requires_grad or bn.weight.requires_grad
                                                     or bn.bias.requires_grad):
        return False
    return True


def batch_norm_act(x: torch.Tensor, bn: torch.nn.BatchNorm1d, relu: bool = False, p: float = 0.0,
                   training: bool | None = None, seed: int | None = None, seed_dev=None) -> torch.Tensor:
    """``dropout(bn(relu(x)))`` -- the chain the reference runs per hidden
    layer with ``use_bn`` (``sage.py:31-38``) -- on three launches forward and
    three backward (``ngnn_bn_fwd_train`` / ``ngnn_bn_bwd``; one launch in eval
    mode) instead of a torch launch per op and pass.  ``relu=False, p=0`` is
    the plain ``bn(x)`` of the input features; an ``x`` that needs no gradient
    skips the backward's dx pass.

    ``bn`` holds the parameters and the buffers (state-dict keys unchanged);
    its running statistics and ``num_batches_tracked`` move on the device as
    ``nn.BatchNorm1d``'s.  ``training=None`` follows ``bn.training``.  The
    dropout is the library's hash dropout keyed by ``(seed ^ *seed_dev, row,
    column)`` (``seed=None``: drawn from torch's CPU generator), applied in
    training only, like ``F.dropout(training=...)``.

    Runs on the kernels when ``batch_norm_act_supported``; anything else
    (bf16, a captured step, a ``bn`` without affine parameters or running
    statistics, eval mode under autograd) is torch's ``relu`` /
    ``nn.BatchNorm1d`` / ``F.dropout``, as before this op existed."""
    training = bn.training if training is None else bool(training)
    p = float(p)
    if not batch_norm_act_supported(x, bn, training):
        if training != bn.training:
            raise ValueError("batch_norm_act: a training flag other than bn.training needs the HIP path")
        y = bn(x.relu() if relu else x)
        return torch.nn.functional.dropout(y, p=p, training=training)
    if not 0.0 <= p <= 1.0:
        raise ValueError(f"batch_norm_act: dropout probability has to be between 0 and 1, got {p}")
    if training and x.size(0) < 2:  # nn.BatchNorm1d's own refusal
        raise ValueError(f"Expected more than 1 value per channel when training, got input size {tuple(x.shape)}")
    if not training or p == 0.0:
        p, seed, seed_dev = 0.0, 0, None
    elif seed is None:
        seed = int(torch.randint(0, 1 << 62, (1,)).item())  # torch's (CPU) RNG stream
    return _BatchNormAct.apply(x, bn.weight, bn.bias, bn, bool(relu), p, training,
                               int(seed) & 0xFFFFFFFFFFFFFFFF, seed_dev)
