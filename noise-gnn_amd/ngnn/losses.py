"""Seed-row cross entropy on the device (ngnn_seed_xent_*).

``seed_cross_entropy(out, y, batch_size)`` == ``F.cross_entropy(out[:batch_size],
y[:batch_size])`` -- the loss of the reference's training loop
(pipeline.py:158) -- instead of the softmax / nll / slice-backward / fill
chain.  When the logits need a gradient, ONE launch
(``ngnn_seed_xent_fwd_grad``) writes the loss and the unit-scale gradient;
the backward then costs nothing when its incoming gradient is the training
step's persistent unit tensor (``unit_grad``, marked ``_ngnn_unit``) and one
launch otherwise.  The input gradient is a view of a zero-initialised
buffer whose rows >= batch_size stay zero (only rows < batch_size are ever
written), held by its node from the forward on (``_GradHold``: one pool of
such buffers for every loss here, and the rule that keeps two nodes of one
backward pass off the same storage), and it tells the SAGE stack's backward
how many leading rows can be nonzero (``_ngnn_nonzero_rows``), so that
backward skips its row-extent scan.

The reference's other losses follow the same plan: ``CTLoss`` and
``CoDiLoss`` (ngnn_ct_loss_* / ngnn_codi_loss_*: both models' row losses,
the argsorts and the exchange on the device) and ``backward_correction``
(ngnn_bc_loss_*: loss and gradient rows in one launch pair, the inverse of
the correction matrix kept on the device), and so does the contrastive term
of the reference's train_ct step, ``contrastive_loss`` (ngnn_contrast_*:
``Discriminator_innerprod`` + ``BCEExeprtLoss`` on the rows an index tensor
names, one launch pair each way), and the uncertainty-weighted consistency
term of its train_ct step, ``get_uncertainty_batch`` and ``fix_cr``
(ngnn_nbr_uncertainty: one launch on the block's by-source CSR;
ngnn_fix_cr_*: one launch pair each way).
"""
from __future__ import annotations

import weakref

import torch

from . import _lib
from ._common import device_counter, read_counter, rows_ld

_ws: dict = {}


def unit_grad(loss: torch.Tensor) -> torch.Tensor:
    """A ones tensor shaped like `loss` that the loss backward recognises as 1
    (no scale launch): for a training step's loss.backward(unit_grad(loss)),
    kept by the caller and never modified."""
    one = torch.ones_like(loss)
    one._ngnn_unit = True
    return one


# ---------------------------------------------------------------------------
# The zero-row gradient pool.  Every loss here that reads only the B seed rows
# of an [N, C] input returns its gradient as a view of a zero-initialised
# buffer: only rows < B are ever written, so rows >= B are zero without a
# fill.  THE RULE: a buffer returned as a gradient by one node is never handed
# to another node that can run in the same backward pass -- autograd adds the
# gradients that meet at one input, and two views of one storage would add up
# to twice the last one written.  So
#   - a node takes its buffer at FORWARD time (_GradHold), for the inputs that
#     need a gradient: as many pending nodes, as many buffers;
#   - it gives the buffer back at its first backward, or when its graph is
#     dropped unused: steady state is one buffer per key, and stream order
#     protects the rows until that backward pass has consumed them;
#   - nothing is drawn from the free list at backward time: a node that is
#     back-propagated again writes into a zero buffer of its own.
_free_grads: dict = {}  # (device, C, tag, dtype) -> buffers no pending node holds


class _GradHold:
    """One pending node's [>= n, c] zero-row buffer.  `tag` tells the losses
    and their B apart: a buffer shared with a larger B would hold that call's
    stale rows in [B, B_larger)."""

    def __init__(self, dev, n: int, c: int, tag, dtype=torch.float32):
        free = _free_grads.setdefault((dev, c, tag, dtype), [])
        self.buf = None
        while free and self.buf is None:
            buf = free.pop()
            if buf.size(0) >= n:  # (a shorter one is dropped: grown on demand)
                self.buf = buf
        if self.buf is None:
            self.buf = torch.zeros(max(n, 1), c, dtype=dtype, device=dev)
        # (weakref finalizer: also when the autograd graph is dropped unused)
        self._pooled = weakref.finalize(self, free.append, self.buf)
        self._own = None

    def rows(self, n: int):
        """``(buf[:n], first)`` for one backward of the holding node.  first:
        the rows are as the forward left them, and the buffer goes back to
        the pool.  Not first (retain_graph): a zero buffer this node owns."""
        if self._pooled.alive:
            self._pooled()
            return self.buf[:n], True
        if self._own is None:
            self._own = torch.zeros_like(self.buf)
        return self._own[:n], False


def _workspace(dev, B: int) -> torch.Tensor:
    """Per-(device, B) loss workspace; zero-filled once (its ticket resets
    itself), then reused by every call on the stream."""
    key = (dev, B)
    buf = _ws.get(key)
    if buf is None:
        n = _lib.load().ngnn_seed_xent_workspace_bytes(B)
        buf = torch.zeros(n, dtype=torch.uint8, device=dev)
        _ws[key] = buf
    return buf


class _SeedRowLoss(torch.autograd.Function):
    """The skeleton of an fp32 loss over the seed rows ``logits[:B]`` whose
    forward launch also writes the unit-scale gradient rows: the hold, the
    unit-gradient shortcut (no launch in backward) and the recompute for any
    other gradient or a second backward.  A subclass gives ``tag`` and
      _fwd(ctx, x, ld, yy, arg, loss, dx) -> the tensors its _bwd needs saved
                                             (dx None: no gradient wanted)
      _bwd(ctx, x, ld, yy, saved, g, dx)  -> rows < B of dx for the scalar g
    where ``arg`` is the loss's one extra argument."""

    @classmethod
    def forward(cls, ctx, logits, y, batch_size: int, arg):
        ctx.B, ctx.n = int(batch_size), logits.size(0)
        x, ctx.ld = rows_ld(logits)
        yy = y[:ctx.B].contiguous()
        loss = torch.empty((), dtype=torch.float32, device=x.device)
        ctx.hold = None
        if ctx.needs_input_grad[0]:
            ctx.hold = _GradHold(x.device, ctx.n, x.size(1), (cls.tag, ctx.B))
        saved = cls._fwd(ctx, x, ctx.ld, yy, arg, loss, None if ctx.hold is None else ctx.hold.buf)
        ctx.save_for_backward(x, yy, *saved)
        return loss

    @classmethod
    def backward(cls, ctx, g):
        x, yy, *saved = ctx.saved_tensors
        dx, first = ctx.hold.rows(ctx.n)
        if not (first and getattr(g, "_ngnn_unit", False)):
            cls._bwd(ctx, x, ctx.ld, yy, saved, g, dx)
        dx._ngnn_nonzero_rows = ctx.B  # rows >= B are zero: the SAGE backward's row bound
        return dx, None, None, None


def _seed_xent_bwd(x, ld, B, yy, ignore, ws, g, count, dx) -> None:
    g = g.contiguous()
    _lib.check(_lib.load().ngnn_seed_xent_bwd(
        _lib.ptr(x), ld, B, x.size(1), _lib.ptr(yy), ignore, _lib.ptr(ws), _lib.ptr(g), _lib.ptr(count),
        _lib.ptr(dx), dx.stride(0), _lib.stream_handle(x.device)), "ngnn_seed_xent_bwd")


class _SeedXent(_SeedRowLoss):
    tag = "xent"

    @staticmethod
    def _fwd(ctx, x, ld, yy, ignore_index, loss, dx):
        count = torch.empty((), dtype=torch.float32, device=x.device)
        ctx.ws, ctx.ignore = _workspace(x.device, ctx.B), int(ignore_index)
        lib, ws = _lib.load(), ctx.ws
        if dx is not None:  # loss + the unit-scale gradient in one launch
            _lib.check(lib.ngnn_seed_xent_fwd_grad(
                _lib.ptr(x), ld, ctx.B, x.size(1), _lib.ptr(yy), ctx.ignore, _lib.ptr(loss), _lib.ptr(count),
                _lib.ptr(dx), dx.stride(0), _lib.ptr(ws), ws.numel(), _lib.stream_handle(x.device)),
                "ngnn_seed_xent_fwd_grad")
        else:
            _lib.check(lib.ngnn_seed_xent_fwd(
                _lib.ptr(x), ld, ctx.B, x.size(1), _lib.ptr(yy), ctx.ignore, _lib.ptr(loss), _lib.ptr(count),
                _lib.ptr(ws), ws.numel(), _lib.stream_handle(x.device)), "ngnn_seed_xent_fwd")
        return (count,)

    @staticmethod
    def _bwd(ctx, x, ld, yy, saved, g, dx):
        _seed_xent_bwd(x, ld, ctx.B, yy, ctx.ignore, ctx.ws, g, saved[0], dx)


class _BF16SeedRows(torch.autograd.Function):
    """A seed-row loss (``node``: _SeedXent or _BCLoss) of bf16 logits: only
    rows < B are widened (B x C, not the N x C logits), the fp32 node runs on
    them, and the gradient comes back as bf16 [N, C] with rows >= B zero (a
    pooled buffer of its own, like the fp32 node's) carrying the row hint."""

    @staticmethod
    def forward(ctx, logits, y, batch_size: int, arg, node):
        B = int(batch_size)
        ctx.node, ctx.n_full = node, logits.size(0)
        ctx.out_hold = None
        if ctx.needs_input_grad[0]:
            ctx.out_hold = _GradHold(logits.device, ctx.n_full, logits.size(1), (node.tag, B), torch.bfloat16)
        # the seed rows widened by the library (exact; an ATen copy kernel
        # otherwise), then the fp32 node's forward on them (it fills ctx for
        # its backward: saved rows, B, n = B)
        lw, ld = rows_ld(logits)
        wide = torch.empty(B, lw.size(1), dtype=torch.float32, device=lw.device)
        _lib.check(_lib.load().ngnn_widen_bf16_rows(_lib.ptr(lw), ld, lw.size(1), B, None, _lib.ptr(wide),
                                                    wide.stride(0), _lib.stream_handle(lw.device)),
                   "ngnn_widen_bf16_rows")
        return node.forward(ctx, wide, y, B, arg)

    @staticmethod
    def backward(ctx, g):
        dx = ctx.node.backward(ctx, g)[0]  # fp32 [B, C], contiguous (ctx.n == B there)
        out, _ = ctx.out_hold.rows(ctx.n_full)
        _lib.check(_lib.load().ngnn_cast_f32_bf16(_lib.ptr(dx), _lib.ptr(out), dx.numel(),
                                                  _lib.stream_handle(dx.device)), "ngnn_cast_f32_bf16")
        out._ngnn_nonzero_rows = ctx.B
        return out, None, None, None, None


class _CastKeepRows(torch.autograd.Function):
    """x.to(dtype) whose backward keeps the nonzero-row hint on the gradient
    (a plain cast's backward returns a fresh tensor without it, and the SAGE
    stack's backward would then bound nothing: every row)."""

    @staticmethod
    def forward(ctx, x, dtype):
        ctx.src = x.dtype
        return x.to(dtype)

    @staticmethod
    def backward(ctx, g):
        gi = g.to(ctx.src)
        rows = getattr(g, "_ngnn_nonzero_rows", None)
        if rows is not None:
            gi._ngnn_nonzero_rows = rows
        return gi, None


def cast_keep_rows(x: torch.Tensor, dtype) -> torch.Tensor:
    return x if x.dtype == dtype else _CastKeepRows.apply(x, dtype)


class _HeadXent(torch.autograd.Function):
    """The loss a graph slot's two-layer forward already took (ngnn.fused.
    LossHead, include/ngnn.h ngnn_xent_head): forward hands its loss over;
    backward, for the training step's unit gradient, hands over the gradient
    rows that forward wrote -- marked with their scatter onto the source rows
    (_ngnn_g_pre), which the stack's backward then skips.  Any other incoming
    gradient: the scaled rows recomputed from the logits (ngnn_seed_xent_bwd)."""

    @staticmethod
    def forward(ctx, logits, res):
        ctx.res = res
        ctx.n = logits.size(0)
        ctx.save_for_backward(logits)
        return res.loss

    @staticmethod
    def backward(ctx, g):
        res = ctx.res
        hd = res.head
        if getattr(g, "_ngnn_unit", False):
            dy = hd.dy[:ctx.n]
            dy._ngnn_nonzero_rows = hd.B
            dy._ngnn_g_pre = hd.g
            return dy, None
        (x,) = ctx.saved_tensors
        # a zero-row buffer kept on the head (one pending node per slot), never
        # the pool's: nothing is drawn from the free list at backward time
        if getattr(hd, "dy_scaled", None) is None:
            hd.dy_scaled = torch.zeros_like(hd.dy)
        dx = hd.dy_scaled[:ctx.n]
        _seed_xent_bwd(x, x.stride(0), hd.B, hd.y[:hd.B], hd.ignore, hd.ws, g, res.count, dx)
        dx._ngnn_nonzero_rows = hd.B
        return dx, None


def seed_cross_entropy(logits: torch.Tensor, y: torch.Tensor, batch_size: int,
                       ignore_index: int = -100) -> torch.Tensor:
    """Mean cross entropy of ``logits[:batch_size]`` against ``y[:batch_size]``."""
    if not logits.is_cuda:
        raise RuntimeError("ngnn.losses.seed_cross_entropy: GPU only (no CPU fallback)")
    res = getattr(logits, "_ngnn_head", None)
    if (res is not None and not res.used and logits.dtype == torch.float32 and logits.requires_grad
            and y.data_ptr() == res.head.y.data_ptr() and y.numel() >= batch_size
            and int(batch_size) == res.head.B and int(ignore_index) == res.head.ignore):
        # the slot's forward took this loss already (ngnn.fused.LossHead)
        res.used = True
        return _HeadXent.apply(logits, res)
    if logits.dtype == torch.bfloat16:  # bf16 models: the loss is taken in fp32
        if logits.dim() == 2 and 0 < batch_size <= logits.size(0) and y.numel() >= batch_size:
            return _BF16SeedRows.apply(logits, y, batch_size, ignore_index, _SeedXent)
        logits = cast_keep_rows(logits, torch.float32)
    if logits.dim() != 2 or logits.dtype != torch.float32:
        raise ValueError("logits must be a 2-D float32 (or bf16) tensor")
    if batch_size <= 0 or batch_size > logits.size(0) or y.numel() < batch_size:
        raise ValueError("batch_size out of range")
    return _SeedXent.apply(logits, y, batch_size, ignore_index)


# ---------------------------------------------------------------------------
# Co-teaching loss (CTLoss, src/utils/losses.py:10-49) on the device

class _CTState:
    """Outputs of one ngnn_ct_loss_fwd launch pair, shared by the two
    per-model autograd nodes (each model's backward reads the rows the other
    model kept from the workspace)."""
    __slots__ = ("ws", "out", "y_noise", "ignore", "B", "C")


class _CTPick(torch.autograd.Function):
    """loss_m (already computed by the shared forward) as a differentiable
    function of y_m alone, so that loss_1.backward() and loss_2.backward()
    each run only their own model's graph, as in pipeline.py:125-131.
    y_m may hold more rows than the loss reads (the whole block's logits,
    CTLoss(..., batch_size=B)): its gradient is then a pooled zero-row buffer,
    taken here at forward time, whose rows < B the backward launch writes (no
    slice backward), marked for the SAGE stack's bounded backward."""

    @staticmethod
    def forward(ctx, y, state: _CTState, m: int):
        ctx.state, ctx.m, ctx.n = state, m, y.size(0)
        ctx.hold = None
        if ctx.n > state.B and ctx.needs_input_grad[0]:  # rows >= B never written: zero
            ctx.hold = _GradHold(y.device, ctx.n, state.C, ("ct", state.B))
        ctx.save_for_backward(y)
        return state.out[m].clone()

    @staticmethod
    def backward(ctx, g):
        (y,) = ctx.saved_tensors
        st = ctx.state
        if ctx.hold is not None:
            dy, _ = ctx.hold.rows(ctx.n)
        else:
            dy = torch.empty(st.B, st.C, dtype=torch.float32, device=y.device)
        g = g.reshape(1).to(torch.float32).contiguous()
        _lib.check(_lib.load().ngnn_ct_loss_bwd(
            ctx.m, _lib.ptr(y), rows_ld(y)[1], st.B, st.C, _lib.ptr(st.y_noise), st.ignore,
            _lib.ptr(st.ws), _lib.ptr(g), _lib.ptr(dy), dy.stride(0),
            _lib.stream_handle(y.device)), "ngnn_ct_loss_bwd")
        dy._ngnn_nonzero_rows = st.B
        return dy, None, None


class CTLoss(torch.nn.Module):
    """Drop-in for the reference's ``CTLoss(device)`` (losses.py:10-49).

    ``forward(y_1, y_2, y_noise, forget_rate, ind, noise_or_not)`` returns the
    same 8-tuple ``(loss_1_update, loss_2_update, pure_ratio_1, pure_ratio_2,
    ind_1_update, ind_2_update, ind_noisy_1, ind_noisy_2)`` with no host
    round trip: the per-row cross entropies, both argsorts, the exchange
    selection and the pure ratios are two device launches
    (``ngnn_ct_loss_fwd``), each loss's backward one launch.

    Differences from the reference, all documented in DESIGN.md: the index
    outputs are device int64 tensors instead of numpy arrays (the pipelines
    discard them, pipeline.py:116); tied losses are ordered by row index
    (np.argsort's quicksort leaves ties unspecified); ``noise_or_not`` is
    best passed as a device bool tensor (a CPU one is copied per call);
    batches of at most 8192 rows.
    """

    def __init__(self, device=None, ignore_index: int = -100):
        super().__init__()
        self.device = device
        self.ignore_index = ignore_index
        # device int32: nonzero once an `ind` entry fell outside noise_or_not
        # (the reference raises IndexError there; checking it needs a sync)
        self.index_error = None

    def forward(self, y_1, y_2, y_noise, forget_rate, ind, noise_or_not, batch_size: int | None = None):
        """batch_size (extension): y_1 / y_2 are a block's whole logits [N, C]
        and the loss reads rows < batch_size -- the reference's
        ``model(x, ei)[:batch_size]`` without the slice (pipeline.py:113-114);
        each model's gradient then comes back [N, C], zero past the seeds."""
        loss_1, loss_2, out, i1, i2, num_remember, err = _exchange_forward(
            "CTLoss", self.ignore_index, None, y_1, y_2, y_noise, forget_rate, ind, noise_or_not, batch_size)
        self.index_error = err
        return (loss_1, loss_2, out[2], out[3], i1[:num_remember], i2[:num_remember],
                i1[num_remember:], i2[num_remember:])


def _exchange_forward(name, ignore_index, co_lambda, y_1, y_2, y_noise, forget_rate, ind, noise_or_not,
                      batch_size):
    """The shared forward of CTLoss (co_lambda None: ngnn_ct_loss_fwd) and
    CoDiLoss (ngnn_codi_loss_fwd): argument checks, one launch pair, the two
    per-model autograd nodes.  Returns (loss_1, loss_2, out[4], ind_1_sorted,
    ind_2_sorted, rows kept, index_error)."""
    if not (y_1.is_cuda and y_2.is_cuda):
        raise RuntimeError(f"ngnn.losses.{name}: GPU only (no CPU fallback)")
    if y_1.dim() != 2 or y_1.shape != y_2.shape or y_1.dtype != torch.float32 \
            or y_2.dtype != torch.float32:
        raise ValueError("y_1, y_2 must be float32 [B, C] tensors of the same shape")
    B, C = y_1.shape
    if batch_size is not None:
        if not 0 < int(batch_size) <= B:
            raise ValueError(f"batch_size {batch_size} outside (0, {B}]")
        B = int(batch_size)
    dev = y_1.device
    remember_rate = 1 - forget_rate
    num_remember = int(remember_rate * B)  # losses.py:29-30, same float arithmetic
    if not 0 <= num_remember <= B:
        raise ValueError(f"forget_rate {forget_rate} gives num_remember {num_remember}")
    (a, lda), (b, ldb) = rows_ld(y_1), rows_ld(y_2)
    yn = y_noise.to(device=dev, dtype=torch.int64).reshape(-1)
    if batch_size is not None:  # (a block's labels / ids: the seed rows')
        yn = yn[:B]
        ind = None if ind is None else ind.reshape(-1)[:B]
    yn = yn.contiguous()
    if yn.numel() != B:
        raise ValueError("y_noise must hold one label per row")
    idx = None if ind is None else ind.to(device=dev, dtype=torch.int64).contiguous()
    clean = None
    if noise_or_not is not None:
        clean = noise_or_not.to(device=dev, dtype=torch.bool).contiguous()
    lib = _lib.load()
    out = torch.empty(4, dtype=torch.float32, device=dev)
    i1 = torch.empty(B, dtype=torch.int64, device=dev)
    i2 = torch.empty(B, dtype=torch.int64, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    # workspace per call (caching allocator, no sync): both backwards read it later
    if co_lambda is None:
        ws = torch.empty(lib.ngnn_ct_loss_workspace_bytes(B), dtype=torch.uint8, device=dev)
        _lib.check(lib.ngnn_ct_loss_fwd(
            _lib.ptr(a), lda, _lib.ptr(b), ldb, B, C, _lib.ptr(yn),
            int(ignore_index), num_remember, _lib.ptr(idx), _lib.ptr(clean),
            0 if clean is None else clean.numel(), _lib.ptr(out), _lib.ptr(i1), _lib.ptr(i2),
            _lib.ptr(ws), ws.numel(), _lib.ptr(err), _lib.stream_handle(dev)), "ngnn_ct_loss_fwd")
    else:
        ws = torch.empty(lib.ngnn_codi_loss_workspace_bytes(B), dtype=torch.uint8, device=dev)
        _lib.check(lib.ngnn_codi_loss_fwd(
            _lib.ptr(a), lda, _lib.ptr(b), ldb, B, C, _lib.ptr(yn),
            int(ignore_index), num_remember, float(co_lambda), _lib.ptr(idx), _lib.ptr(clean),
            0 if clean is None else clean.numel(), _lib.ptr(out), _lib.ptr(i1), _lib.ptr(i2), None,
            _lib.ptr(ws), ws.numel(), _lib.ptr(err), _lib.stream_handle(dev)), "ngnn_codi_loss_fwd")
        if num_remember == 0:  # an empty selection keeps every row (losses.py:125-128)
            num_remember = B
    st = _CTState()
    st.ws, st.out, st.y_noise, st.ignore, st.B, st.C = ws, out, yn, int(ignore_index), B, C
    loss_1 = _CTPick.apply(a, st, 0)
    loss_2 = _CTPick.apply(b, st, 1)
    return loss_1, loss_2, out, i1, i2, num_remember, err


class CoDiLoss(torch.nn.Module):
    """Drop-in for the reference's ``CoDiLoss(device, co_lambda)`` (losses.py:
    72-137): CTLoss's exchange, each model's rows ranked by ``cross_entropy -
    co_lambda * JS(y_1, y_2)`` (JS detached, ``js_loss_compute``'s form) --
    two device launches (``ngnn_codi_loss_fwd``) instead of the softmax /
    kl_div chain and two ``np.argsort`` host round trips; each loss's backward
    one launch.

    ``forward`` returns the reference's ``(loss_1, loss_2, pure_ratio_1,
    pure_ratio_2, 0, 0, 0, 0)``; with ``return_indices=True`` the last four
    are CTLoss's device index tensors (kept and forgotten rows of each
    model).  A forget rate that remembers no row keeps ALL rows, as the
    reference (losses.py:125-128).  Ties, ``noise_or_not``, ``index_error``,
    ``batch_size`` and the 8192-row limit: as ``CTLoss``."""

    def __init__(self, device=None, co_lambda: float = 0.1, ignore_index: int = -100,
                 return_indices: bool = False):
        super().__init__()
        self.device = device
        self.co_lambda = co_lambda
        self.ignore_index = ignore_index
        self.return_indices = return_indices
        self.index_error = None

    def forward(self, y_1, y_2, y_noise, forget_rate, ind, noise_or_not, batch_size: int | None = None):
        loss_1, loss_2, out, i1, i2, kept, err = _exchange_forward(
            "CoDiLoss", self.ignore_index, self.co_lambda, y_1, y_2, y_noise, forget_rate, ind,
            noise_or_not, batch_size)
        self.index_error = err
        if not self.return_indices:
            return loss_1, loss_2, out[2], out[3], 0, 0, 0, 0
        return loss_1, loss_2, out[2], out[3], i1[:kept], i2[:kept], i1[kept:], i2[kept:]


# ---------------------------------------------------------------------------
# Backward loss correction (backward_correction, src/utils/losses.py:51-70)

_cinv: dict = {}  # (id(C), device) -> (weakref to C, version, host copy or None, Cinv on the device)


def _cinv_drop(key, _ref=None) -> None:
    _cinv.pop(key, None)


def _correction_inverse(C, dev) -> torch.Tensor:
    """``np.linalg.inv(C).astype(np.float32)`` (losses.py:62) on `dev`, taken
    once per matrix: cached by the object and the version of its contents (a
    tensor's ``_version``; a numpy array's values, compared against a kept
    copy -- C x C, cheaper than the inverse), dropped with the object."""
    import numpy as np
    key = (id(C), dev)
    ent = _cinv.get(key)
    is_t = torch.is_tensor(C)
    if ent is not None and ent[0]() is C:
        if is_t:
            if ent[1] == C._version:
                return ent[3]
        elif ent[2].shape == C.shape and ent[2].dtype == C.dtype and np.array_equal(ent[2], C):
            return ent[3]
    host = C.detach().cpu().numpy() if is_t else np.asarray(C)
    inv = torch.from_numpy(np.linalg.inv(host).astype(np.float32)).to(dev).contiguous()
    try:
        ref = weakref.ref(C, lambda _r, k=key: _cinv_drop(k))
    except TypeError:  # (a list: no weak reference, nothing to key on)
        return inv
    _cinv[key] = (ref, C._version if is_t else None, None if is_t else host.copy(), inv)
    return inv


class _BCLoss(_SeedRowLoss):
    tag = "bc"

    @staticmethod
    def _fwd(ctx, x, ld, yy, cinv, loss, dx):
        lib = _lib.load()
        ws = torch.empty(lib.ngnn_bc_loss_workspace_bytes(ctx.B), dtype=torch.uint8, device=x.device)
        _lib.check(lib.ngnn_bc_loss_fwd(
            _lib.ptr(x), ld, ctx.B, x.size(1), _lib.ptr(yy), _lib.ptr(cinv), cinv.stride(0), _lib.ptr(loss),
            _lib.ptr(dx), 0 if dx is None else dx.stride(0), _lib.ptr(ws), ws.numel(),
            _lib.stream_handle(x.device)), "ngnn_bc_loss_fwd")
        return (cinv,)

    @staticmethod
    def _bwd(ctx, x, ld, yy, saved, g, dx):
        (cinv,) = saved
        g = g.reshape(1).to(torch.float32).contiguous()
        _lib.check(_lib.load().ngnn_bc_loss_bwd(
            _lib.ptr(x), ld, ctx.B, x.size(1), _lib.ptr(yy), _lib.ptr(cinv), cinv.stride(0), _lib.ptr(g),
            _lib.ptr(dx), dx.stride(0), _lib.stream_handle(x.device)), "ngnn_bc_loss_bwd")


def backward_correction(output: torch.Tensor, labels: torch.Tensor, C, nbr_class: int, device=None,
                        batch_size: int | None = None) -> torch.Tensor:
    """Drop-in for the reference's ``backward_correction(output, labels, C,
    nbr_class, device)`` (losses.py:51-70): ``-mean(onehot(labels) @ inv(C) *
    log(clamp(softmax(output), 1e-5, 1 - 1e-5)))`` as two launches, its
    gradient written by the first.  ``C`` (numpy array or tensor) is inverted
    once and kept on the device (``_correction_inverse``).

    batch_size (extension): `output` is a block's whole logits [N, C] and the
    loss reads rows < batch_size; the gradient then comes back [N, C] from a
    zero-row buffer, marked for the SAGE stack's bounded backward.  No
    ignore_index (the reference's scatter_ would raise): a label outside
    [0, nbr_class) makes the loss NaN."""
    if not output.is_cuda:
        raise RuntimeError("ngnn.losses.backward_correction: GPU only (no CPU fallback)")
    if output.dim() != 2 or output.dtype not in (torch.float32, torch.bfloat16):
        raise ValueError("output must be a 2-D float32 (or bf16) tensor")
    nc = int(nbr_class)
    if output.size(1) != nc or tuple(C.shape) != (nc, nc):
        raise ValueError(f"output [N, {output.size(1)}] and C {tuple(C.shape)} do not match nbr_class {nc}")
    B = output.size(0) if batch_size is None else int(batch_size)
    labels = labels.reshape(-1)
    if B <= 0 or B > output.size(0) or labels.numel() < B:
        raise ValueError("batch_size out of range")
    if batch_size is None and labels.numel() != B:
        raise ValueError("labels must hold one label per row")
    cinv = _correction_inverse(C, output.device)
    y = labels.to(device=output.device, dtype=torch.int64)
    if output.dtype == torch.bfloat16:
        return _BF16SeedRows.apply(output, y, B, cinv, _BCLoss)
    return _BCLoss.apply(output, y, B, cinv)


# ---------------------------------------------------------------------------
# Contrastive discriminator loss (Discriminator_innerprod + BCEExeprtLoss,
# src/utils/data_utils.py:34-64)

def contrast_bad_indices(device=None, reset: bool = False) -> int:
    """How many ``index`` entries ``contrastive_loss`` met on ``device`` outside
    its rows (each makes that call's loss NaN).  Debugging only: reading the
    device counter synchronises (``contrastive_loss.bad_index`` is the counter
    itself, a device tensor)."""
    return read_counter("bad-index", device, "contrastive_loss", reset)


class _Contrast(torch.autograd.Function):
    """ngnn_contrast_fwd / _bwd.  B None: the gradients are fresh [N, H] zero
    tensors.  B given: each needed gradient is a zero-row buffer taken at
    forward time for this node alone (two contrastive terms pending in one
    step, one per model, get different buffers), its B leading rows cleared
    on the stream before the scatter."""

    @staticmethod
    def forward(ctx, h, hp, hn, index, B):
        dev = h.device
        N, H = h.shape
        rows = N if B is None else B
        M = index.numel()
        lib = _lib.load()
        out = torch.empty(3, dtype=torch.float32, device=dev)
        ws = torch.empty(lib.ngnn_contrast_workspace_bytes(M), dtype=torch.uint8, device=dev)
        bad = device_counter("bad-index", dev, "contrastive_loss")
        _lib.check(lib.ngnn_contrast_fwd(
            _lib.ptr(h), h.stride(0), _lib.ptr(hp), hp.stride(0), _lib.ptr(hn), hn.stride(0), rows, H,
            _lib.ptr(index), M, _lib.ptr(out), _lib.ptr(bad), _lib.ptr(ws), ws.numel(),
            _lib.stream_handle(dev)), "ngnn_contrast_fwd")
        ctx.holds = [None, None, None]
        if B is not None:
            for k in range(3):
                if ctx.needs_input_grad[k]:
                    ctx.holds[k] = _GradHold(dev, N, H, ("contrast", B))
        ctx.save_for_backward(h, hp, hn, index)
        ctx.ws, ctx.B, ctx.rows = ws, B, rows
        return out[0].clone()

    @staticmethod
    def backward(ctx, g):
        h, hp, hn, index = ctx.saved_tensors
        dev = h.device
        N, H = h.shape
        grads = [None, None, None]
        for k in range(3):
            if not ctx.needs_input_grad[k]:
                continue
            hold = ctx.holds[k]
            if hold is None:
                grads[k] = torch.zeros(N, H, dtype=torch.float32, device=dev)
            else:
                d, _ = hold.rows(N)
                d[:ctx.B].zero_()
                d._ngnn_nonzero_rows = ctx.B  # rows >= B are zero: the SAGE backward's row bound
                grads[k] = d
        g = g.reshape(1).to(torch.float32).contiguous()
        dh, dp, dn = grads
        _lib.check(_lib.load().ngnn_contrast_bwd(
            _lib.ptr(h), h.stride(0), _lib.ptr(hp), hp.stride(0), _lib.ptr(hn), hn.stride(0), ctx.rows, H,
            _lib.ptr(index), index.numel(), _lib.ptr(ctx.ws), _lib.ptr(g),
            _lib.ptr(dh), 0 if dh is None else dh.stride(0), _lib.ptr(dp), 0 if dp is None else dp.stride(0),
            _lib.ptr(dn), 0 if dn is None else dn.stride(0), _lib.stream_handle(dev)), "ngnn_contrast_bwd")
        return dh, dp, dn, None, None


def contrastive_loss(h: torch.Tensor, h_pos: torch.Tensor, h_neg: torch.Tensor, index: torch.Tensor,
                     batch_size: int | None = None) -> torch.Tensor:
    """``BCEExeprtLoss(n)(*Discriminator_innerprod()(h[index], h_pos[index],
    h_neg[index]))`` of the reference's train_ct step (pipeline_test.py:
    150-158) as one launch pair each way (``ngnn_contrast_fwd`` / ``_bwd``):
    ``mean softplus(-<h_i, h_pos_i>) + mean softplus(<h_i, h_neg_i>)`` over the
    rows ``index`` (a device int64 tensor, e.g. ``CTLoss``'s ``ind_noisy_m``),
    with no gathered copies and no ``[N, H]`` index-backward zero fills beyond
    the gradients themselves.  Deterministic forward; the backward adds with
    float atomics (duplicates accumulate as ``index_put_(accumulate=True)``;
    distinct indices: bitwise reproducible) and keeps the positive term's
    gradient at large logits, where torch's fp32 ``BCEWithLogitsLoss`` backward
    returns 0.

    batch_size=B (extension): the caller promises every index is < B (seed
    rows); each gradient is then a zero-row buffer whose B leading rows are
    cleared and scattered into, marked for the SAGE stack's bounded backward
    (``_ngnn_nonzero_rows``), and an index >= B counts as bad.  A bad index
    reads and writes nothing, makes the loss NaN and is counted on the device
    (``contrastive_loss.bad_index``: the int32 counter tensor, no sync;
    ``contrast_bad_indices()`` reads it).  No rows (``index`` empty): NaN, the
    reference's mean over nothing, without a launch.  fp32, GPU only."""
    for name, t in (("h", h), ("h_pos", h_pos), ("h_neg", h_neg)):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise RuntimeError(f"ngnn.losses.contrastive_loss: GPU only (no CPU fallback): {name}")
    if h.dim() != 2 or h.shape != h_pos.shape or h.shape != h_neg.shape:
        raise ValueError("h, h_pos, h_neg must be [N, H] tensors of the same shape")
    if not (h.dtype == h_pos.dtype == h_neg.dtype == torch.float32):
        raise TypeError("contrastive_loss: only float32 is supported")
    if not isinstance(index, torch.Tensor) or not index.is_cuda or index.dtype != torch.int64:
        raise ValueError("contrastive_loss: index must be a device int64 tensor")
    N, H = h.shape
    if batch_size is not None:
        batch_size = int(batch_size)
        if not 0 < batch_size <= N:
            raise ValueError(f"batch_size {batch_size} outside (0, {N}]")
    contrastive_loss.bad_index = device_counter("bad-index", h.device, "contrastive_loss")
    index = index.reshape(-1).contiguous()
    if H == 0:
        raise ValueError("contrastive_loss: H must be positive")
    if index.numel() == 0:  # (the entries refuse M == 0)
        return torch.full((), float("nan"), dtype=torch.float32, device=h.device)
    # stricter than rows_ld alone: a single row with a short stride is copied
    # too, so that _Contrast can pass stride(0) as every operand's ld
    a, p, n = (rows_ld(t if t.stride(0) >= H else t.contiguous())[0] for t in (h, h_pos, h_neg))
    return _Contrast.apply(a, p, n, index, batch_size)


contrastive_loss.bad_index = None


class Discriminator_innerprod(torch.nn.Module):
    """Drop-in for the reference's ``Discriminator_innerprod()``
    (data_utils.py:53-64): ``forward(H, Hp1, Hn)`` -> the two ``[M, 1]`` logit
    columns ``sum(H * Hp1, 1)`` and ``sum(H * Hn, 1)``.  Kept so that the
    reference's two-step call (gather, discriminate, ``BCEExeprtLoss``) runs
    unchanged; it is the torch composition on the device.  The fused path,
    which takes the row indices instead of gathered copies, is
    ``contrastive_loss``."""

    def forward(self, H, Hp1, Hn):
        if not (H.is_cuda and Hp1.is_cuda and Hn.is_cuda):
            raise RuntimeError("ngnn.losses.Discriminator_innerprod: GPU only (no CPU fallback)")
        logits_pa = torch.sum(torch.mul(H, Hp1), dim=1, keepdim=True)
        logits_n = torch.sum(torch.mul(H, Hn), dim=1, keepdim=True)
        return logits_pa, logits_n


class BCEExeprtLoss(torch.nn.Module):
    """Drop-in for the reference's ``BCEExeprtLoss(nbr_nodes)`` (data_utils.py:
    34-50; the name is the reference's spelling): ``forward(logits_p1,
    logits_n)`` -> ``BCEWithLogits(logits_p1, 1) + BCEWithLogits(logits_n, 0)``,
    each a mean, written as ``mean softplus(-p) + mean softplus(n)`` (the same
    value; its backward keeps sigma(-p) at large p).  The second half of the
    two-step call; the fused path is ``contrastive_loss``."""

    def __init__(self, nbr_nodes=None):
        super().__init__()
        self.nbr_nodes = nbr_nodes

    def forward(self, logits_p1, logits_n):
        if not (logits_p1.is_cuda and logits_n.is_cuda):
            raise RuntimeError("ngnn.losses.BCEExeprtLoss: GPU only (no CPU fallback)")
        pos = torch.squeeze(logits_p1)
        neg = torch.squeeze(logits_n)
        return torch.nn.functional.softplus(-pos).mean() + torch.nn.functional.softplus(neg).mean()


# ---------------------------------------------------------------------------
# Uncertainty-weighted consistency (get_uncertainty_batch, fix_cr:
# src/utils/losses.py:185-246; pipeline_ctp.py:127-135)

def get_uncertainty_batch(edge_index, y_pure: torch.Tensor, nbr_classes: int, device=None,
                          epsilon: float = 1e-16, rows: int | None = None) -> torch.Tensor:
    """Drop-in for the reference's ``get_uncertainty_batch(edge_index, y_pure,
    nbr_classes, device, epsilon)`` (losses.py:185-204): per node the entropy
    weight ``exp(-H(mean of exp(y_pure) over its out-neighbours) /
    log2(nbr_classes))``, grouped by ``edge_index[0]`` as the reference's
    ``A @ p`` -- ONE launch (``ngnn_nbr_uncertainty``) on the by-source CSR the
    model's backward builds anyway (``get_block(...).transposed()``), instead
    of ``edge_index.cpu()``, a scipy COO build, a sparse upload,
    ``torch.sparse.mm`` and a dozen elementwise launches.  No host wait, no
    atomics: bitwise reproducible for a given block.

    ``edge_index``: a ``[2, E]`` device tensor or a ``Block``.  ``rows``
    (extension): only ``w[:rows]`` is computed and returned -- all the
    pipeline reads (``w[:batch_size]``).  The result never carries a gradient
    (the reference is called under ``no_grad``).  ``nbr_classes < 2`` raises
    ``ValueError`` (the reference divides by ``log2(1) = 0``).  ``device`` is
    accepted and unused.  fp32, GPU only."""
    from .block import get_block
    if not isinstance(y_pure, torch.Tensor) or not y_pure.is_cuda:
        raise RuntimeError("ngnn.losses.get_uncertainty_batch: GPU only (no CPU fallback)")
    if isinstance(edge_index, torch.Tensor) and not edge_index.is_cuda:
        raise RuntimeError("ngnn.losses.get_uncertainty_batch: GPU only (no CPU fallback): edge_index")
    if int(nbr_classes) < 2:
        raise ValueError(f"get_uncertainty_batch: nbr_classes {nbr_classes} < 2")
    if y_pure.dim() != 2 or y_pure.dtype != torch.float32:
        raise ValueError("y_pure must be a 2-D float32 tensor")
    y, ld = rows_ld(y_pure.detach())
    N, C = y.shape
    blk = get_block(edge_index, N)
    if blk.n_src != N or blk.n_dst != N:
        raise ValueError(f"the block has {blk.n_src} x {blk.n_dst} nodes, y_pure {N} rows")
    R = N if rows is None else int(rows)
    if not 0 <= R <= N:
        raise ValueError(f"rows {rows} outside [0, {N}]")
    w = torch.empty(R, dtype=torch.float32, device=y.device)
    if R:
        csr = blk.transposed()
        _lib.check(_lib.load().ngnn_nbr_uncertainty(
            _lib.ptr(y), ld, N, C, _lib.ptr(csr.rowptr), _lib.ptr(csr.col),
            R, int(nbr_classes), float(epsilon), _lib.ptr(w), _lib.stream_handle(y.device)),
            "ngnn_nbr_uncertainty")
    return w


_FIX_CR_MODES = {("ce", True): 0, ("ce", False): 1, ("l2", True): 2, ("l2", False): 2}


class _FixCR(torch.autograd.Function):
    """ngnn_fix_cr_fwd / _bwd on the B rows it is handed (the caller's
    ``y[:B]`` views: torch's slice backward zero-fills the rows past B).  As
    _BCLoss, the forward writes the unit-scale gradient rows; the backward
    hands them over for the training step's unit gradient and otherwise
    rewrites them for the incoming device scalar (one launch, recomputed from
    the inputs)."""

    @staticmethod
    def forward(ctx, yp, yn, w, mode: int, p_cutoff: float):
        B, C = yp.shape
        dev = yp.device
        ctx.ld = rows_ld(yp)[1], rows_ld(yn)[1]  # (fix_cr passed both through rows_ld: no copy here)
        lib = _lib.load()
        loss = torch.empty((), dtype=torch.float32, device=dev)
        ws = torch.empty(lib.ngnn_fix_cr_workspace_bytes(B), dtype=torch.uint8, device=dev)
        # hard labels: nothing flows into y_pure (its gradient is None)
        dp = torch.empty(B, C, dtype=torch.float32, device=dev) if ctx.needs_input_grad[0] and mode else None
        dn = torch.empty(B, C, dtype=torch.float32, device=dev) if ctx.needs_input_grad[1] else None
        _lib.check(lib.ngnn_fix_cr_fwd(
            _lib.ptr(yp), ctx.ld[0], _lib.ptr(yn), ctx.ld[1], B, C, mode, p_cutoff, _lib.ptr(w),
            _lib.ptr(loss), _lib.ptr(dp), C, _lib.ptr(dn), C, _lib.ptr(ws), ws.numel(),
            _lib.stream_handle(dev)), "ngnn_fix_cr_fwd")
        ctx.save_for_backward(yp, yn, w)
        ctx.mode, ctx.p_cutoff, ctx.dp, ctx.dn = mode, p_cutoff, dp, dn
        ctx.want = (dp is not None, dn is not None)
        return loss

    @staticmethod
    def backward(ctx, g):
        yp, yn, w = ctx.saved_tensors
        B, C = yp.shape
        dp, dn = ctx.dp, ctx.dn
        ctx.dp = ctx.dn = None  # handed over once; a second backward recomputes
        fresh = (ctx.want[0] and dp is None) or (ctx.want[1] and dn is None)
        if fresh:
            dp = torch.empty(B, C, dtype=torch.float32, device=yp.device) if ctx.want[0] else None
            dn = torch.empty(B, C, dtype=torch.float32, device=yp.device) if ctx.want[1] else None
        if fresh or not getattr(g, "_ngnn_unit", False):
            g = g.reshape(1).to(torch.float32).contiguous()
            _lib.check(_lib.load().ngnn_fix_cr_bwd(
                _lib.ptr(yp), ctx.ld[0], _lib.ptr(yn), ctx.ld[1], B, C, ctx.mode, ctx.p_cutoff,
                _lib.ptr(w), _lib.ptr(g), _lib.ptr(dp), C, _lib.ptr(dn), C,
                _lib.stream_handle(yp.device)), "ngnn_fix_cr_bwd")
        return dp, dn, None, None, None


def fix_cr(y_pure: torch.Tensor, y_noisy: torch.Tensor, ind_noisy=None, batch_size: int = 512,
           name: str = "ce", T: float = 1.0, p_cutoff: float = 0.0, use_hard_labels: bool = True,
           w: torch.Tensor | None = None) -> torch.Tensor:
    """Drop-in for the reference's ``fix_cr(y_pure, y_noisy, ind_noisy,
    batch_size, name, T, p_cutoff, use_hard_labels, w)`` (losses.py:206-246):
    the consistency term between the log-probabilities of the pure and the
    noisy pass on the rows ``< batch_size`` -- ``name='ce'``: the cross
    entropy of ``exp(y_noisy)`` (fed as logits, as the reference) against the
    pseudo label of ``exp(y_pure)`` (its first argmax, or the probabilities
    themselves with ``use_hard_labels=False``, not detached), masked by
    ``max >= p_cutoff`` (a factor: the mean runs over all rows), weighted by
    ``w[:batch_size]``; ``name='l2'``: ``mse_loss(y_noisy, y_pure)``, which
    reads neither ``w`` nor ``p_cutoff``.  One launch pair
    (``ngnn_fix_cr_fwd``) writes the loss and both gradients' rows.

    ``B = min(batch_size, rows)``; ``w`` is detached; ``ind_noisy`` and ``T``
    are accepted and never read (the reference builds a mask from
    ``ind_noisy`` and drops it), so nothing goes to the host.  fp32, GPU
    only."""
    for nm, t in (("y_pure", y_pure), ("y_noisy", y_noisy)):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise RuntimeError(f"ngnn.losses.fix_cr: GPU only (no CPU fallback): {nm}")
    if name not in ("ce", "l2"):
        raise ValueError(f"fix_cr: name {name!r} is neither 'ce' nor 'l2'")
    if y_pure.dim() != 2 or y_pure.shape != y_noisy.shape:
        raise ValueError("y_pure, y_noisy must be [N, C] tensors of the same shape")
    if y_pure.dtype != torch.float32 or y_noisy.dtype != torch.float32:
        raise TypeError("fix_cr: only float32 is supported")
    B = min(int(batch_size), y_pure.size(0))
    if B <= 0 or y_pure.size(1) == 0:
        raise ValueError("fix_cr: no rows or no classes")
    mode = _FIX_CR_MODES[(name, bool(use_hard_labels))]
    yp, yn = rows_ld(y_pure[:B])[0], rows_ld(y_noisy[:B])[0]
    wb = None
    if w is not None and mode != 2:
        if not w.is_cuda:
            raise RuntimeError("ngnn.losses.fix_cr: GPU only (no CPU fallback): w")
        wb = w.detach().reshape(-1)
        if wb.numel() < B:
            raise ValueError(f"w holds {wb.numel()} entries, the loss reads {B}")
        wb = wb[:B].to(torch.float32).contiguous()
    return _FixCR.apply(yp, yn, wb, mode, float(p_cutoff))
