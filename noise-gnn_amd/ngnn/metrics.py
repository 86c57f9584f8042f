"""Epoch metrics and per-split accuracy on the device (``ngnn_step_metrics``
and ``ngnn_split_accuracy``).  GPU only: there is no CPU
fallback.

``EpochMeter`` replaces the host reads that end every batch of the
reference's training loops (``pipeline.py:120-125``, ``:164-165``:
``float(loss)``, ``int(out.argmax(dim=-1).eq(y).sum())``, ``100 *
pure_ratio``): one launch per step adds them into 64 bytes on the device and
``result()`` copies those once per epoch.  ``split_accuracy`` replaces the
evaluation's ``argmax``, three index gathers and three ``Evaluator.eval``
calls (``pipeline.py:182-195``) by one pass over the logits.
"""
from __future__ import annotations

import collections
import ctypes
import weakref

import torch

from . import _lib, _timing
from ._common import rows_ld

MAX_SCALARS = 4
MAX_SEGMENTS = 8

SplitAccuracy = collections.namedtuple("SplitAccuracy", ["accuracy", "counts", "pred", "confusion"])
SplitCounts = collections.namedtuple("SplitCounts", ["evaluated", "correct", "bad", "ignored"])


def confusion_max_classes() -> int:
    """The most classes ``split_accuracy(confusion=True)`` takes (the matrix
    is gathered in LDS)."""
    return int(_lib.load().ngnn_confusion_max_classes())


def _dtype_code(t: torch.Tensor, what: str) -> int:
    if t.dtype == torch.float32:
        return _lib.F32
    if t.dtype == torch.bfloat16:
        return _lib.BF16
    raise TypeError(f"{what}: logits must be float32 or bfloat16, got {t.dtype}")


def _logits_2d(t, what: str) -> tuple[torch.Tensor, int]:
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{what}: logits must be a torch tensor")
    if not t.is_cuda:
        raise RuntimeError(f"ngnn runs on the GPU only: {what}'s logits are on the CPU")
    if t.dim() != 2 or t.size(1) < 1:
        raise ValueError(f"{what}: logits must be [rows, C] with C >= 1, got shape {tuple(t.shape)}")
    # (rows of a column slice or of a padded buffer are read in place: only the columns must be dense)
    return rows_ld(t.detach())


def _labels_1d(y, dev, what: str) -> torch.Tensor:
    if not isinstance(y, torch.Tensor):
        raise TypeError(f"{what}: labels must be a torch tensor")
    if not y.is_cuda:
        raise RuntimeError(f"ngnn runs on the GPU only: {what}'s labels are on the CPU")
    if y.device != dev:
        raise ValueError(f"{what}: labels are on {y.device}, logits on {dev}")
    if y.dim() == 2 and y.size(1) == 1:
        y = y[:, 0]
    if y.dim() != 1:
        raise ValueError(f"{what}: labels must be [B] or [B, 1], got shape {tuple(y.shape)}")
    if y.is_floating_point() or y.is_complex() or y.dtype == torch.bool:
        raise TypeError(f"{what}: labels must be integers, got {y.dtype}")
    return y.detach().to(torch.int64).contiguous()


class EpochMeter:
    """The epoch's running ``steps``, ``rows``, ``correct``, ``bad_labels``
    and up to four named scalar sums, kept in eight 8-byte words on the
    device (include/ngnn.h, ``ngnn_step_metrics``).

        meter = EpochMeter(dev, names=("loss",))
        for batch in loader:
            step(batch.x, batch.edge_index, batch.y, batch_size=batch.batch_size)
            meter.update(step.out, batch.y, step.loss, batch_size=batch.batch_size)
        r = meter.result()      # the epoch's only host copy, 64 bytes
        train_loss, train_acc = r["means"]["loss"], meter.accuracy(split_idx["train"].size(0))

    ``update`` is one launch, no allocation (for float32 / bfloat16 logits
    with dense columns, int64 labels and float32 scalars) and no host wait,
    so it can follow a ``GraphedTrainStep`` replay or be captured in a graph
    of its own."""

    def __init__(self, device, names=("loss",)):
        names = tuple(names)
        if len(names) > MAX_SCALARS:
            raise ValueError(f"EpochMeter: at most {MAX_SCALARS} names, got {len(names)}")
        if len(set(names)) != len(names):
            raise ValueError(f"EpochMeter: names must differ, got {names}")
        dev = torch.device(device)
        if dev.type != "cuda":
            raise RuntimeError(f"ngnn runs on the GPU only: EpochMeter on {dev}")
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        self.device, self.names = dev, names
        self.acc = torch.zeros(8, dtype=torch.int64, device=dev)

    def reset(self) -> None:
        self.acc.zero_()

    def update(self, logits, y, *scalars, batch_size=None, ignore_index: int = -100) -> None:
        """Adds one step: rows ``< batch_size`` of ``logits`` (``[>= B, C]``,
        the step's whole output or its seed rows; no slice needed) against
        ``y[:batch_size]`` (``[>= B]`` or ``[>= B, 1]``; ``batch_size=None``:
        all of ``y``), and one device scalar (a one-element float tensor, or
        ``None``) per name.  Returns ``None``; nothing is read on the host."""
        lg, ld = _logits_2d(logits, "EpochMeter.update")
        dev = lg.device
        if dev != self.device:
            raise ValueError(f"EpochMeter.update: logits are on {dev}, the meter on {self.device}")
        yy = _labels_1d(y, dev, "EpochMeter.update")
        B = yy.numel() if batch_size is None else int(batch_size)
        if B < 0 or B > yy.numel() or B > lg.size(0):
            raise ValueError(f"EpochMeter.update: batch_size {B} with {yy.numel()} labels and {lg.size(0)} rows")
        if len(scalars) > len(self.names):
            raise ValueError(f"EpochMeter.update: {len(scalars)} scalars for names {self.names}")
        ptrs = [0] * MAX_SCALARS
        keep = []
        for k, s in enumerate(scalars):
            if s is None:
                continue
            if not isinstance(s, torch.Tensor):
                raise TypeError(f"EpochMeter.update: {self.names[k]} must be a device tensor (a Python number "
                                "would have been read on the host already)")
            if not s.is_cuda:
                raise RuntimeError(f"ngnn runs on the GPU only: EpochMeter.update's {self.names[k]} is on the CPU")
            if s.numel() != 1 or s.device != dev:
                raise ValueError(f"EpochMeter.update: {self.names[k]} must hold one element on {dev}")
            s = s.detach()
            if s.dtype != torch.float32:
                s = s.float()
            keep.append(s)
            ptrs[k] = s.data_ptr()
        C = lg.size(1)
        with _timing.span("step_metrics", B * (C * lg.element_size() + 8) + 64):
            rc = _lib.load().ngnn_step_metrics(_lib.ptr(lg), ld, _dtype_code(lg, "EpochMeter.update"), B, C,
                                               _lib.ptr(yy), int(ignore_index), ptrs[0], ptrs[1], ptrs[2], ptrs[3],
                                               self.acc.data_ptr(), _lib.stream_handle(dev))
        _lib.check(rc, "ngnn_step_metrics")

    def result(self) -> dict:
        """``steps``, ``rows``, ``correct``, ``bad_labels``, ``sums[name]``
        and ``means[name] = sum / steps`` (the reference's ``total /
        len(train_loader)``): the meter's only host copy, 64 bytes, made by
        every call (a captured ``update`` may have run since the last)."""
        host = self.acc.cpu().numpy()
        steps, rows, correct, bad = (int(v) for v in host[:4])
        sums_f = host[4:].view("float64")
        sums = {n: float(sums_f[k]) for k, n in enumerate(self.names)}
        means = {n: (v / steps if steps else float("nan")) for n, v in sums.items()}
        return dict(steps=steps, rows=rows, correct=correct, bad_labels=bad, sums=sums, means=means)

    def accuracy(self, denominator=None) -> float:
        """``correct / denominator``; the reference divides by
        ``split_idx['train'].size(0)``.  Default: the rows counted."""
        r = self.result()
        d = r["rows"] if denominator is None else int(denominator)
        return r["correct"] / d if d else float("nan")


_SPLITS_KEPT = 8
_splits: collections.OrderedDict = collections.OrderedDict()  # key -> (weakrefs, versions, rows on dev, bounds)


def _split_rows(split_idx: dict, dev):
    """cat(split_idx.values()) on `dev` as int64 and the segment bounds,
    built (and uploaded) once per dict of tensors: cached by the identity and
    ``_version`` of every tensor, dropped with any of them."""
    names = tuple(split_idx)
    lists = tuple(split_idx.values())
    for n, t in zip(names, lists):
        if not isinstance(t, torch.Tensor) or t.dim() != 1:
            raise TypeError(f"split_accuracy: split {n!r} must be a 1-D index tensor")
        if t.is_floating_point() or t.is_complex() or t.dtype == torch.bool:
            raise TypeError(f"split_accuracy: split {n!r} must hold integers, got {t.dtype}")
    key = (names, tuple(id(t) for t in lists), dev)
    vers = tuple(t._version for t in lists)
    ent = _splits.get(key)
    if ent is not None and ent[1] == vers and all(r() is t for r, t in zip(ent[0], lists)):
        _splits.move_to_end(key)
        return ent[2], ent[3]
    bounds = [0]
    for t in lists:
        bounds.append(bounds[-1] + t.numel())
    if bounds[-1]:
        rows = torch.cat([t.detach().to(dev, torch.int64) for t in lists]).contiguous()
    else:
        rows = torch.zeros(0, dtype=torch.int64, device=dev)
    refs = tuple(weakref.ref(t, lambda _r, k=key: _splits.pop(k, None)) for t in lists)
    _splits[key] = (refs, vers, rows, bounds)
    _splits.move_to_end(key)
    if len(_splits) > _SPLITS_KEPT:
        _splits.popitem(last=False)
    return rows, bounds


def split_accuracy(out, y, split_idx=None, *, return_pred: bool = False, confusion: bool = False,
                   return_counts: bool = False, ignore_index: int = -100):
    """Accuracy of the ``[N, C]`` logits ``out`` against the labels ``y``
    (``[N]`` or ``[N, 1]``) over each index list of ``split_idx`` -- a dict
    of int64 index tensors, as ``dataset.get_idx_split()`` gives; ``None``:
    one split ``"all"`` over every row -- in one pass (``ngnn_split_accuracy``).
    Returns ``{name: correct / len(list)}``, the OGB Evaluator's and
    ``accuracy_score``'s quotient (``nan`` for an empty list), from one host
    copy of the counts.  Lists may overlap and repeat ids; every entry
    counts, as ``y_pred[split_idx[k]]`` does.

    With ``return_pred``, ``confusion`` or ``return_counts`` the result is
    ``SplitAccuracy(accuracy, counts, pred, confusion)``: ``counts[name]`` a
    ``SplitCounts(evaluated, correct, bad, ignored)`` of Python ints;
    ``pred[name]`` the int64 device tensor of the list's argmaxes (views of
    one tensor; for ``split_idx=None`` ``pred["all"]`` is ``[N]``);
    ``confusion`` the int64 ``[C, C]`` device matrix over all lists,
    ``[label, argmax]`` (``C <= confusion_max_classes()``).  What was not
    asked for is ``None``.

    An index outside ``[0, N)``, or a label outside ``[0, C)`` that is not
    ``ignore_index``, raises ``ValueError`` naming the split (the reference
    raises ``IndexError``); such a row is never read."""
    lg, ld = _logits_2d(out, "split_accuracy")
    dev = lg.device
    yy = _labels_1d(y, dev, "split_accuracy")
    N, C = lg.shape
    if yy.numel() != N:
        raise ValueError(f"split_accuracy: {yy.numel()} labels for {N} rows")
    if split_idx is None:
        names, rows, bounds = ("all",), None, [0, N]
    else:
        if not isinstance(split_idx, dict) or not 1 <= len(split_idx) <= MAX_SEGMENTS:
            raise ValueError(f"split_accuracy: split_idx must be a dict of 1 to {MAX_SEGMENTS} index tensors")
        names = tuple(split_idx)
        rows, bounds = _split_rows(split_idx, dev)
    S, M = len(names), bounds[-1]
    if confusion and C > confusion_max_classes():
        raise ValueError(f"split_accuracy: confusion needs C <= {confusion_max_classes()}, got {C}")
    counts = torch.empty(S, 4, dtype=torch.int64, device=dev)
    pred = torch.empty(M, dtype=torch.int64, device=dev) if return_pred else None
    conf = torch.empty(C, C, dtype=torch.int64, device=dev) if confusion else None
    host_bounds = (ctypes.c_int64 * (S + 1))(*bounds)
    with _timing.span("split_accuracy", M * (C * lg.element_size() + 16 + (8 if return_pred else 0))):
        rc = _lib.load().ngnn_split_accuracy(_lib.ptr(lg), ld, _dtype_code(lg, "split_accuracy"), N, C, _lib.ptr(yy),
                                             int(ignore_index), _lib.ptr(rows), M, S, host_bounds,
                                             counts.data_ptr(), _lib.ptr(pred), _lib.ptr(conf),
                                             _lib.stream_handle(dev))
    _lib.check(rc, "ngnn_split_accuracy")
    host = counts.cpu().tolist()  # the call's one host copy
    per = {n: SplitCounts(*host[s]) for s, n in enumerate(names)}
    for n, c in per.items():
        if c.bad:
            raise ValueError(f"split_accuracy: split {n!r} has {c.bad} entries with an index outside [0, {N}) "
                             f"or a label outside [0, {C})")
    acc = {n: (per[n].correct / (bounds[s + 1] - bounds[s]) if bounds[s + 1] > bounds[s] else float("nan"))
           for s, n in enumerate(names)}
    if not (return_pred or confusion or return_counts):
        return acc
    preds = {n: pred[bounds[s]:bounds[s + 1]] for s, n in enumerate(names)} if return_pred else None
    return SplitAccuracy(acc, per, preds, conf)
