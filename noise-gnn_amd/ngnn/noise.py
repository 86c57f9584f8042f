"""Label-noise injection (the reference's ``src/utils/noise.py``): the
transition matrix on the host in numpy, the per-node draw in one launch on
the device (``ngnn_flip_labels``).  GPU only: there is no CPU
fallback.

``noise_matrix`` repeats the reference's numpy operations in their order, so
under the same ``np.random.seed`` the matrix is bitwise the reference's.  The
draw is this library's own (include/ngnn.h): a pure function of ``(seed, node
index, label, matrix)``, so every rank of a data-parallel run computes the
same noisy labels with no broadcast, and a run can be repeated.
"""
from __future__ import annotations

import collections

import numpy as np
import torch

from . import _lib, _timing
from ._common import device_counter, read_counter

NOISE_TYPES = ("sym", "next_pair", "rand_pair", "aim_pair")
# the launch geometry include/ngnn.h documents for ngnn_flip_labels
BLOCK_THREADS = 1024
NODES_PER_THREAD_TRIP = 4

LabelNoiseStats = collections.namedtuple("LabelNoiseStats", ["noise_or_not", "counts", "bad"])


def noise_matrix(nbr_classes: int, noise_type: str = "sym", prob: float = 0.3) -> np.ndarray:
    """The ``[C, C]`` float64 transition matrix of ``flip_label``
    (``noise.py:11-50``): row ``l`` is the distribution of the noisy label of
    a node whose clean label is ``l``.  The two random types draw their two
    ``np.random.permutation`` from numpy's global generator, as the reference
    does.  An unknown ``noise_type`` (the reference prints and then fails with
    a ``NameError``) and ``aim_pair`` with ``nbr_classes <= 5`` (up to 3 the
    reference returns an empty array its caller cannot unpack, at 4 and 5 it
    fails with an ``IndexError`` while it fills the matrix) are ``ValueError``."""
    if noise_type not in NOISE_TYPES:
        raise ValueError(f"noise_matrix: wrong noise type {noise_type!r}, one of {NOISE_TYPES}")
    C = int(nbr_classes)
    if noise_type == "sym":
        return np.diag(np.array([1 - prob] * C), k=0) + (np.ones((C, C)) - np.diag(np.ones(C), k=0)) * (prob / (C - 1))
    if noise_type == "next_pair":
        return (np.diag(np.array([1 - prob] * C), k=0) + np.diag(np.array([prob] * (C - 1)), k=1)
                + np.diag(np.array([prob]), k=-(C - 1)))
    numbers = np.arange(C)
    if noise_type == "rand_pair":
        perm1 = np.random.permutation(C)
        perm2 = np.random.permutation(C)
        pairs = np.vstack((numbers[perm1], numbers[perm2]))
    else:
        fixed = np.array([[0, 1, 2], [3, 4, 5]])
        m = fixed.shape[1]
        if C <= fixed.max():
            # (the reference returns an empty array up to 3 classes and fails with an IndexError at 4 and 5)
            raise ValueError(f"noise_matrix: aim_pair's fixed pairs name classes 0..{fixed.max()}, got {C} classes")
        perm1 = np.random.permutation(C - m)
        perm2 = np.random.permutation(C - m)
        numbers1 = np.setdiff1d(numbers, fixed[0, :])
        numbers2 = np.setdiff1d(numbers, fixed[1, :])
        pairs = np.concatenate((np.vstack((numbers1[perm1], numbers2[perm2])), fixed), axis=1)
    noise_mat = np.diag(np.array([1 - prob] * C), k=0)
    mat = np.zeros((C, C))
    for i in range(C):
        mat[pairs[0, i], pairs[1, i]] = prob
    noise_mat += mat
    return noise_mat


def _checked_matrix(noise_mat, C: int) -> np.ndarray:
    M = np.asarray(noise_mat, dtype=np.float64)
    if M.shape != (C, C):
        raise ValueError(f"flip_label: noise_mat must be [{C}, {C}], got shape {M.shape}")
    if not (M >= 0).all():  # (a NaN fails too)
        raise ValueError("flip_label: noise_mat has a negative (or NaN) entry")
    if not (np.abs(M.sum(axis=1) - 1.0) <= 1e-6).all():
        raise ValueError("flip_label: every row of noise_mat must sum to 1 (within 1e-6)")
    return M


def threshold_table(noise_mat) -> tuple[np.ndarray, np.ndarray]:
    """``(thr, last)`` of include/ngnn.h: ``thr`` uint32 ``[C, C]`` with
    ``thr[l][k] = min(floor(cumsum(M[l])[k] * 2^32), 2^32 - 1)`` for ``k <
    last[l]``, ``last`` int32 ``[C]`` the last class of non-zero probability
    in each row.  The threshold of every ``k >= last[l]`` is 2^32, which no
    32-bit draw reaches: those entries of ``thr`` are never read (they hold
    0xFFFFFFFF)."""
    M = np.asarray(noise_mat, dtype=np.float64)
    C = M.shape[0]
    cs = np.cumsum(M, axis=1)
    t = np.minimum(np.floor(cs * 4294967296.0), 4294967295.0).astype(np.uint64)
    last = (C - 1 - np.argmax(M[:, ::-1] > 0, axis=1)).astype(np.int32)
    t[np.arange(C)[None, :] >= last[:, None]] = 0xFFFFFFFF
    return t.astype(np.uint32), last


_TABLES_KEPT = 16
_tables: collections.OrderedDict = collections.OrderedDict()  # (device index, C, matrix bytes) -> int32 [C*C + C]


def _device_table(M: np.ndarray, dev: torch.device) -> torch.Tensor:
    """thr then last, one int32 tensor on `dev`, built and uploaded once per
    matrix: cached by the matrix's contents (C x C doubles to hash, cheaper
    than the table), the oldest of more than a few matrices dropped."""
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    key = (idx, M.shape[0], M.tobytes())
    tab = _tables.get(key)
    if tab is None:
        thr, last = threshold_table(M)
        host = np.concatenate([thr.view(np.int32).ravel(), last])
        tab = _tables[key] = torch.from_numpy(host).to(dev)
        if len(_tables) > _TABLES_KEPT:
            _tables.popitem(last=False)
    return tab


def label_noise_bad_labels(device=None, reset: bool = False) -> int:
    """How many labels ``flip_label`` met on ``device`` outside ``[0,
    nbr_classes)`` (each is copied unchanged; the reference raises an
    ``IndexError``).  Debugging only: reading the device counter
    synchronises."""
    return read_counter("bad-label", device, "flip_label", reset)


def max_classes() -> int:
    """The largest ``nbr_classes`` the kernel takes (its table and histogram
    live in LDS)."""
    return int(_lib.load().ngnn_flip_labels_max_classes())


def flip_label(labels: torch.Tensor, nbr_classes: int, noise_type: str = "sym", prob: float = 0.3, *,
               seed: int | None = None, noise_mat=None, device=None, out: torch.Tensor | None = None,
               index_offset: int = 0, return_stats: bool = False):
    """The reference's ``flip_label(labels, nbr_classes, noise_type, prob)``
    (``src/utils/noise.py:6-61``): every label ``l`` is redrawn from row ``l``
    of the transition matrix.  Returns ``(noisy_labels, noise_mat)`` as the
    reference does -- ``noisy_labels`` int64 ``[N]`` on the labels' device,
    ``noise_mat`` the numpy matrix -- and with ``return_stats=True`` a third
    item ``LabelNoiseStats(noise_or_not, counts, bad)``: bool ``[N]``
    (``noisy == clean``), int64 ``[C, C]`` (``counts[l][j]`` nodes went from
    ``l`` to ``j``) and this device's bad-label counter, all device tensors.

    One launch (``ngnn_flip_labels``) instead of a Python loop over the nodes;
    no device synchronisation and no device-to-host copy (a matrix's first
    use uploads its threshold table, kept on the device afterwards).  ``labels`` is
    ``[N]`` or ``[N, 1]`` (OGB's ``data.y``), contiguous or not; labels on the
    CPU raise unless ``device=`` is given, which moves them there once.

    The draw is this library's own (include/ngnn.h), a pure function of
    ``(seed, index_offset + i, labels[i], noise_mat)``: flipping
    ``labels[a:b]`` with ``index_offset=a`` gives rows ``a:b`` of the whole
    flip.  ``seed=None`` draws a 62-bit seed from torch's default CPU
    generator (host only), so ``torch.manual_seed`` makes a run repeatable.
    ``noise_mat=`` skips ``noise_matrix``: a ``[C, C]`` non-negative matrix
    whose rows sum to 1 within 1e-6.  ``out=`` (int64 ``[N]``, contiguous,
    not overlapping ``labels``) is written and returned, so a tensor a graph
    or a captured step holds can be flipped again in place of a new one.  A
    label outside ``[0, nbr_classes)`` is copied unchanged and counted
    (``label_noise_bad_labels``)."""
    if not isinstance(labels, torch.Tensor):
        raise TypeError("flip_label: labels must be a torch tensor")
    if device is not None:
        labels = labels.to(device)
    if not labels.is_cuda:
        raise RuntimeError("ngnn runs on the GPU only: flip_label's labels are on the CPU (pass device=)")
    if labels.dim() == 2 and labels.size(1) == 1:
        labels = labels[:, 0]
    if labels.dim() != 1:
        raise ValueError(f"flip_label: labels must be [N] or [N, 1], got shape {tuple(labels.shape)}")
    if labels.is_floating_point() or labels.is_complex() or labels.dtype == torch.bool:
        raise TypeError(f"flip_label: labels must be integers, got {labels.dtype}")
    C = int(nbr_classes)
    limit = max_classes()
    if not 1 <= C <= limit:
        raise ValueError(f"flip_label: nbr_classes must be in [1, {limit}], got {C}")
    index_offset = int(index_offset)
    if index_offset < 0:
        raise ValueError(f"flip_label: index_offset must not be negative, got {index_offset}")
    M = noise_matrix(C, noise_type, prob) if noise_mat is None else noise_mat
    Mc = _checked_matrix(M, C)
    dev = labels.device
    y = labels.detach().to(torch.int64).contiguous()
    N = y.numel()
    if out is None:
        out = torch.empty(N, dtype=torch.int64, device=dev)
    else:
        if not (isinstance(out, torch.Tensor) and out.dtype == torch.int64 and out.device == dev
                and out.dim() == 1 and out.numel() == N and out.is_contiguous()):
            raise ValueError(f"flip_label: out must be a contiguous int64 [{N}] tensor on {dev}")
        if N and out.data_ptr() < y.data_ptr() + 8 * N and y.data_ptr() < out.data_ptr() + 8 * N:
            raise ValueError("flip_label: out must not alias labels")
    if seed is None:
        seed = int(torch.randint(0, 1 << 62, (1,)).item())
    tab = _device_table(Mc, dev)
    bad = device_counter("bad-label", dev, "flip_label")
    clean = counts = None
    if return_stats:
        clean = torch.empty(N, dtype=torch.bool, device=dev)
        counts = torch.zeros(C, C, dtype=torch.int64, device=dev)
    with _timing.span("flip_labels", 17 * N + 4 * C * (C + 1)):
        rc = _lib.load().ngnn_flip_labels(_lib.ptr(y), N, C, tab.data_ptr(), tab.data_ptr() + 4 * C * C,
                                          int(seed) & 0xFFFFFFFFFFFFFFFF, index_offset, _lib.ptr(out),
                                          _lib.ptr(clean), _lib.ptr(counts), _lib.ptr(bad),
                                          _lib.stream_handle(dev))
    _lib.check(rc, "ngnn_flip_labels")
    if return_stats:
        return out, M, LabelNoiseStats(clean, counts, bad)
    return out, M
