"""CPU checks of the metrics entries (added within ABI 22): all three resolve,
are bound and declared, the version stayed 22, the header names the one host
pointer, the Python names exist and refuse CPU tensors, and every argument
error comes back as its negative code before anything touches a device."""
import ctypes
import os
import re

import pytest
import torch

from ngnn import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ngnn.h")
NAMES = ("ngnn_confusion_max_classes", "ngnn_step_metrics", "ngnn_split_accuracy")
P = 256  # a dummy non-null, aligned pointer: a call that got past its checks would fault


def test_symbols_resolve_bound_and_declared_within_abi_22():
    lib = _lib.load()
    raw = open(HEADER).read()
    txt = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES
        assert re.search(r"\b" + name + r"\s*\(", txt), name
    assert lib.ngnn_abi_version() == 22 and _lib.ABI_VERSION == 22
    assert int(re.search(r"#define NGNN_ABI_VERSION (\d+)", raw).group(1)) == 22
    assert raw.count("Added within ABI 22") >= 7
    assert lib.ngnn_confusion_max_classes() == 128
    section = raw[raw.index("ngnn_split_accuracy:"):]
    assert "HOST pointer" in section  # bounds: the one exception to "device pointers only"


def test_python_names_exist_and_refuse_the_cpu():
    import ngnn
    from ngnn import metrics
    assert ngnn.EpochMeter is metrics.EpochMeter and "EpochMeter" in ngnn.__all__
    assert ngnn.split_accuracy is metrics.split_accuracy and "split_accuracy" in ngnn.__all__
    assert ngnn.metrics is metrics and "metrics" in ngnn.__all__
    out, y = torch.zeros(8, 4), torch.zeros(8, dtype=torch.long)
    with pytest.raises(RuntimeError):
        metrics.split_accuracy(out, y)
    with pytest.raises(RuntimeError):
        metrics.split_accuracy(out, y.view(-1, 1), {"train": torch.arange(4)})
    with pytest.raises(RuntimeError):
        metrics.EpochMeter("cpu")
    with pytest.raises(ValueError):
        metrics.EpochMeter("cuda:0", names=("a", "b", "c", "d", "e"))


def _step(lib, logits=P, ld=47, dtype=_lib.F32, B=64, C=47, y=P + 65536, ignore=-100, s=(None,) * 4,
          acc=P + 131072):
    return lib.ngnn_step_metrics(logits, ld, dtype, B, C, y, ignore, *s, acc, None)


def test_step_metrics_argument_errors_return_before_launch():
    lib = _lib.load()
    for name in ("logits", "y", "acc"):
        assert _step(lib, **{name: None}) == _lib.E_ARG, name
    assert _step(lib, acc=None, B=0) == _lib.E_ARG
    assert _step(lib, C=0, ld=0) == _lib.E_ARG
    assert _step(lib, C=-2, ld=47) == _lib.E_ARG
    assert _step(lib, B=-1) == _lib.E_ARG
    assert _step(lib, ld=46) == _lib.E_SHAPE
    assert _step(lib, ld=0) == _lib.E_SHAPE
    assert _step(lib, B=1 << 31) == _lib.E_RANGE
    assert _step(lib, B=1 << 40) == _lib.E_RANGE
    assert _step(lib, C=1 << 31, ld=1 << 31) == _lib.E_RANGE
    assert _step(lib, dtype=2) == _lib.E_DTYPE
    assert _step(lib, dtype=-1) == _lib.E_DTYPE
    for off in (1, 2, 4, 7):
        assert _step(lib, acc=P + 131072 + off) == _lib.E_ALIGN, off
    assert _step(lib, acc=P + 131072 + 4, s=(P, P, P, P), dtype=_lib.BF16) == _lib.E_ALIGN


def _bounds(*b):
    return (ctypes.c_int64 * len(b))(*b)


def _split(lib, logits=P, ld=47, dtype=_lib.F32, N=1000, C=47, y=P + 65536, ignore=-100, rows=P + 131072, M=300,
           S=3, bounds=(0, 100, 200, 300), counts=P + 196608, pred=None, confusion=None):
    b = None if bounds is None else _bounds(*bounds)
    return lib.ngnn_split_accuracy(logits, ld, dtype, N, C, y, ignore, rows, M, S, b, counts, pred, confusion, None)


def test_split_accuracy_argument_errors_return_before_launch():
    lib = _lib.load()
    limit = lib.ngnn_confusion_max_classes()
    assert _split(lib, S=0, bounds=(0,)) == _lib.E_ARG
    assert _split(lib, S=9, bounds=(0,) * 9 + (300,)) == _lib.E_ARG
    assert _split(lib, S=-1) == _lib.E_ARG
    # bounds: bounds[0] = 0, non-decreasing, bounds[S] = M
    assert _split(lib, bounds=(1, 100, 200, 300)) == _lib.E_ARG
    assert _split(lib, bounds=(0, 200, 100, 300)) == _lib.E_ARG
    assert _split(lib, bounds=(0, 100, 200, 299)) == _lib.E_ARG
    assert _split(lib, bounds=(0, 100, 200, 301)) == _lib.E_ARG
    assert _split(lib, bounds=(0, -1, 200, 300)) == _lib.E_ARG
    assert _split(lib, bounds=None) == _lib.E_ARG
    for name in ("logits", "y", "counts"):
        assert _split(lib, **{name: None}) == _lib.E_ARG, name
    assert _split(lib, rows=None) == _lib.E_ARG  # (no list: M must be N)
    assert _split(lib, C=0, ld=0) == _lib.E_ARG
    assert _split(lib, N=-1) == _lib.E_ARG
    assert _split(lib, M=-1, bounds=(0, 0, 0, -1)) == _lib.E_ARG
    assert _split(lib, ld=46) == _lib.E_SHAPE
    assert _split(lib, N=1 << 31) == _lib.E_RANGE
    assert _split(lib, M=1 << 31, bounds=(0, 100, 200, 1 << 31)) == _lib.E_RANGE
    assert _split(lib, C=1 << 31, ld=1 << 31) == _lib.E_RANGE
    assert _split(lib, dtype=5) == _lib.E_DTYPE
    assert _split(lib, C=limit + 1, ld=limit + 1, confusion=P) == _lib.E_SHAPE
    assert _split(lib, C=limit + 1, ld=limit, confusion=None) == _lib.E_SHAPE  # (ld < C)
    for rc in (_lib.E_ARG, _lib.E_SHAPE, _lib.E_RANGE, _lib.E_DTYPE, _lib.E_ALIGN):
        assert b"unknown" not in lib.ngnn_strerror(rc)
