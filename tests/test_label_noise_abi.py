"""CPU checks of the flip_label entries (added within ABI 22): both resolve,
are bound and declared, the version stayed 22, the header states the draw's
salt and the aliasing rule, the Python names exist and refuse CPU labels, and
every argument error comes back as its negative code before anything touches
a device."""
import os
import re

import numpy as np
import pytest
import torch

from ngnn import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ngnn.h")
NAMES = ("ngnn_flip_labels_max_classes", "ngnn_flip_labels")
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
    assert raw.count("Added within ABI 22") >= 6
    # the header states the draw: its salt (not one of the two already in use) and the aliasing rule
    section = raw[raw.index("ngnn_flip_labels:"):]
    assert "0xA0761D6478BD642F" in section
    assert "must not alias y" in section


def test_python_names_exist_and_refuse_the_cpu():
    import ngnn
    from ngnn import noise
    assert ngnn.flip_label is noise.flip_label and "flip_label" in ngnn.__all__
    assert ngnn.noise_matrix is noise.noise_matrix and "noise_matrix" in ngnn.__all__
    assert callable(noise.label_noise_bad_labels)
    y = torch.zeros(8, dtype=torch.long)
    with pytest.raises(RuntimeError):
        noise.flip_label(y, 4, "sym", 0.3, seed=1)
    with pytest.raises(RuntimeError):
        noise.flip_label(y.view(-1, 1), 4, noise_mat=np.eye(4), seed=1)


def _flip(lib, y=P, n=300, C=47, thr=P + 4096, last=P + 65536, seed=1, i0=0, out=P + 131072, clean=None,
          counts=None, bad=None):
    return lib.ngnn_flip_labels(y, n, C, thr, last, seed, i0, out, clean, counts, bad, None)


def test_argument_errors_return_before_launch():
    lib = _lib.load()
    limit = lib.ngnn_flip_labels_max_classes()
    assert limit >= 100
    for name in ("y", "out", "thr", "last"):
        assert _flip(lib, **{name: None}) == _lib.E_ARG, name
    assert _flip(lib, n=-1) == _lib.E_ARG
    assert _flip(lib, C=0) == _lib.E_ARG
    assert _flip(lib, C=-3) == _lib.E_ARG
    assert _flip(lib, i0=-1) == _lib.E_ARG
    assert _flip(lib, n=1 << 31) == _lib.E_RANGE
    assert _flip(lib, n=1 << 40) == _lib.E_RANGE
    assert _flip(lib, C=limit + 1) == _lib.E_SHAPE
    assert _flip(lib, C=limit + 1, clean=P, counts=P, bad=P) == _lib.E_SHAPE
    assert _flip(lib, C=1 << 20) == _lib.E_SHAPE
    # nothing to flip: success, nothing read (no pointer needed)
    assert _flip(lib, y=None, out=None, thr=None, last=None, n=0) == _lib.OK
    assert _flip(lib, y=None, out=None, thr=None, last=None, n=0, C=limit) == _lib.OK
    for rc in (_lib.E_ARG, _lib.E_SHAPE, _lib.E_RANGE):
        assert b"unknown" not in lib.ngnn_strerror(rc)
