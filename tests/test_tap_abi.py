"""CPU checks of the hidden-state tap entries (added within ABI 22): both
resolve, are bound and declared, the version stayed 22, and every argument
error comes back as its negative code before anything touches a device."""
import os
import re

from ngnn import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ngnn.h")
NAMES = ("ngnn_dropout_rows", "ngnn_tap_grad")
P, Q = 16, 32  # dummy non-null pointers: a call that got past its checks would fault


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


def _drop(lib, h=P, ldh=128, n_rows=67, nrd=None, F=128, p=0.5, out=Q, ldo=128):
    return lib.ngnn_dropout_rows(h, ldh, n_rows, nrd, F, p, 7, None, out, ldo, None)


def _grad(lib, dy=P, ldy=128, xd=P, ldx=128, dh=P, ldg=128, h=P, ldh=128, n_rows=67, F=128, dz=Q, ldz=128):
    return lib.ngnn_tap_grad(dy, ldy, xd, ldx, 2.0, dh, ldg, h, ldh, n_rows, None, F, dz, ldz, None)


def test_argument_errors_return_before_launch():
    lib = _lib.load()
    for call in (_drop, _grad):
        assert call(lib, n_rows=-1) == _lib.E_ARG   # negative sizes
        assert call(lib, F=-1) == _lib.E_ARG
        assert call(lib, ldh=127) == _lib.E_SHAPE   # a leading dimension below F
        assert call(lib, h=None) == _lib.E_ARG      # null required pointers
        assert call(lib, n_rows=1 << 31) == _lib.E_RANGE
        assert call(lib, n_rows=0) == _lib.OK       # a no-op: no pointer is read
    assert _drop(lib, ldo=100) == _lib.E_SHAPE
    assert _drop(lib, out=None) == _lib.E_ARG
    assert _drop(lib, out=P) == _lib.E_ARG          # out must not alias h
    for p in (-0.1, 1.5, float("nan")):
        assert _drop(lib, p=p) == _lib.E_ARG
    assert _drop(lib, n_rows=0, h=None, out=None) == _lib.OK
    for ld in ("ldy", "ldx", "ldg", "ldz"):
        assert _grad(lib, **{ld: 127}) == _lib.E_SHAPE
    assert _grad(lib, dh=None) == _lib.E_ARG
    assert _grad(lib, dz=None) == _lib.E_ARG
    # the nullable operands: their leading dimensions are checked only with them
    assert _grad(lib, n_rows=0, xd=None, ldx=0) == _lib.OK
    assert _grad(lib, n_rows=0, dy=None, ldy=0, xd=None, ldx=0) == _lib.OK
    assert _grad(lib, n_rows=0, dy=None, dh=None, h=None, dz=None) == _lib.OK
    for rc in (_lib.E_ARG, _lib.E_SHAPE, _lib.E_RANGE):
        assert b"unknown" not in lib.ngnn_strerror(rc)
