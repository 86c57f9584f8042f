"""CPU checks of the block-free inference entries (ABI 22): the header, the
ctypes table and the library agree on the version, both entries resolve, and
argument errors come back as negative codes before anything touches a device."""
import os
import re

from ngnn import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ngnn.h")


def test_abi_is_22_everywhere():
    lib = _lib.load()
    m = re.search(r"#define NGNN_ABI_VERSION (\d+)", open(HEADER).read())
    assert int(m.group(1)) == 22
    assert _lib.ABI_VERSION == 22
    assert lib.ngnn_abi_version() == 22


def test_infer_symbols_resolve_and_are_declared():
    lib = _lib.load()
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in ("ngnn_infer_draw", "ngnn_infer_narrow"):
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES
        assert re.search(r"\b" + name + r"\s*\(", txt), name


def _draw(lib, r0, n_rows, bs, fanout, ws_bytes=1 << 20):
    # dummy non-null pointers: a call that got past its checks would fault, so
    # every case below must return first
    return lib.ngnn_infer_draw(16, 16, None, r0, n_rows, bs, fanout, 7, 1, 16, 16, 16, ws_bytes, None)


def _narrow(lib, r0, n_rows, bs, fanout, reduce=1, ldz=48, Fo=47):
    return lib.ngnn_infer_narrow(16, 16, None, r0, n_rows, bs, fanout, 7, 1, 16, ldz, 16, 48, None, Fo,
                                 reduce, 0, 16, 47, None)


def test_argument_errors_return_before_launch():
    lib = _lib.load()
    for call in (_draw, _narrow):
        assert call(lib, 0, 100, 64, 65) == _lib.E_SHAPE        # fanout > 64
        assert call(lib, 32, 100, 64, 15) == _lib.E_ARG         # r0 not a multiple of batch_size
        assert call(lib, 0, -1, 64, 15) == _lib.E_ARG           # negative size
        assert call(lib, 0, 100, 0, 15) == _lib.E_ARG           # no batch size
        assert call(lib, 0, 1 << 27, 64, 16) == _lib.E_RANGE    # n_rows * fanout >= 2^31
    assert _draw(lib, 0, 5000, 64, 15, ws_bytes=4) == _lib.E_WORKSPACE
    assert lib.ngnn_infer_draw_workspace_bytes(5000) >= 4 * 5
    assert lib.ngnn_infer_draw_workspace_bytes(-1) == 0
    assert _narrow(lib, 0, 100, 64, 15, reduce=2) == _lib.E_ARG   # max is not linear
    assert _narrow(lib, 0, 100, 64, 15, ldz=47) == _lib.E_SHAPE   # z rows are 16-B pieces
    assert _narrow(lib, 0, 100, 64, 15, ldz=44) == _lib.E_SHAPE   # ... of at least ceil4(Fo)
    # zero rows: a no-op success (no pointer is read)
    assert _narrow(lib, 0, 0, 64, 15) == 0
    for rc in (_lib.E_ARG, _lib.E_SHAPE, _lib.E_RANGE, _lib.E_WORKSPACE):
        assert b"unknown" not in lib.ngnn_strerror(rc)
