"""CPU checks of the node-noise entries (added within ABI 22): both resolve,
are bound and declared, the version stayed 22, and every argument error comes
back as its negative code before anything touches a device."""
import os
import re

from ngnn import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ngnn.h")
NAMES = ("ngnn_node_noise_fwd", "ngnn_node_noise_bwd")
P = 16  # a dummy non-null pointer: a call that got past its checks would fault


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
    assert "Added within ABI 22" in raw
    assert int(re.search(r"#define NGNN_NOISE_SIGN (\d+)", raw).group(1)) == _lib.NOISE_SIGN


def _fwd(lib, x=P, ldx=128, noise=P, ldn=128, n_nodes=200, n_id=P, n_rows=67, F=128, flags=0, out=P,
         ldo=128):
    return lib.ngnn_node_noise_fwd(x, ldx, noise, ldn, n_nodes, n_id, n_rows, F, 0.1, flags, out, ldo,
                                   None, None)


def _bwd(lib, g=P, ldg=128, x=P, ldx=128, noise=P, ldn=128, n_nodes=200, n_id=P, scatter=1, n_rows=67,
         F=128, flags=0, dnoise=P, ldd=128):
    return lib.ngnn_node_noise_bwd(g, ldg, x, ldx, noise, ldn, n_nodes, n_id, scatter, n_rows, F, 0.1,
                                   flags, dnoise, ldd, None, None)


def test_argument_errors_return_before_launch():
    lib = _lib.load()
    for call in (_fwd, _bwd):
        assert call(lib, n_rows=-1) == _lib.E_ARG                    # negative sizes
        assert call(lib, F=-1) == _lib.E_ARG
        assert call(lib, n_nodes=-1) == _lib.E_ARG
        assert call(lib, ldn=127) == _lib.E_SHAPE                    # ld* < F
        assert call(lib, n_id=None, n_rows=67) == _lib.E_ARG         # no ids: n_rows must be n_nodes
        assert call(lib, noise=None) == _lib.E_ARG                   # null data pointers
        assert call(lib, flags=2) == _lib.E_ARG                      # unknown flag
        assert call(lib, n_rows=1 << 31) == _lib.E_RANGE
        assert call(lib, n_rows=0) == 0                              # a no-op: no pointer is read
        assert call(lib, n_rows=0, n_nodes=0, n_id=None, noise=None) == 0
    assert _fwd(lib, ldx=127) == _lib.E_SHAPE
    assert _fwd(lib, ldo=100) == _lib.E_SHAPE
    assert _fwd(lib, x=None) == _lib.E_ARG
    assert _fwd(lib, out=None) == _lib.E_ARG
    assert _fwd(lib, n_rows=0, x=None, out=None) == 0
    assert _bwd(lib, ldg=127) == _lib.E_SHAPE
    assert _bwd(lib, ldd=127) == _lib.E_SHAPE
    assert _bwd(lib, g=None) == _lib.E_ARG
    assert _bwd(lib, dnoise=None) == _lib.E_ARG
    assert _bwd(lib, scatter=2) == _lib.E_ARG
    # x is read only under NGNN_NOISE_SIGN: its pointer and ldx are checked only then
    assert _bwd(lib, x=None, flags=_lib.NOISE_SIGN) == _lib.E_ARG
    assert _bwd(lib, ldx=127, flags=_lib.NOISE_SIGN) == _lib.E_SHAPE
    assert _bwd(lib, n_rows=0, x=None, ldx=0, g=None, dnoise=None) == 0
    for rc in (_lib.E_ARG, _lib.E_SHAPE, _lib.E_RANGE):
        assert b"unknown" not in lib.ngnn_strerror(rc)
