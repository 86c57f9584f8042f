"""CPU checks of the rewiring entries (added within ABI 22): both resolve, are
bound and declared, the version stayed 22, the workspace is far below N x N,
and every argument error comes back as its negative code before anything
touches a device."""
import os
import re

from ngnn import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ngnn.h")
NAMES = ("ngnn_topk_rewire_workspace_bytes", "ngnn_topk_rewire")
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
    assert raw.count("Added within ABI 22") >= 2


def test_python_name_is_exported():
    import ngnn
    from ngnn import ops
    assert ngnn.topk_rewire is ops.topk_rewire and "topk_rewire" in ngnn.__all__


def _call(lib, h=P, ldh=256, n=1000, F=256, src=P, dst=P, e=5000, k2=200, pos=P, pos_cap=5200, neg=P,
          neg_cap=5200, counts=P, ws=P, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = lib.ngnn_topk_rewire_workspace_bytes(n, F, e, k2)
    return lib.ngnn_topk_rewire(h, ldh, n, F, src, dst, e, k2, pos, pos_cap, neg, neg_cap, counts, None, None,
                                ws, ws_bytes, None)


def test_workspace_never_holds_n_by_n():
    lib = _lib.load()
    n, F, e = 21600, 256, 60000
    k2 = 2 * int(n * 0.2)
    ws = lib.ngnn_topk_rewire_workspace_bytes(n, F, e, k2)
    assert ws > n * F * 4
    assert ws < n * n * 4 // 8  # one dense fp32 matrix is 1.87 GB; the composition holds several
    # O(N F + E + k2) plus bounded lists: doubling N adds what its rows and diagonal need, no more
    ws2 = lib.ngnn_topk_rewire_workspace_bytes(2 * n, F, e, k2)
    assert ws2 - ws < 2 * n * (F + 16) * 4 + n * 200
    assert lib.ngnn_topk_rewire_workspace_bytes(0, F, e, 0) == 0
    assert lib.ngnn_topk_rewire_workspace_bytes(65536, F, e, k2) == 0
    assert lib.ngnn_topk_rewire_workspace_bytes(-1, F, e, k2) == 0


def test_argument_errors_return_before_launch():
    lib = _lib.load()
    assert _call(lib, n=-1, ws_bytes=1 << 40) == _lib.E_ARG          # negative sizes
    assert _call(lib, F=-1, ws_bytes=1 << 40) == _lib.E_ARG
    assert _call(lib, e=-1, ws_bytes=1 << 40) == _lib.E_ARG
    assert _call(lib, k2=-2, ws_bytes=1 << 40) == _lib.E_ARG
    assert _call(lib, pos_cap=-1) == _lib.E_ARG
    assert _call(lib, neg_cap=-1) == _lib.E_ARG
    assert _call(lib, ldh=-1) == _lib.E_ARG
    assert _call(lib, ldh=255) == _lib.E_SHAPE                       # ldh < F
    assert _call(lib, n=65536, ws_bytes=1 << 40) == _lib.E_RANGE     # a flat index must fit 32 bits
    assert _call(lib, n=10, k2=102, ws_bytes=1 << 40) == _lib.E_RANGE  # k2 > n * n
    assert _call(lib, e=(1 << 29) + 1, ws_bytes=1 << 40) == _lib.E_RANGE
    assert _call(lib, pos_cap=1 << 31) == _lib.E_RANGE
    for name in ("h", "src", "dst", "pos", "neg", "counts", "ws"):   # null pointers
        assert _call(lib, **{name: None}) == _lib.E_ARG, name
    assert _call(lib, ws=P + 8) == _lib.E_ALIGN
    assert _call(lib, pos=P + 4) == _lib.E_ALIGN
    need = lib.ngnn_topk_rewire_workspace_bytes(1000, 256, 5000, 200)
    assert need > 0
    assert _call(lib, ws_bytes=need - 1) == _lib.E_WORKSPACE
    assert _call(lib, ws_bytes=0) == _lib.E_WORKSPACE
    # n == 0: a no-op, no pointer is read
    assert _call(lib, n=0, k2=0, h=None, src=None, dst=None, pos=None, neg=None, counts=None, ws=None,
                 ws_bytes=0) == 0
    # edges are not read without edges, h not without columns: their pointers may be absent
    assert _call(lib, e=0, src=None, dst=None, ws_bytes=0) == _lib.E_WORKSPACE
    assert _call(lib, F=0, ldh=0, h=None, ws_bytes=0) == _lib.E_WORKSPACE
    for rc in (_lib.E_ARG, _lib.E_SHAPE, _lib.E_RANGE, _lib.E_ALIGN, _lib.E_WORKSPACE):
        assert b"unknown" not in lib.ngnn_strerror(rc)
