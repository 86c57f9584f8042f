"""CPU checks of the shuffle_pos and contrastive-loss entries (added within
ABI 22): all resolve, are bound and declared, the version stayed 22, the
Python names exist and refuse CPU tensors, and every argument error comes
back as its negative code before anything touches a device."""
import os
import re

import pytest
import torch

from ngnn import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ngnn.h")
NAMES = ("ngnn_shuffle_rows", "ngnn_contrast_workspace_bytes", "ngnn_contrast_fwd", "ngnn_contrast_bwd")
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
    assert raw.count("Added within ABI 22") >= 4
    # the header states the draw: both salts and the aliasing rule
    assert "0x632BE59BD9B4E019" in raw and "0xD1B54A32D192ED03" in raw
    assert "must not alias" in raw


def test_python_names_exist_and_refuse_the_cpu():
    import ngnn
    from ngnn import losses, ops
    assert ngnn.shuffle_pos is ops.shuffle_pos and "shuffle_pos" in ngnn.__all__
    x = torch.zeros(4, 6)
    with pytest.raises(RuntimeError):
        ops.shuffle_pos(x, prob=0.5, seed=1)
    idx = torch.zeros(2, dtype=torch.long)
    with pytest.raises(RuntimeError):
        losses.contrastive_loss(x, x, x, idx)
    with pytest.raises(RuntimeError):
        losses.contrastive_loss(x, x, x, idx, batch_size=2)
    disc, crit = losses.Discriminator_innerprod(), losses.BCEExeprtLoss(4)
    with pytest.raises(RuntimeError):
        disc(x, x, x)
    with pytest.raises(RuntimeError):
        crit(torch.zeros(4, 1), torch.zeros(4, 1))
    assert callable(losses.contrast_bad_indices) and hasattr(losses.contrastive_loss, "bad_index")


def test_workspace_size():
    fn = _lib.load().ngnn_contrast_workspace_bytes
    assert fn(0) == 0 and fn(-3) == 0
    last = 0
    for M in (1, 2, 64, 205, 1025, 1 << 20):
        assert fn(M) >= 16 * M  # a_i and b_i, kept in double
        assert fn(M) >= last
        last = fn(M)


def _shuffle(lib, x=P, ldx=100, n=300, F=100, m=70, seed=1, out=P + 4096, ldo=100):
    return lib.ngnn_shuffle_rows(x, ldx, n, F, m, seed, out, ldo, None)


def test_shuffle_argument_errors_return_before_launch():
    lib = _lib.load()
    assert _shuffle(lib, x=None) == _lib.E_ARG
    assert _shuffle(lib, out=None) == _lib.E_ARG
    assert _shuffle(lib, n=-1) == _lib.E_ARG
    assert _shuffle(lib, F=-1, m=0, ldx=0, ldo=0) == _lib.E_ARG
    assert _shuffle(lib, m=-1) == _lib.E_ARG
    assert _shuffle(lib, m=101) == _lib.E_ARG            # m > F
    assert _shuffle(lib, ldx=99) == _lib.E_SHAPE
    assert _shuffle(lib, ldo=99) == _lib.E_SHAPE
    assert _shuffle(lib, n=1 << 31) == _lib.E_RANGE
    assert _shuffle(lib, F=65536, m=0, ldx=65536, ldo=65536) == _lib.E_RANGE
    # nothing to move: success, nothing read (no pointer needed)
    assert _shuffle(lib, x=None, out=None, n=0) == _lib.OK
    assert _shuffle(lib, x=None, out=None, F=0, m=0) == _lib.OK


def _fwd(lib, h=P, ldh=256, hp=P, ldp=256, hn=P, ldn=256, n=1000, F=256, idx=P, M=205, out=P, bad=P, ws=P,
         ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = lib.ngnn_contrast_workspace_bytes(M)
    return lib.ngnn_contrast_fwd(h, ldh, hp, ldp, hn, ldn, n, F, idx, M, out, bad, ws, ws_bytes, None)


def _bwd(lib, h=P, ldh=256, hp=P, ldp=256, hn=P, ldn=256, n=1000, F=256, idx=P, M=205, ws=P, g=P, dh=P,
         lddh=256, dhp=P, lddp=256, dhn=P, lddn=256):
    return lib.ngnn_contrast_bwd(h, ldh, hp, ldp, hn, ldn, n, F, idx, M, ws, g, dh, lddh, dhp, lddp, dhn, lddn,
                                 None)


def test_contrast_argument_errors_return_before_launch():
    lib = _lib.load()
    for name in ("h", "hp", "hn", "idx", "out", "ws"):
        assert _fwd(lib, **{name: None}) == _lib.E_ARG, name
    assert _fwd(lib, M=0, ws_bytes=1024) == _lib.E_ARG       # the entries refuse an empty selection
    assert _fwd(lib, M=-1, ws_bytes=1024) == _lib.E_ARG
    assert _fwd(lib, n=0) == _lib.E_ARG
    assert _fwd(lib, F=0) == _lib.E_ARG
    for name in ("ldh", "ldp", "ldn"):
        assert _fwd(lib, **{name: 255}) == _lib.E_SHAPE, name
    assert _fwd(lib, n=1 << 31) == _lib.E_RANGE
    assert _fwd(lib, M=1 << 31, ws_bytes=1 << 40) == _lib.E_RANGE
    assert _fwd(lib, F=1 << 31, ldh=1 << 31, ldp=1 << 31, ldn=1 << 31) == _lib.E_RANGE
    need = lib.ngnn_contrast_workspace_bytes(205)
    assert _fwd(lib, ws_bytes=need - 1) == _lib.E_WORKSPACE
    assert _fwd(lib, ws_bytes=0) == _lib.E_WORKSPACE
    assert _fwd(lib, ws=P + 4) == _lib.E_WORKSPACE           # misaligned
    for name in ("h", "hp", "hn", "idx", "ws", "g"):
        assert _bwd(lib, **{name: None}) == _lib.E_ARG, name
    assert _bwd(lib, M=0) == _lib.E_ARG
    assert _bwd(lib, n=0) == _lib.E_ARG
    assert _bwd(lib, F=0) == _lib.E_ARG
    for name in ("ldh", "ldp", "ldn", "lddh", "lddp", "lddn"):
        assert _bwd(lib, **{name: 255}) == _lib.E_SHAPE, name
    assert _bwd(lib, dh=None, lddh=0, lddp=255) == _lib.E_SHAPE  # an absent gradient's stride is not looked at
    assert _bwd(lib, n=1 << 31) == _lib.E_RANGE
    # no gradient wanted: nothing to launch
    assert _bwd(lib, dh=None, lddh=0, dhp=None, lddp=0, dhn=None, lddn=0) == _lib.OK
    for rc in (_lib.E_ARG, _lib.E_SHAPE, _lib.E_RANGE, _lib.E_WORKSPACE):
        assert b"unknown" not in lib.ngnn_strerror(rc)
