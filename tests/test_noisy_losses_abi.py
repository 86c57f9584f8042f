"""CPU checks of the backward-correction and CoDi loss entries (added within
ABI 22): all resolve, are bound and declared, the version stayed 22, the
Python names exist, and every argument error comes back as its negative code
before anything touches a device."""
import os
import re

import pytest
import torch

from ngnn import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ngnn.h")
NAMES = ("ngnn_bc_loss_workspace_bytes", "ngnn_bc_loss_fwd", "ngnn_bc_loss_bwd",
         "ngnn_codi_loss_workspace_bytes", "ngnn_codi_loss_fwd", "ngnn_codi_loss_bwd")
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
    assert raw.count("Added within ABI 22") >= 3


def test_python_names_exist_and_refuse_the_cpu():
    from ngnn.losses import CoDiLoss, backward_correction
    crit = CoDiLoss(None)
    assert crit.co_lambda == 0.1 and crit.ignore_index == -100 and crit.return_indices is False
    y = torch.zeros(4, 3)
    with pytest.raises(RuntimeError):
        backward_correction(y, torch.zeros(4, dtype=torch.long), torch.eye(3), 3)
    with pytest.raises(RuntimeError):
        crit(y, y, torch.zeros(4, dtype=torch.long), 0.2, None, None)


def test_workspace_sizes():
    lib = _lib.load()
    for B in (1, 5, 1024, 8192):
        assert lib.ngnn_bc_loss_workspace_bytes(B) >= 4 * B
        # CTLoss's layout (k_ct_bwd reads it as is) plus the two key rows
        assert lib.ngnn_codi_loss_workspace_bytes(B) >= lib.ngnn_ct_loss_workspace_bytes(B) + 8 * B - 512
        assert lib.ngnn_codi_loss_workspace_bytes(B) >= 4 * (8 * B + 2)
    for fn in (lib.ngnn_bc_loss_workspace_bytes, lib.ngnn_codi_loss_workspace_bytes):
        assert fn(0) == 0 and fn(-3) == 0


def _bc_fwd(lib, x=P, ld=47, B=300, C=47, y=P, cinv=P, ldc=47, loss=P, dx=P, ldd=47, ws=P, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = lib.ngnn_bc_loss_workspace_bytes(B)
    return lib.ngnn_bc_loss_fwd(x, ld, B, C, y, cinv, ldc, loss, dx, ldd, ws, ws_bytes, None)


def _bc_bwd(lib, x=P, ld=47, B=300, C=47, y=P, cinv=P, ldc=47, g=P, dx=P, ldd=47):
    return lib.ngnn_bc_loss_bwd(x, ld, B, C, y, cinv, ldc, g, dx, ldd, None)


def _codi_fwd(lib, y1=P, ld1=47, y2=P, ld2=47, B=300, C=47, yn=P, R=240, lam=0.1, ind=P, clean=P, n_noise=900,
              out=P, i1=P, i2=P, js=None, ws=P, ws_bytes=None, err=P):
    if ws_bytes is None:
        ws_bytes = lib.ngnn_codi_loss_workspace_bytes(B)
    return lib.ngnn_codi_loss_fwd(y1, ld1, y2, ld2, B, C, yn, -100, R, lam, ind, clean, n_noise, out, i1, i2,
                                  js, ws, ws_bytes, err, None)


def _codi_bwd(lib, model=0, y=P, ld=47, B=300, C=47, yn=P, ws=P, g=P, dy=P, ldd=47):
    return lib.ngnn_codi_loss_bwd(model, y, ld, B, C, yn, -100, ws, g, dy, ldd, None)


def test_bc_argument_errors_return_before_launch():
    lib = _lib.load()
    for name in ("x", "y", "cinv", "loss", "ws"):
        assert _bc_fwd(lib, **{name: None}) == _lib.E_ARG, name
    assert _bc_fwd(lib, B=0, ws_bytes=1024) == _lib.E_ARG
    assert _bc_fwd(lib, B=-1, ws_bytes=1024) == _lib.E_ARG
    assert _bc_fwd(lib, C=0) == _lib.E_ARG
    assert _bc_fwd(lib, ld=46) == _lib.E_SHAPE       # ld < C
    assert _bc_fwd(lib, ldc=46) == _lib.E_SHAPE
    assert _bc_fwd(lib, ldd=46) == _lib.E_SHAPE
    assert _bc_fwd(lib, B=1 << 31, ws_bytes=1 << 40) == _lib.E_RANGE
    need = lib.ngnn_bc_loss_workspace_bytes(300)
    assert _bc_fwd(lib, ws_bytes=need - 1) == _lib.E_WORKSPACE
    assert _bc_fwd(lib, ws_bytes=0) == _lib.E_WORKSPACE
    assert _bc_fwd(lib, ws=P + 4) == _lib.E_WORKSPACE  # misaligned
    for name in ("x", "y", "cinv", "g", "dx"):
        assert _bc_bwd(lib, **{name: None}) == _lib.E_ARG, name
    assert _bc_bwd(lib, B=0) == _lib.E_ARG
    assert _bc_bwd(lib, ld=46) == _lib.E_SHAPE
    assert _bc_bwd(lib, ldc=46) == _lib.E_SHAPE
    assert _bc_bwd(lib, ldd=46) == _lib.E_SHAPE
    assert _bc_bwd(lib, C=1 << 31, ld=1 << 31, ldc=1 << 31, ldd=1 << 31) == _lib.E_RANGE


def test_codi_argument_errors_return_before_launch():
    lib = _lib.load()
    for name in ("y1", "y2", "yn", "out", "i1", "i2", "ws", "err"):
        assert _codi_fwd(lib, **{name: None}) == _lib.E_ARG, name
    assert _codi_fwd(lib, B=0, R=0, ws_bytes=1 << 20) == _lib.E_ARG
    assert _codi_fwd(lib, C=0) == _lib.E_ARG
    assert _codi_fwd(lib, R=-1) == _lib.E_ARG
    assert _codi_fwd(lib, R=301) == _lib.E_ARG          # num_remember > B
    assert _codi_fwd(lib, n_noise=0) == _lib.E_ARG      # noise_or_not given without a size
    assert _codi_fwd(lib, ld1=46) == _lib.E_SHAPE       # ld < C
    assert _codi_fwd(lib, ld2=46) == _lib.E_SHAPE
    assert _codi_fwd(lib, B=8193, ws_bytes=1 << 20) == _lib.E_SHAPE  # B > 8192
    need = lib.ngnn_codi_loss_workspace_bytes(300)
    assert _codi_fwd(lib, ws_bytes=need - 1) == _lib.E_WORKSPACE
    # CTLoss's (smaller) workspace does not do
    assert _codi_fwd(lib, ws_bytes=lib.ngnn_ct_loss_workspace_bytes(300)) == _lib.E_WORKSPACE
    assert _codi_fwd(lib, ws=P + 8) == _lib.E_WORKSPACE
    assert _codi_bwd(lib, model=2) == _lib.E_ARG
    for name in ("y", "yn", "ws", "g", "dy"):
        assert _codi_bwd(lib, **{name: None}) == _lib.E_ARG, name
    assert _codi_bwd(lib, ld=46) == _lib.E_SHAPE
    assert _codi_bwd(lib, ldd=46) == _lib.E_SHAPE
    assert _codi_bwd(lib, B=8193) == _lib.E_SHAPE
    for rc in (_lib.E_ARG, _lib.E_SHAPE, _lib.E_RANGE, _lib.E_WORKSPACE):
        assert b"unknown" not in lib.ngnn_strerror(rc)
