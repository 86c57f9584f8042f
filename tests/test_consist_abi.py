"""CPU checks of the neighbourhood-uncertainty and consistency-loss entries
(added within ABI 22): all resolve, are bound and declared, the version
stayed 22, the Python names exist and refuse CPU tensors, and every argument
error comes back as its negative code before anything touches a device."""
import inspect
import os
import re

import pytest
import torch

from ngnn import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ngnn.h")
NAMES = ("ngnn_nbr_uncertainty", "ngnn_fix_cr_workspace_bytes", "ngnn_fix_cr_fwd", "ngnn_fix_cr_bwd")
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
    assert raw.count("Added within ABI 22") >= 5
    # the header states the direction and the tie rule
    assert "grouped by SOURCE" in raw and "FIRST index" in raw


def test_python_names_exist_and_refuse_the_cpu():
    from ngnn import losses
    sig = inspect.signature(losses.get_uncertainty_batch)
    assert list(sig.parameters) == ["edge_index", "y_pure", "nbr_classes", "device", "epsilon", "rows"]
    assert sig.parameters["epsilon"].default == 1e-16 and sig.parameters["rows"].default is None
    sig = inspect.signature(losses.fix_cr)
    assert list(sig.parameters) == ["y_pure", "y_noisy", "ind_noisy", "batch_size", "name", "T", "p_cutoff",
                                    "use_hard_labels", "w"]
    assert [sig.parameters[k].default for k in ("batch_size", "name", "T", "p_cutoff", "use_hard_labels", "w")] \
        == [512, "ce", 1.0, 0.0, True, None]
    y = torch.log_softmax(torch.zeros(4, 6), dim=1)
    ei = torch.tensor([[0, 1], [1, 2]])
    with pytest.raises(RuntimeError):
        losses.get_uncertainty_batch(ei, y, 6)
    with pytest.raises(RuntimeError):
        losses.get_uncertainty_batch(ei, y, 6, rows=2)
    for kw in ({}, {"name": "l2"}, {"use_hard_labels": False}, {"w": torch.ones(4)}):
        with pytest.raises(RuntimeError):
            losses.fix_cr(y, y, None, batch_size=2, **kw)


def test_workspace_size():
    fn = _lib.load().ngnn_fix_cr_workspace_bytes
    assert fn(0) == 0 and fn(-3) == 0
    last = 0
    for B in (1, 2, 64, 205, 1025, 1 << 20):
        assert fn(B) >= 4 * B  # one row term each
        assert fn(B) >= last
        last = fn(B)


def _unc(lib, logp=P, ld=47, n=300, C=47, rowptr=P, col=P, R=300, k=47, eps=1e-16, w=P):
    return lib.ngnn_nbr_uncertainty(logp, ld, n, C, rowptr, col, R, k, eps, w, None)


def test_uncertainty_argument_errors_return_before_launch():
    lib = _lib.load()
    for name in ("logp", "rowptr", "w"):
        assert _unc(lib, **{name: None}) == _lib.E_ARG, name
    assert _unc(lib, n=-1, R=0) == _lib.E_ARG
    assert _unc(lib, C=-1) == _lib.E_ARG
    assert _unc(lib, R=-1) == _lib.E_ARG
    assert _unc(lib, R=301) == _lib.E_ARG                 # R > n_rows
    assert _unc(lib, k=1) == _lib.E_ARG and _unc(lib, k=0) == _lib.E_ARG
    assert _unc(lib, ld=46) == _lib.E_SHAPE
    assert _unc(lib, n=1 << 31) == _lib.E_RANGE
    assert _unc(lib, n=1 << 32, R=1 << 31) == _lib.E_RANGE
    assert _unc(lib, C=65536, ld=65536) == _lib.E_RANGE
    # no rows to write: success, nothing read (no pointer needed)
    assert _unc(lib, logp=None, rowptr=None, col=None, w=None, R=0) == _lib.OK
    assert _unc(lib, logp=None, rowptr=None, col=None, w=None, n=0, R=0) == _lib.OK


def _fwd(lib, yp=P, ldp=47, yn=P, ldn=47, B=300, C=47, mode=0, cut=0.5, w=P, loss=P, dp=P, lddp=47, dn=P,
         lddn=47, ws=P, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = lib.ngnn_fix_cr_workspace_bytes(B)
    return lib.ngnn_fix_cr_fwd(yp, ldp, yn, ldn, B, C, mode, cut, w, loss, dp, lddp, dn, lddn, ws, ws_bytes, None)


def _bwd(lib, yp=P, ldp=47, yn=P, ldn=47, B=300, C=47, mode=0, cut=0.5, w=P, g=P, dp=P, lddp=47, dn=P, lddn=47):
    return lib.ngnn_fix_cr_bwd(yp, ldp, yn, ldn, B, C, mode, cut, w, g, dp, lddp, dn, lddn, None)


def test_fix_cr_argument_errors_return_before_launch():
    lib = _lib.load()
    for name in ("yp", "yn", "loss", "ws"):
        assert _fwd(lib, **{name: None}) == _lib.E_ARG, name
    assert _fwd(lib, B=0, ws_bytes=1024) == _lib.E_ARG and _fwd(lib, B=-1, ws_bytes=1024) == _lib.E_ARG
    assert _fwd(lib, C=0) == _lib.E_ARG
    assert _fwd(lib, mode=3) == _lib.E_ARG and _fwd(lib, mode=-1) == _lib.E_ARG
    for name in ("ldp", "ldn", "lddp", "lddn"):
        assert _fwd(lib, **{name: 46}) == _lib.E_SHAPE, name
    assert _fwd(lib, dp=None, lddp=0, lddn=46) == _lib.E_SHAPE  # an absent gradient's stride is not looked at
    assert _fwd(lib, B=1 << 31, ws_bytes=1 << 40) == _lib.E_RANGE
    assert _fwd(lib, C=65536, ldp=65536, ldn=65536, lddp=65536, lddn=65536) == _lib.E_RANGE
    need = lib.ngnn_fix_cr_workspace_bytes(300)
    assert _fwd(lib, ws_bytes=need - 1) == _lib.E_WORKSPACE
    assert _fwd(lib, ws_bytes=0) == _lib.E_WORKSPACE
    assert _fwd(lib, ws=P + 4) == _lib.E_WORKSPACE           # misaligned
    for name in ("yp", "yn", "g"):
        assert _bwd(lib, **{name: None}) == _lib.E_ARG, name
    assert _bwd(lib, B=0) == _lib.E_ARG and _bwd(lib, C=0) == _lib.E_ARG and _bwd(lib, mode=3) == _lib.E_ARG
    for name in ("ldp", "ldn", "lddp", "lddn"):
        assert _bwd(lib, **{name: 46}) == _lib.E_SHAPE, name
    assert _bwd(lib, B=1 << 31) == _lib.E_RANGE
    assert _bwd(lib, C=65536, ldp=65536, ldn=65536, lddp=65536, lddn=65536) == _lib.E_RANGE
    # no gradient wanted: nothing to launch
    assert _bwd(lib, dp=None, lddp=0, dn=None, lddn=0) == _lib.OK
    for rc in (_lib.E_ARG, _lib.E_SHAPE, _lib.E_RANGE, _lib.E_WORKSPACE):
        assert b"unknown" not in lib.ngnn_strerror(rc)
