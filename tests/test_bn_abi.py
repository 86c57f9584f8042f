"""CPU checks of the fused ReLU-BatchNorm-dropout entries (added within ABI
22): the symbols resolve, are bound and declared, the version stayed 22, every
argument error comes back as its negative code with a message before anything
touches a device, the workspace size follows the slab count, and the Python
op exists with the stated signature and leaves CPU tensors to torch."""
import inspect
import os
import re

import torch
import torch.nn as nn

import ngnn
from ngnn import _lib, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ngnn.h")
NAMES = ("ngnn_bn_slab_rows", "ngnn_bn_workspace_bytes", "ngnn_bn_fwd_train", "ngnn_bn_fwd_eval", "ngnn_bn_bwd")
P = 256  # a dummy non-null, aligned pointer: a call that got past its checks would fault
ARG_ERRORS = (_lib.E_ARG, _lib.E_SHAPE, _lib.E_RANGE, _lib.E_WORKSPACE)


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
    block = raw[raw.index("fused ReLU-BatchNorm-dropout"):]
    assert "Added within ABI 22" in block
    # the header states the variance method and the determinism
    assert "never E[a^2] - E[a]^2" in block and "Chan" in block and "no atomics" in block


def test_slab_rows_and_workspace_bytes():
    lib = _lib.load()
    S = lib.ngnn_bn_slab_rows()
    assert S > 0
    # one (mean, M2) pair of doubles per slab and column
    assert lib.ngnn_bn_workspace_bytes(S, 8) == 2 * 8 * 8
    assert lib.ngnn_bn_workspace_bytes(S + 1, 8) == 2 * 2 * 8 * 8
    assert lib.ngnn_bn_workspace_bytes(3 * S + 5, 100) == 4 * 2 * 100 * 8
    assert lib.ngnn_bn_workspace_bytes(0, 8) == 0 and lib.ngnn_bn_workspace_bytes(8, 0) == 0


def _train(lib, **kw):
    a = dict(x=P, ldx=37, n=777, F=37, relu=1, gamma=P, beta=P, eps=1e-5, momentum=0.1, rm=P, rv=P, nbt=P,
             p=0.5, seed=1, seed_dev=None, out=P, ldo=37, mean=P, mean_lo=P, invstd=P, ws=P, ws_bytes=1 << 20)
    a.update(kw)
    return lib.ngnn_bn_fwd_train(a["x"], a["ldx"], a["n"], a["F"], a["relu"], a["gamma"], a["beta"], a["eps"],
                                 a["momentum"], a["rm"], a["rv"], a["nbt"], a["p"], a["seed"], a["seed_dev"],
                                 a["out"], a["ldo"], a["mean"], a["mean_lo"], a["invstd"], a["ws"],
                                 a["ws_bytes"], None)


def _eval(lib, **kw):
    a = dict(x=P, ldx=37, n=777, F=37, relu=1, gamma=P, beta=P, eps=1e-5, rm=P, rv=P, out=P, ldo=37)
    a.update(kw)
    return lib.ngnn_bn_fwd_eval(a["x"], a["ldx"], a["n"], a["F"], a["relu"], a["gamma"], a["beta"], a["eps"],
                                a["rm"], a["rv"], a["out"], a["ldo"], None)


def _bwd(lib, **kw):
    a = dict(dout=P, ldg=37, x=P, ldx=37, n=777, F=37, relu=1, gamma=P, mean=P, mean_lo=P, invstd=P, p=0.5, seed=1,
             seed_dev=None, dgamma=P, dbeta=P, dx=P, ldd=37, ws=P, ws_bytes=1 << 20)
    a.update(kw)
    return lib.ngnn_bn_bwd(a["dout"], a["ldg"], a["x"], a["ldx"], a["n"], a["F"], a["relu"], a["gamma"], a["mean"],
                           a["mean_lo"], a["invstd"], a["p"], a["seed"], a["seed_dev"], a["dgamma"], a["dbeta"], a["dx"],
                           a["ldd"], a["ws"], a["ws_bytes"], None)


def test_train_argument_errors_return_before_launch():
    lib = _lib.load()
    for n in (0, 1, -1):  # no batch statistics of fewer than two rows
        assert _train(lib, n=n) == _lib.E_ARG, n
    for F in (0, -3):
        assert _train(lib, F=F) == _lib.E_ARG, F
    for name in ("x", "gamma", "beta", "rm", "rv", "nbt", "out", "mean", "mean_lo", "invstd"):
        assert _train(lib, **{name: None}) == _lib.E_ARG, name
    assert _train(lib, p=-0.1) == _lib.E_ARG and _train(lib, p=1.5) == _lib.E_ARG
    assert _train(lib, p=float("nan")) == _lib.E_ARG
    assert _train(lib, eps=-1.0) == _lib.E_ARG and _train(lib, momentum=1.5) == _lib.E_ARG
    assert _train(lib, ldx=36) == _lib.E_SHAPE and _train(lib, ldo=36) == _lib.E_SHAPE
    assert _train(lib, n=(1 << 31) - 1) == _lib.E_RANGE
    assert _train(lib, F=(1 << 20) + 1, ldx=1 << 21, ldo=1 << 21) == _lib.E_RANGE
    need = lib.ngnn_bn_workspace_bytes(777, 37)
    assert _train(lib, ws=None) == _lib.E_WORKSPACE
    assert _train(lib, ws_bytes=need - 1) == _lib.E_WORKSPACE
    assert _train(lib, ws=P + 4) == _lib.E_WORKSPACE  # misaligned for the fp64 partials


def test_eval_argument_errors_return_before_launch():
    lib = _lib.load()
    assert _eval(lib, n=-1) == _lib.E_ARG and _eval(lib, F=0) == _lib.E_ARG
    for name in ("x", "gamma", "beta", "rm", "rv", "out"):
        assert _eval(lib, **{name: None}) == _lib.E_ARG, name
    assert _eval(lib, ldx=36) == _lib.E_SHAPE and _eval(lib, ldo=36) == _lib.E_SHAPE
    assert _eval(lib, n=(1 << 31) - 1) == _lib.E_RANGE
    assert _eval(lib, n=0, x=None, out=None) == _lib.OK  # no row: success, nothing read


def test_bwd_argument_errors_return_before_launch():
    lib = _lib.load()
    for n in (0, 1, -1):
        assert _bwd(lib, n=n) == _lib.E_ARG, n
    assert _bwd(lib, F=0) == _lib.E_ARG
    for name in ("dout", "x", "gamma", "mean", "mean_lo", "invstd", "dgamma", "dbeta"):
        assert _bwd(lib, **{name: None}) == _lib.E_ARG, name
    assert _bwd(lib, p=2.0) == _lib.E_ARG
    for name in ("ldg", "ldx", "ldd"):
        assert _bwd(lib, **{name: 36}) == _lib.E_SHAPE, name
    assert _bwd(lib, ws_bytes=8) == _lib.E_WORKSPACE and _bwd(lib, ws=None) == _lib.E_WORKSPACE
    # dx == NULL is the skipped second pass, not an error: its stride is not looked at
    assert _bwd(lib, dx=None, ldd=0, ws=None) == _lib.E_WORKSPACE


def test_every_argument_error_has_a_message():
    lib = _lib.load()
    for rc in ARG_ERRORS:
        msg = lib.ngnn_strerror(rc).decode()
        assert msg.startswith("ngnn: ") and "unknown" not in msg, (rc, msg)


def test_python_op_exists_with_the_stated_signature():
    assert ngnn.batch_norm_act is ops.batch_norm_act and "batch_norm_act" in ngnn.__all__
    sig = inspect.signature(ops.batch_norm_act)
    assert list(sig.parameters) == ["x", "bn", "relu", "p", "training", "seed", "seed_dev"]
    assert [q.default for q in sig.parameters.values()][2:] == [False, 0.0, None, None, None]


def test_unsupported_inputs_take_torchs_ops_unchanged():
    torch.manual_seed(0)
    x = torch.randn(9, 4) - 0.2
    bn, ref = nn.BatchNorm1d(4), nn.BatchNorm1d(4)
    assert not ops.batch_norm_act_supported(x, bn, True)  # a CPU tensor
    out = ops.batch_norm_act(x, bn, relu=True)
    assert torch.equal(out, ref(x.relu()))
    assert torch.equal(bn.running_var, ref.running_var) and int(bn.num_batches_tracked) == 1
    bn.eval(), ref.eval()
    assert torch.equal(ops.batch_norm_act(x, bn, relu=True, p=0.5), ref(x.relu()))  # eval: no dropout
    # models keep their state-dict keys
    keys = sorted(k for k in ngnn.SAGE(4, 8, 3, 2, use_bn=True).state_dict() if k.startswith("bn"))
    assert keys == sorted(f"bn{i}.{k}" for i in (1, 2) for k in
                          ("weight", "bias", "running_mean", "running_var", "num_batches_tracked"))
