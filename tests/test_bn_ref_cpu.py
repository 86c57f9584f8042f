"""The float64 reference of the fused ReLU-BatchNorm-dropout op against
``nn.BatchNorm1d`` in float64, and the tolerance rule of the hard columns.

On the probe input (tests/bn_ref.py::probe_input, N = 777, F = 37) the error
of columns (i) randn + 4096, (ii) randn * 1e-3 + 100 and (iii) the constant
2.5 is decided by cancellation between the mean and the values, not by the
kernel: fp32 holds 4096.x to 2.4e-4, so no fp32 mean can do better.  The
rule for those columns is therefore relative to torch's own fp32 CPU
BatchNorm on the same input,

    per-column error against float64  <=  max(1e-5, 2 * e_torch),

and this file pins that the rule tells right from wrong: the chunked Chan
merge the kernels run (eight-row chunks, 256-row slabs, float64 registers,
rounded once) and a float64 two-pass sum meet it, and E[a^2] - E[a]^2 in fp32
misses it by orders of magnitude (class (i): 0.97 against a bar of 1.4e-4).
On the plain columns torch's own error (5e-7) stays below the project's 1e-5
output bar.

torch's CPU BatchNorm accumulates fp32 inputs in float64, so its mean and
invstd are the correctly rounded ones; fp32-register restatements of a
two-pass sum and of a 64-row-slab Chan merge measured here reach it on
classes (i) and (iii) but not on class (ii) (out error 7.3e-3 and 3.4e-3
against a bar of 5.5e-4: a column mean of 100 summed in fp32 is off by
several ulps, and invstd = 1000 multiplies that).  That is why the kernels
carry the statistics in float64; the fp32 forms are not asserted either way.
"""
import numpy as np
import pytest
import torch
import torch.nn as nn

import bn_ref

N, F, EPS = 777, 37, 1e-5
f32 = np.float32


def _params(f, seed=1):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(f, generator=g) + 0.5, torch.randn(f, generator=g)


def _torch_bn(x, gamma, beta, dtype, relu):
    """(out, save_mean, save_invstd) of torch's CPU batch norm in `dtype`."""
    a = torch.relu(x.to(dtype)) if relu else x.to(dtype)
    return torch.native_batch_norm(a, gamma.to(dtype), beta.to(dtype), None, None, True, 0.1, EPS)


@pytest.mark.parametrize("relu", [False, True])
def test_reference_forward_and_backward_match_float64_batchnorm(relu):
    x, _, _ = bn_ref.probe_input(N, F)
    gamma, beta = _params(F)
    bn = nn.BatchNorm1d(F, eps=EPS).double()
    with torch.no_grad():
        bn.weight.copy_(gamma)
        bn.bias.copy_(beta)
    xd = x.double().requires_grad_(True)
    out = bn(torch.relu(xd) if relu else xd)
    dout = torch.randn(N, F, generator=torch.Generator().manual_seed(2)).double()
    out.backward(dout)
    y, mean, invstd, uvar = bn_ref.forward(x, gamma, beta, EPS, relu)
    torch.testing.assert_close(y, out.detach(), rtol=1e-11, atol=1e-9)  # (4096-sized cancellation in fp64)
    torch.testing.assert_close(0.1 * mean, bn.running_mean, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(0.9 + 0.1 * uvar, bn.running_var, rtol=1e-12, atol=1e-12)
    dx, dgamma, dbeta = bn_ref.backward(dout, x, gamma, EPS, relu)
    torch.testing.assert_close(dx, xd.grad, rtol=1e-9, atol=1e-9)
    torch.testing.assert_close(dgamma, bn.weight.grad, rtol=1e-9, atol=1e-8)
    torch.testing.assert_close(dbeta, bn.bias.grad, rtol=1e-12, atol=1e-12)
    if relu:  # class (iv): all zero after the ReLU, variance 0, the output is beta
        assert torch.equal(y[:, bn_ref.ALL_NEG], beta.double()[bn_ref.ALL_NEG].expand(N))


def test_dropout_replica_rates_and_modes():
    for p in (0.5, 0.25, 0.9):
        keep = bn_ref.dropout_keep(0x1234_5678_9ABC, 512, 100, p)
        want = 1.0 - bn_ref.dropout_thresh(p) / 256.0
        assert abs(float(keep.float().mean()) - want) < 0.01, p
    assert bn_ref.dropout_keep(7, 4, 9, 0.0).all() and not bn_ref.dropout_keep(7, 4, 9, 1.0).any()
    assert bn_ref.dropout_scale(0.5) == 2.0 and bn_ref.dropout_scale(1.0) == 0.0


# ---- fp32 restatements of three ways to take the column statistics ----

def _seq_sum(a):
    return np.cumsum(a, axis=0, dtype=a.dtype)[-1]


def _two_pass(a):
    n = a.dtype.type(a.shape[0])
    mean = _seq_sum(a) / n
    return mean, _seq_sum((a - mean) ** 2) / n


def _chan(a, slab, chunk=None):
    """(mean, biased var): per-slab two-pass statistics (per `chunk` rows
    first when given) merged by Chan's formula in ascending order, in a's dtype."""
    t = a.dtype.type
    n, mean, m2 = t(0), np.zeros(a.shape[1], a.dtype), np.zeros(a.shape[1], a.dtype)
    for s in range(0, a.shape[0], slab):
        blk = a[s:s + slab]
        if chunk:
            mb, vb = _chan(blk, chunk)
        else:
            mb, vb = _two_pass(blk)
        nb = t(blk.shape[0])
        d = mb - mean
        w = nb / (n + nb)
        mean = mean + d * w
        m2 = m2 + vb * nb + d * d * (n * w)
        n += nb
    return mean, m2 / n


def _sum_of_squares(a):
    n = a.dtype.type(a.shape[0])
    mean = _seq_sum(a) / n
    return mean, _seq_sum(a * a) / n - mean * mean


def _apply_f32(a, mean, var, gamma, beta):
    mean, var = mean.astype(f32), var.astype(np.float64)
    invstd = (1.0 / np.sqrt(var + EPS)).astype(f32)
    return ((a - mean) * invstd) * gamma + beta, mean, invstd


def test_tolerance_rule_on_the_probe_columns():
    x, hard, plain = bn_ref.probe_input(N, F)
    gamma, beta = _params(F)
    want = bn_ref.forward(x, gamma, beta, EPS)[:3]
    e_torch = [bn_ref.col_err(g, w) for g, w in zip(_torch_bn(x, gamma, beta, torch.float32, False), want)]
    # torch's own fp32 error on the plain columns is inside the project's bar
    assert float(e_torch[0][plain].max()) < 1e-5
    a = x.numpy()
    ga, be = gamma.numpy(), beta.numpy()

    def errs(stats):
        got = _apply_f32(a, *stats, ga, be)
        return [bn_ref.col_err(torch.from_numpy(np.asarray(g, np.float64)), w) for g, w in zip(got, want)]

    # clip: the sum-of-squares variance of the constant column can come out
    # negative, which no kernel would pass to a square root
    clip = lambda s: (s[0], np.maximum(s[1], 0))  # noqa: E731
    a64 = a.astype(np.float64)
    good = {"kernel order fp64": _chan(a64, 256, 8), "two-pass fp64": _two_pass(a64)}
    for name, stats in good.items():
        for what, e, et in zip(("out", "mean", "invstd"), errs(stats), e_torch):
            bar = bn_ref.column_bar(et)
            assert bool((e[hard] <= bar[hard]).all()), (name, what, e[hard].tolist(), bar[hard].tolist())
    e_bad = errs(clip(_sum_of_squares(a)))[0]
    bar = bn_ref.column_bar(e_torch[0])
    assert float(e_bad[0]) > 1e3 * float(bar[0])    # class (i): off by orders of magnitude
    assert float(e_bad[1]) > 10 * float(bar[1])     # class (ii)
    # the constant column: every accepted method returns beta exactly
    for stats in good.values():
        out = _apply_f32(a, *stats, ga, be)[0]
        assert np.array_equal(out[:, 2], np.full(N, be[2], f32))
