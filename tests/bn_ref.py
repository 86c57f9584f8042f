"""Host restatements for the fused ReLU-BatchNorm-dropout op (TEST
INFRASTRUCTURE: only tests import it; the product path is
ngnn.ops.batch_norm_act on the device).

* ``dropout_keep`` / ``dropout_thresh`` / ``dropout_scale``: the replica of
  ``ngnn_device.h::Dropout`` (restated from tests/test_gpu_fused.py).
* ``forward`` / ``backward``: the formulas of include/ngnn.h in float64.
* ``probe_input``: the column classes the tolerance rule is pinned on, and
  ``column_bar``: that rule.
"""
import math

import numpy as np
import torch

M32 = np.uint64(0xFFFFFFFF)


def _lowbias32(x):
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7FEB352D)) & M32
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846CA68B)) & M32
    return x ^ (x >> np.uint64(16))


def dropout_thresh(p):
    pf = float(np.float32(p))
    if pf <= 0:
        return 0
    return max(1, min(256, math.ceil(pf * 256.0)))


def dropout_scale(p):
    """Survivor scale 256 / (256 - thresh), thresh = ceil(p * 256), in fp32."""
    t = dropout_thresh(p)
    return 0.0 if t >= 256 else float(np.float32(256.0) / np.float32(256 - t))


def dropout_keep(seed, n_rows, n_cols, p):
    """Byte mode (thresh != 128): one hash per column quad, keep <=> byte
    (col % 4) >= thresh.  Bit mode (p = 0.5): keep <=> bit c & 31 of the hash
    of word c >> 5.  thresh == 0 keeps everything."""
    thresh = dropout_thresh(p)
    if thresh == 0:
        return torch.ones(n_rows, n_cols, dtype=torch.bool)
    u = np.uint64
    s0, s1 = u(seed & 0xFFFFFFFF), u((seed >> 32) & 0xFFFFFFFF)
    r = np.arange(n_rows, dtype=np.uint64)[:, None]
    c = np.arange(n_cols, dtype=np.uint64)[None, :]
    rk = _lowbias32(r ^ s0) ^ s1
    if thresh == 128:
        h = _lowbias32((rk + (c >> u(5))) & M32)
        return torch.from_numpy(((h >> (c & u(31))) & u(1)) == u(1))
    h = _lowbias32((rk + (c >> u(2))) & M32)
    byte = (h >> (u(8) * (c & u(3)))) & u(0xFF)
    return torch.from_numpy(byte >= u(thresh))


def forward(x, gamma, beta, eps=1e-5, relu=False, keep=None, scale=1.0):
    """float64: ``(out, mean, invstd, unbiased_var)`` of
    out = keep * scale * (gamma * (a - mean) * invstd + beta)."""
    x, gamma, beta = x.double(), gamma.double(), beta.double()
    a = torch.relu(x) if relu else x
    n = a.size(0)
    mean = a.mean(0)
    m2 = (a - mean).square().sum(0)
    invstd = 1.0 / torch.sqrt(m2 / n + eps)
    y = gamma * (a - mean) * invstd + beta
    if keep is not None:
        y = torch.where(keep, y * scale, torch.zeros_like(y))
    return y, mean, invstd, m2 / (n - 1)


def backward(dout, x, gamma, eps=1e-5, relu=False, keep=None, scale=1.0):
    """float64 ``(dx, dgamma, dbeta)`` of ``forward``."""
    dout, x, gamma = dout.double(), x.double(), gamma.double()
    a = torch.relu(x) if relu else x
    n = a.size(0)
    mean = a.mean(0)
    invstd = 1.0 / torch.sqrt((a - mean).square().sum(0) / n + eps)
    xhat = (a - mean) * invstd
    g = dout if keep is None else torch.where(keep, dout * scale, torch.zeros_like(dout))
    dbeta = g.sum(0)
    dgamma = (g * xhat).sum(0)
    dx = gamma * invstd * (g - dbeta / n - xhat * dgamma / n)
    if relu:
        dx = torch.where(x > 0, dx, torch.zeros_like(dx))
    return dx, dgamma, dbeta


# the probe's column classes: cancellation between the mean and the values
# decides the error of (i)-(iii); (iv) has variance 0 after the ReLU
HARD = {"i": 0, "ii": 1, "iii": 2}
ALL_NEG = 3


def probe_input(n, f, seed=0):
    """fp32 [n, f]: plain randn, with (f >= 5) column 0 = randn + 4096, column
    1 = randn * 1e-3 + 100, column 2 = 2.5, column 3 all negative.  Returns
    ``(x, hard, plain)``: the indices of classes (i)-(iii) and of the plain
    columns."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, f, generator=g)
    if f < 5:
        return x, [], list(range(f))
    x[:, 0] += 4096.0
    x[:, 1] = x[:, 1] * 1e-3 + 100.0
    x[:, 2] = 2.5
    x[:, 3] = -x[:, 3].abs() - 0.5
    return x, [0, 1, 2], list(range(4, f))


def col_err(got, want):
    """Per-column max |got - want| in float64 (a vector stays a vector)."""
    e = (got.detach().double().cpu() - want.detach().double().cpu()).abs()
    return e if e.dim() == 1 else e.amax(0)


def column_bar(e_torch):
    """Classes (i)-(iii): max(1e-5, 2 * e_torch) per column, e_torch the error
    of torch's own fp32 CPU BatchNorm on the same input."""
    return torch.clamp(2.0 * e_torch, min=1e-5)
