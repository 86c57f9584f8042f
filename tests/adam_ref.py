"""One Adam step restated in float64 (torch.optim.Adam's documented rule,
amsgrad and maximize off) -- the reference the optimizer kernels are measured
against.  Plain torch on the CPU.

The hyper-parameters are rounded to fp32 first: the C ABI takes ``float``, so
0.999f (not 0.999) is the contract.  Everything after that is float64.
"""
import torch


def f32(x) -> float:
    """x as the fp32 value the ABI receives, held in a Python float."""
    return float(torch.tensor(float(x), dtype=torch.float32))


def adam_step(p, g, m, v, t, lr, betas, eps, weight_decay):
    """(p', m', v') of step number t (1 for the first) from float64 p, g, m, v."""
    assert all(x.dtype == torch.float64 for x in (p, g, m, v)) and int(t) >= 1
    lr, b1, b2, eps, wd = f32(lr), f32(betas[0]), f32(betas[1]), f32(eps), f32(weight_decay)
    if wd != 0.0:
        g = g + wd * p
    m = b1 * m + (1.0 - b1) * g
    v = b2 * v + (1.0 - b2) * g * g
    m_hat = m / (1.0 - b1 ** int(t))
    v_hat = v / (1.0 - b2 ** int(t))
    return p - lr * m_hat / (v_hat.sqrt() + eps), m, v


def adam_step_bf16(p_bf16, g_bf16, m, v, t, lr, betas, eps, weight_decay):
    """The same step for a bf16 parameter and gradient (widened exactly);
    float64 moments.  p' is returned in float64, BEFORE its rounding to bf16."""
    assert p_bf16.dtype == torch.bfloat16 and g_bf16.dtype == torch.bfloat16
    return adam_step(p_bf16.double(), g_bf16.double(), m, v, t, lr, betas, eps, weight_decay)
