"""Torch restatements of the reference's two noisy-label losses (TEST
INFRASTRUCTURE: the product path is ngnn.losses.backward_correction /
ngnn.losses.CoDiLoss on the device).  Dtype-generic: run on float64 inputs
they are the yardstick of the GPU tests; run on float32 they reproduce the
reference (tests/golden/bc_*.npz, codi_*.npz, made by
tests/golden/make_golden_noisy_losses.py from the reference's own module).

``backward_correction`` follows src/utils/losses.py:51-70: the correction
matrix inverted in its own precision and rounded to float32 (:62), a one-hot
of the labels (:64-66), softmax and clamp to [1e-5, 1 - 1e-5] (:67-69), and
``-mean(onehot @ Cinv * log(clamped))`` (:70).

``codi_loss`` follows CoDiLoss.forward (:106-137): js_loss_compute's per-row
value (:92-104: kl_div of both log-softmaxes against the mean of the two
softmaxes, halved -- KL(mean || .), not the textbook JS), detached; the keys
``CE - co_lambda * js`` (:110, :115); their ascending argsort (np.argsort
leaves ties unspecified: here by row index, a stable sort, as the device);
num_remember = int((1 - forget_rate) * B), and ALL rows when that is 0
(:125-128); the pure ratios (:130-131) and the exchange on the plain cross
entropy (:133-134).  Extensions the device op has: ``ignore_index`` rows
count 0 in the key and are left out of the means (F.cross_entropy's rule),
and ``sel`` overrides the kept sets (for boundary near ties).
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

CLAMP_LO, CLAMP_HI = 1e-5, 1.0 - 1e-5


def correction_inverse(C) -> torch.Tensor:
    """losses.py:62: np.linalg.inv(C).astype(np.float32), as a tensor."""
    C = C.detach().cpu().numpy() if torch.is_tensor(C) else np.asarray(C)
    return torch.from_numpy(np.linalg.inv(C).astype(np.float32))


def backward_correction(output, labels, C, nbr_class):
    c_inv = correction_inverse(C).to(output.dtype)
    label_oh = torch.zeros(len(labels), nbr_class, dtype=output.dtype)
    label_oh.scatter_(1, labels.view(-1, 1), 1)
    p = torch.softmax(output, dim=1)
    p = torch.clamp(p, min=CLAMP_LO, max=CLAMP_HI)
    return -torch.mean(torch.matmul(label_oh, c_inv) * torch.log(p))


def js_rows(y_1, y_2):
    """js_loss_compute(y_1, y_2, reduce=False)."""
    lp, lq = F.log_softmax(y_1, dim=1), F.log_softmax(y_2, dim=1)
    mean = (lp.exp() + lq.exp()) / 2
    kl_1 = torch.xlogy(mean, mean) - mean * lp  # F.kl_div(lp, mean, reduction='none')
    kl_2 = torch.xlogy(mean, mean) - mean * lq
    return ((kl_1 + kl_2) / 2).sum(1)


def codi_keys(y_1, y_2, y_noise, co_lambda, ignore_index=-100):
    """(key_1, key_2, js): what each model's rows are ranked by."""
    js = js_rows(y_1, y_2).detach()
    ce_1 = F.cross_entropy(y_1, y_noise, reduction="none", ignore_index=ignore_index).detach()
    ce_2 = F.cross_entropy(y_2, y_noise, reduction="none", ignore_index=ignore_index).detach()
    return ce_1 - co_lambda * js, ce_2 - co_lambda * js, js


def codi_loss(y_1, y_2, y_noise, forget_rate, ind, noise_or_not, co_lambda=0.1, ignore_index=-100, sel=None):
    """Returns (loss_1, loss_2, pure_ratio_1, pure_ratio_2, ind_1_update,
    ind_2_update, ind_noisy_1, ind_noisy_2); sel = (kept_1, kept_2) replaces
    the sorted selections (then the last two are None)."""
    key_1, key_2, _ = codi_keys(y_1, y_2, y_noise, co_lambda, ignore_index)
    B = len(key_1)
    num_remember = int((1 - forget_rate) * B)
    if num_remember == 0:
        num_remember = B
    if sel is None:
        s1 = torch.sort(key_1, stable=True).indices
        s2 = torch.sort(key_2, stable=True).indices
        k1, k2, n1, n2 = s1[:num_remember], s2[:num_remember], s1[num_remember:], s2[num_remember:]
    else:
        k1, k2, n1, n2 = sel[0], sel[1], None, None
    if noise_or_not is None:
        pr1 = pr2 = torch.tensor(float("nan"))
    else:
        ind = torch.arange(B) if ind is None else ind
        pr1 = torch.sum(noise_or_not[ind[k1]]) / float(num_remember)
        pr2 = torch.sum(noise_or_not[ind[k2]]) / float(num_remember)
    loss_1 = F.cross_entropy(y_1[k2], y_noise[k2], ignore_index=ignore_index)
    loss_2 = F.cross_entropy(y_2[k1], y_noise[k1], ignore_index=ignore_index)
    return loss_1, loss_2, pr1, pr2, k1, k2, n1, n2


# ---- inputs shared by the generator and the tests

def uniform_flip_matrix(nc: int, rate: float) -> np.ndarray:
    """Every label kept with 1 - rate, flipped evenly to the others."""
    m = np.full((nc, nc), rate / (nc - 1), dtype=np.float64)
    np.fill_diagonal(m, 1.0 - rate)
    return m


def pair_flip_matrix(nc: int, rate: float) -> np.ndarray:
    """Label c kept with 1 - rate, flipped to c + 1 (mod nc): not symmetric,
    and neither is its inverse."""
    m = np.eye(nc, dtype=np.float64) * (1.0 - rate)
    for c in range(nc):
        m[c, (c + 1) % nc] += rate
    return m


def logits(B, C, scale, seed, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    return (scale * torch.randn(B, C, generator=g)).to(dtype)


def bc_logits(B, C, scale, seed, dtype=torch.float32):
    """Logits (rounded to `dtype`, returned in it) none of whose softmax values
    a float32 evaluation could put on the other side of a clamp threshold
    (there the gradient jumps by the entry's whole weight): rows that are not
    admissible (bc_admissible_rows) are drawn again, from the same generator."""
    g = torch.Generator().manual_seed(seed)
    x = (scale * torch.randn(B, C, generator=g)).to(dtype)
    for _ in range(200):
        bad = torch.nonzero(~bc_admissible_rows(x.float())).flatten()
        if bad.numel() == 0:
            return x
        x[bad] = (scale * torch.randn(bad.numel(), C, generator=g)).to(dtype)
    raise AssertionError("no admissible logits")


def bc_admissible_rows(x):
    """Per row: every softmax value (float64) a relative 1e-3 off both clamp
    thresholds, in the threshold's own scale (clamp_stats), and four float32
    ulps of 1 off the high one."""
    p = torch.softmax(x.double(), dim=1)
    d = torch.minimum((p - CLAMP_LO).abs(), (p - CLAMP_HI).abs()).min(1).values
    return (d >= 1e-3 * CLAMP_LO) & ((p - CLAMP_HI).abs().min(1).values >= 2.4e-7)


def key_gap(key, num_remember) -> float:
    """The gap between the last kept and the first forgotten key."""
    s = torch.sort(key.double(), stable=True).values
    if num_remember <= 0 or num_remember >= len(s):
        return float("inf")
    return float(s[num_remember] - s[num_remember - 1])


def clamp_stats(output):
    """(#p below the low threshold, #p above the high one, the smallest
    relative distance of any p to either threshold), in float64.  Relative
    to the threshold's own scale: |p - 1e-5| / 1e-5 at the low one and
    |(1 - p) - 1e-5| / 1e-5 at the high one (which sits 1e-5 below 1)."""
    p = torch.softmax(output.double(), dim=1)
    rel = torch.minimum((p - CLAMP_LO).abs(), (p - CLAMP_HI).abs()) / CLAMP_LO
    return int((p < CLAMP_LO).sum()), int((p > CLAMP_HI).sum()), float(rel.min())
