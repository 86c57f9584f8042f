"""Generate tests/golden/codi_*.npz and tests/golden/bc_*.npz.

Run where the reference checkout is present:

    python tests/golden/make_golden_noisy_losses.py --ref <reference checkout>

As make_golden_rewire.py: the reference's OWN ``src/utils/losses.py`` is
imported from the read-only checkout, and its ``CoDiLoss(device, co_lambda)``
and ``backward_correction(output, labels, C, nbr_class, device)`` are run on
the CPU in float32.  Only tensors are written: the inputs, the outputs and
both input gradients.  For CoDi the kept sets are read off the gradients
(the reference returns zeros for them): the nonzero rows of grad_y1 are
``ind_2_update``, those of grad_y2 ``ind_1_update``.

Asserted here, so that a test against these files cannot hinge on rounding:
CoDi -- the key gap at the selection boundary of both models is >= 1e-3;
backward correction -- no softmax value lies within a relative 1e-3 of
either clamp threshold, and at least one lies below 1e-5 (the clamp is
exercised).
"""
from __future__ import annotations

import argparse
import importlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import losses_noisy_ref as R  # noqa: E402

# name -> (B, C, forget_rate, seed, co_lambda)
CODI_CASES = {
    "codi_b300": (300, 47, 0.2, 2000, 0.1),
    "codi_b1024": (1024, 40, 0.45, 2001, 0.1),
}
# name -> (B, C, logit scale, seed, matrix)
BC_CASES = {
    "bc_b300": (300, 47, 2.0, 2100, "uniform"),
    "bc_b65": (65, 7, 8.0, 2101, "pair"),
}


def codi_case(mod, name, B, C, forget, seed, lam):
    g = torch.Generator().manual_seed(seed)
    y1 = (2 * torch.randn(B, C, generator=g)).requires_grad_(True)
    y2 = (2 * torch.randn(B, C, generator=g)).requires_grad_(True)
    yn = torch.randint(0, C, (B,), generator=g)
    ind = torch.randperm(3 * B, generator=g)[:B]
    clean = torch.rand(3 * B, generator=g) < 0.6
    nr = int((1 - forget) * B)
    k1, k2, _ = R.codi_keys(y1.detach().double(), y2.detach().double(), yn, lam)
    gaps = (R.key_gap(k1, nr), R.key_gap(k2, nr))
    assert min(gaps) >= 1e-3, f"{name}: boundary key gaps {gaps}"
    out = mod.CoDiLoss("cpu", co_lambda=lam)(y1, y2, yn, forget, ind, clean)
    out[0].backward()
    out[1].backward()
    keep2 = torch.nonzero(y1.grad.abs().sum(1) > 0).flatten()
    keep1 = torch.nonzero(y2.grad.abs().sum(1) > 0).flatten()
    assert keep1.numel() == nr and keep2.numel() == nr
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(
        path, y1=y1.detach().numpy(), y2=y2.detach().numpy(), y_noise=yn.numpy(), ind=ind.numpy(),
        noise_or_not=clean.numpy(), forget_rate=np.array(forget, dtype=np.float64),
        co_lambda=np.array(lam, dtype=np.float64), loss_1=out[0].detach().numpy(),
        loss_2=out[1].detach().numpy(), pure_ratio_1=np.asarray(out[2], dtype=np.float32),
        pure_ratio_2=np.asarray(out[3], dtype=np.float32), ind_1_update=keep1.numpy(),
        ind_2_update=keep2.numpy(), grad_y1=y1.grad.numpy(), grad_y2=y2.grad.numpy(),
        **{"meta/seed": np.array(seed)})
    print(f"{name}: {os.path.getsize(path) / 1024:.1f} KiB, kept {nr} of {B}, key gaps {gaps[0]:.2e} {gaps[1]:.2e}")


def bc_case(mod, name, B, C, scale, seed, kind):
    g = torch.Generator().manual_seed(seed)
    x = (scale * torch.randn(B, C, generator=g)).requires_grad_(True)
    y = torch.randint(0, C, (B,), generator=g)
    mat = R.uniform_flip_matrix(C, 0.3) if kind == "uniform" else R.pair_flip_matrix(C, 0.3)
    low, high, near = R.clamp_stats(x.detach())
    assert near >= 1e-3, f"{name}: a softmax value within {near:.2e} (relative) of a clamp threshold"
    assert low >= 1, f"{name}: the clamp is not exercised"
    # float32 resolves p near 1 to 6e-8 only: keep four of its ulps off the high threshold
    p = torch.softmax(x.detach().double(), dim=1)
    assert float((p - R.CLAMP_HI).abs().min()) >= 2.4e-7, f"{name}: a float32 softmax value could cross 1 - 1e-5"
    loss = mod.backward_correction(x, y, mat, C, "cpu")
    loss.backward()
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, output=x.detach().numpy(), labels=y.numpy(), C=mat,
                        loss=loss.detach().numpy(), grad_output=x.grad.numpy(),
                        **{"meta/seed": np.array(seed)})
    print(f"{name}: {os.path.getsize(path) / 1024:.1f} KiB, {low} low and {high} high clamped, nearest {near:.2e}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="the reference checkout (read only)")
    args = ap.parse_args()
    if args.ref not in sys.path:
        sys.path.insert(0, args.ref)
    mod = importlib.import_module("src.utils.losses")
    for name, case in CODI_CASES.items():
        codi_case(mod, name, *case)
    for name, case in BC_CASES.items():
        bc_case(mod, name, *case)


if __name__ == "__main__":
    main()
