"""Generate tests/golden/contrast_*.npz.

Run where the reference checkout is present:

    python tests/golden/make_golden_contrast.py --ref <reference checkout>

As make_golden_noisy_losses.py: the reference's OWN ``src/utils/data_utils.py``
is imported from the read-only checkout, and its ``Discriminator_innerprod()``
and ``BCEExeprtLoss(nbr_nodes)`` are run on the CPU in float32 on the rows
``idx`` of three activation matrices, as pipeline_test.py:150-158 does.  Only
tensors are written: the inputs, ``idx``, the loss and the three input
gradients.

The inputs are ``relu(0.25 * randn)``, which keeps the logits below about 8.
Asserted here, so that a test against these files cannot hinge on the
reference's own rounding: each float32 gradient lies within 5e-6 of its
float64 counterpart's max (half the project's gradient bar).
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

import contrast_ref as R  # noqa: E402

# name -> (N, H, M or None for every row permuted, seed)
CASES = {
    "contrast_n128_h130": (128, 130, 41, 3000),
    "contrast_n64_h512": (64, 512, None, 3001),
}
REF_REL = 5e-6


def case(mod, name, N, H, M, seed):
    h, hp, hn = (t.requires_grad_(True) for t in R.relu_inputs(N, H, seed))
    g = torch.Generator().manual_seed(seed + 500)
    idx = torch.randperm(N, generator=g)[:N if M is None else M]
    logits_pa, logits_n = mod.Discriminator_innerprod()(h[idx], hp[idx], hn[idx])
    loss = mod.BCEExeprtLoss(N)(logits_pa, logits_n)
    loss.backward()
    want = R.contrast_ref_f64(h, hp, hn, idx)
    worst = 0.0
    for got, ref in zip((h.grad, hp.grad, hn.grad), want[1:]):
        ratio = float((got.double() - ref).abs().max() / ref.abs().max())
        worst = max(worst, ratio)
        assert ratio <= REF_REL, f"{name}: the reference's float32 gradient is {ratio:.2e} of max off float64"
    top = float(torch.cat([logits_pa, logits_n]).detach().abs().max())
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, h=h.detach().numpy(), hp=hp.detach().numpy(), hn=hn.detach().numpy(),
                        idx=idx.numpy(), loss=loss.detach().numpy(), grad_h=h.grad.numpy(),
                        grad_hp=hp.grad.numpy(), grad_hn=hn.grad.numpy(), **{"meta/seed": np.array(seed)})
    print(f"{name}: {os.path.getsize(path) / 1024:.1f} KiB, M {idx.numel()}, max |logit| {top:.2f}, "
          f"float32 gradients within {worst:.2e} of float64")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="the reference checkout (read only)")
    args = ap.parse_args()
    if args.ref not in sys.path:
        sys.path.insert(0, args.ref)
    mod = importlib.import_module("src.utils.data_utils")
    for name, c in CASES.items():
        case(mod, name, *c)


if __name__ == "__main__":
    main()
