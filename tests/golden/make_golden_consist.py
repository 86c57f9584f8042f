"""Generate tests/golden/consist_b300.npz and tests/golden/consist_b65.npz.

Run where the reference checkout is present:

    python tests/golden/make_golden_consist.py --ref <reference checkout>

As make_golden_noisy_losses.py: the reference's OWN ``src/utils/losses.py``
is imported from the read-only checkout, and its ``get_uncertainty_batch``
and ``fix_cr`` are run on the CPU in float32.  Only tensors are written: the
inputs, ``w``, and for hard / soft / l2 the loss and both input gradients
(rows < B; a gradient autograd leaves None is stored as zeros), plus the
hard and soft losses with ``w=None`` and with ``p_cutoff=0``.

Each graph has its edges in random order (neither row sorted), source 0 (a
row < B) with >= 200 out-edges, one exact duplicate edge, one self-loop, and
source 1 (a row < B) without out-edges.

Asserted here, so that no test hinges on rounding (the seed is walked upward
from the recorded base until all hold, and the seed used is stored): on rows
< B the top two of exp(y_pure) differ by >= 1e-3 relative; no row's maximum
lies within 1e-3 relative of p_cutoff; at least one row is masked out and at
least one kept.
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

import consist_ref as R  # noqa: E402

# name -> (N, C, B, random edges, logit scale, p_cutoff, base seed)
CASES = {
    "consist_b300": (420, 47, 300, 2300, 2.0, 0.5, 3000),
    "consist_b65": (130, 7, 65, 500, 3.0, 0.7, 3100),
}
MODES = {"hard": ("ce", True), "soft": ("ce", False), "l2": ("l2", True)}


def run(mod, yp, yn, B, name, hard, cutoff, w):
    a, b = yp.clone().requires_grad_(True), yn.clone().requires_grad_(True)
    loss = mod.fix_cr(a, b, np.arange(3), batch_size=B, name=name, p_cutoff=cutoff, use_hard_labels=hard, w=w)
    loss.backward()
    zero = torch.zeros_like(a)
    ga = zero if a.grad is None else a.grad
    gb = zero if b.grad is None else b.grad
    assert torch.count_nonzero(ga[B:]) == 0 and torch.count_nonzero(gb[B:]) == 0
    return loss.detach().numpy(), ga[:B].numpy(), gb[:B].numpy()


def case(mod, tag, N, C, B, E, scale, cutoff, seed):
    yp, yn, used, kept = R.admissible_pair(N, C, B, scale, cutoff, seed)
    ei = R.graph_edges(N, E, used)
    deg = torch.bincount(ei[0], minlength=N)
    assert int(deg[0]) >= 200 and int(deg[1]) == 0
    assert bool((ei[0] == ei[1]).any())
    assert torch.unique(ei, dim=1).size(1) < ei.size(1)
    assert bool((ei[0][1:] < ei[0][:-1]).any()) and bool((ei[1][1:] < ei[1][:-1]).any())
    with torch.no_grad():
        w = mod.get_uncertainty_batch(ei, yp, C, "cpu")
    assert w.dtype == torch.float32 and w.shape == (N,) and float(w[1]) == 1.0
    out = {"edge_index": ei.numpy(), "y_pure": yp.numpy(), "y_noisy": yn.numpy(), "w": w.numpy(),
           "B": np.array(B), "C": np.array(C), "p_cutoff": np.array(cutoff, dtype=np.float64),
           "mask": R.keep_mask(yp, B, cutoff).numpy(), "meta/seed": np.array(used)}
    for mode, (name, hard) in MODES.items():
        loss, ga, gb = run(mod, yp, yn, B, name, hard, cutoff, w)
        out[f"{mode}/loss"], out[f"{mode}/grad_pure"], out[f"{mode}/grad_noisy"] = loss, ga, gb
        if mode != "l2":
            out[f"{mode}/loss_w_none"] = run(mod, yp, yn, B, name, hard, cutoff, None)[0]
            out[f"{mode}/loss_cutoff0"] = run(mod, yp, yn, B, name, hard, 0.0, w)[0]
    path = os.path.join(HERE, tag + ".npz")
    np.savez_compressed(path, **out)
    print(f"{tag}: {os.path.getsize(path) / 1024:.1f} KiB, seed {used}, {ei.size(1)} edges, kept {kept} of {B}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="the reference checkout (read only)")
    args = ap.parse_args()
    if args.ref not in sys.path:
        sys.path.insert(0, args.ref)
    mod = importlib.import_module("src.utils.losses")
    for tag, c in CASES.items():
        case(mod, tag, *c)


if __name__ == "__main__":
    main()
