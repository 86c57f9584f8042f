"""Generate tests/golden/label_noise.npz.

Run where the reference checkout is present:

    python tests/golden/make_golden_label_noise.py --ref <reference checkout>

As make_golden_contrast.py: the reference's OWN ``src/utils/noise.py`` is
imported from the read-only checkout and its ``flip_label(labels, nbr_classes,
noise_type, prob)`` is run on the CPU, under ``np.random.seed(seed)``, on the
first 20,000 entries of ``np.random.RandomState(5).randint(0, C, 200000)`` for
the five cases of tests/label_noise_ref.py.  Only arrays are written, per
case: the numpy seed, the reference's ``noise_mat`` (float64) and its noisy
labels in the narrowest integer type.  Where the reference itself fails
(``aim_pair`` below 6 classes: an ``IndexError`` while it fills the matrix),
the case holds its seed and the exception's name instead.

Asserted here: every noisy label is a class of non-zero probability in its
clean label's row, and the squeezed output kept its length.
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

import label_noise_ref as R  # noqa: E402

SEED0 = 4100


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="the reference checkout (read only)")
    args = ap.parse_args()
    if args.ref not in sys.path:
        sys.path.insert(0, args.ref)
    mod = importlib.import_module("src.utils.noise")
    arrays = {}
    for n, (name, (noise_type, C, prob)) in enumerate(R.CASES.items()):
        seed = SEED0 + n
        y = R.case_labels(C)[:R.N_FIXTURE]
        np.random.seed(seed)
        try:
            noisy, mat = mod.flip_label(torch.from_numpy(y), C, noise_type, prob)
        except IndexError as e:
            # aim_pair's fixed pairs name classes 0..5: below 6 classes the reference cannot build its matrix
            arrays[name + "/seed"] = np.array(seed)
            arrays[name + "/reference_raised"] = np.array(type(e).__name__)
            print(f"{name}: the reference raised {type(e).__name__}: {e}")
            continue
        noisy = noisy.numpy()
        assert noisy.shape == y.shape and mat.shape == (C, C) and mat.dtype == np.float64
        assert (mat[y, noisy] > 0).all()
        arrays[name + "/seed"] = np.array(seed)
        arrays[name + "/noise_mat"] = mat
        arrays[name + "/noisy"] = noisy.astype(np.min_scalar_type(C - 1))
        print(f"{name}: kept {float((noisy == y).mean()):.4f} of {y.size} labels (1 - prob = {1 - prob})")
    path = os.path.join(HERE, "label_noise.npz")
    np.savez_compressed(path, **arrays)
    print(f"label_noise.npz: {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
