"""Generate tests/golden/rewire_*.npz.

Run where the reference checkout is present:

    python tests/golden/make_golden_rewire.py --ref <reference checkout>

As make_golden_sagepl.py: the reference's OWN ``src/utils/augmentation.py``
is imported from the read-only checkout and its ``topk_rewire(h, edge_index,
'cpu', k_percent, directed=False)`` is executed on the CPU.  Only tensors are
written: ``h``, ``edge_index``, ``k_percent`` and the two edge lists it
returned.  Every case has 10 duplicated edges and 5 self-loops
(tests/rewire_ref.make_case) and records its seed.
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

from rewire_ref import make_case  # noqa: E402

# name -> (N, F, ReLU'd, seed, k_percent)
CASES = {
    "rewire_relu_333": (333, 100, True, 3100, 0.1),
    "rewire_signed_257": (257, 131, False, 3200, 0.2),
    "rewire_relu_130": (130, 32, True, 3300, 0.1),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="the reference checkout (read only)")
    args = ap.parse_args()
    if args.ref not in sys.path:
        sys.path.insert(0, args.ref)
    aug = importlib.import_module("src.utils.augmentation")
    for name, (n, f, relu, seed, kp) in CASES.items():
        h, ei = make_case(n, f, relu, seed)
        pos, neg = aug.topk_rewire(h, ei, "cpu", k_percent=kp, directed=False)
        path = os.path.join(HERE, name + ".npz")
        np.savez_compressed(path, h=h.numpy(), edge_index=ei.numpy(), k_percent=np.array(kp, dtype=np.float64),
                            pos_edge=pos.numpy(), neg_edge=neg.numpy(), **{"meta/seed": np.array(seed)})
        print(f"{name}: {os.path.getsize(path) / 1024:.1f} KiB, E={ei.size(1)}, pos={tuple(pos.shape)}, "
              f"neg={tuple(neg.shape)}")


if __name__ == "__main__":
    main()
