"""Generate tests/golden/sageh_block.npz and sageh_eval.npz.

Run where the reference checkout is present:

    python tests/golden/make_golden_sageh.py --ref <reference checkout>

As make_golden_sagepl.py: the reference's OWN ``src/models/layers/sageH.py``
is imported from the read-only checkout and executed, with
``torch_geometric.nn`` supplied by ``oracle.pyg_ref``
(make_golden.install_shim).  Only tensors are written: inputs, the state dict
(the unused ``act`` and ``bnl`` members included), both outputs, two random
cotangents and every weight gradient of ``(out * G1).sum() + (h * G2).sum()``.
Both cases run with ``dropout=0.0`` (the reference's dropout is torch's RNG).
"""
from __future__ import annotations

import argparse
import importlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden import block_graph, install_shim, random_graph  # noqa: E402


def run_case(model, x, ei, training, seed):
    out, h = model(x, ei, training=training)
    g = torch.Generator().manual_seed(seed)
    G1 = torch.randn(out.shape, generator=g)
    G2 = torch.randn(h.shape, generator=g)
    ((out * G1).sum() + (h * G2).sum()).backward()
    rec = {"x": x.numpy(), "edge_index": ei.numpy(), "G1": G1.numpy(), "G2": G2.numpy(),
           "out/out": out.detach().numpy(), "out/h": h.detach().numpy(),
           "meta/seed": np.array(seed), "meta/training": np.array(bool(training))}
    for k, v in model.state_dict().items():
        rec["param/" + k] = v.detach().numpy().copy()
    for k, p in model.named_parameters():
        if p.grad is not None:  # (act and bnl take no part in the forward)
            rec["grad/" + k] = p.grad.detach().numpy().copy()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="the reference checkout (read only)")
    args = ap.parse_args()
    install_shim("mean")
    if args.ref not in sys.path:
        sys.path.insert(0, args.ref)
    sys.modules.pop("src.models.layers.sageH", None)
    sh = importlib.import_module("src.models.layers.sageH")
    cases = {}

    # 1. a sampled block, 3 layers 100 -> 32 -> 32 -> 47 (training=True: the default)
    torch.manual_seed(2100)
    n_id, ei = block_graph(1, 12, [10, 5], 250)
    x = torch.randn(len(n_id), 100, generator=torch.Generator().manual_seed(31))
    cases["sageh_block"] = run_case(sh.SAGEH(100, 32, 47, 3, dropout=0.0), x, ei, True, 2100)

    # 2. 2 layers 8 -> 8 -> 3 with training=False
    torch.manual_seed(2200)
    ei = random_graph(33, 40, 300, "dst")
    x = torch.randn(40, 8, generator=torch.Generator().manual_seed(34))
    cases["sageh_eval"] = run_case(sh.SAGEH(8, 8, 3, 2, dropout=0.0), x, ei, False, 2200)

    for name, rec in cases.items():
        path = os.path.join(HERE, name + ".npz")
        np.savez_compressed(path, **rec)
        print(f"{name}: {os.path.getsize(path) / 1024:.1f} KiB, keys={len(rec)}, "
              f"out={tuple(rec['out/out'].shape)}, h={tuple(rec['out/h'].shape)}")


if __name__ == "__main__":
    main()
