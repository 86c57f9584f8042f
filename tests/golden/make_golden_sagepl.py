"""Generate tests/golden/sagepl_block.npz and sagepl_sign.npz.

Run where the reference checkout is present:

    python tests/golden/make_golden_sagepl.py --ref <reference checkout>

As make_golden.py: the reference's OWN ``src/models/layers/sagePL.py`` is
imported from the read-only checkout and executed, with ``torch_geometric.nn``
supplied by ``oracle.pyg_ref`` (make_golden.install_shim).  Only tensors are
written: inputs, parameters, the six outputs, the cotangents and the
gradients.  Of the noise table's gradient only the rows named by ``n_id`` are
stored, with a flag that every other row is exactly zero.
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

OUT_NAMES = ("h_pure", "logp_pure", "z_pure", "h_noisy", "logp_noisy", "z_noisy")


def run_case(model, x, ei, n_id, rate, seed):
    model.eval()
    outs = model(x, ei, noise_rate=rate, n_id=n_id)
    g = torch.Generator().manual_seed(seed)
    G1 = torch.randn(outs[3].shape, generator=g)
    G2 = torch.randn(outs[5].shape, generator=g)
    G3 = torch.randn(outs[2].shape, generator=g)
    ((outs[3] * G1).sum() + (outs[5] * G2).sum() + (outs[2] * G3).sum()).backward()
    rec = {"x": x.numpy(), "edge_index": ei.numpy(), "noise_rate": np.array(rate, dtype=np.float64),
           "G1": G1.numpy(), "G2": G2.numpy(), "G3": G3.numpy(), "meta/seed": np.array(seed)}
    for name, o in zip(OUT_NAMES, outs):
        rec["out/" + name] = o.detach().numpy()
    for k, v in model.state_dict().items():
        rec["param/" + k] = v.detach().numpy().copy()
    rows = torch.arange(model.noise.size(0)) if n_id is None else n_id
    for k, p in model.named_parameters():
        if k == "noise":
            gn = p.grad.detach()
            rec["grad/noise_rows"] = gn[rows].numpy().copy()
            rest = torch.ones(gn.size(0), dtype=torch.bool)
            rest[rows] = False
            rec["grad/noise_rest_zero"] = np.array(bool((gn[rest] == 0).all()))
        else:
            rec["grad/" + k] = p.grad.detach().numpy().copy()
    if n_id is not None:
        rec["n_id"] = n_id.numpy()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="the reference checkout (read only)")
    args = ap.parse_args()
    install_shim("mean")
    if args.ref not in sys.path:
        sys.path.insert(0, args.ref)
    sys.modules.pop("src.models.layers.sagePL", None)
    pl = importlib.import_module("src.models.layers.sagePL")
    cases = {}

    # 1. a sampled block with n_id (no sign factor), 3 layers 100 -> 32 -> 32 -> 47,
    #    one of the block's noise rows all zero (the clamped-norm branch)
    torch.manual_seed(1100)
    n_id, ei = block_graph(1, 12, [10, 5], 250)
    x = torch.randn(len(n_id), 100, generator=torch.Generator().manual_seed(21))
    m = pl.SAGEPL(100, 32, 47, 3, nbr_nodes=250, dropout=0.0)
    with torch.no_grad():
        m.noise[n_id[5]] = 0.0
    cases["sagepl_block"] = run_case(m, x, ei, n_id, 0.05, 1100)
    cases["sagepl_block"]["meta/zero_row"] = np.array(int(n_id[5]))

    # 2. n_id=None: the sign branch over the whole table, exact zeros in x
    torch.manual_seed(1200)
    n_sub = 40
    ei = random_graph(23, n_sub, 300, "dst")
    x = torch.relu(torch.randn(n_sub, 8, generator=torch.Generator().manual_seed(24))).round()
    x[::3] = -x[::3]
    m = pl.SAGEPL(8, 8, 3, 2, nbr_nodes=n_sub, dropout=0.0)
    cases["sagepl_sign"] = run_case(m, x, ei, None, 0.1, 1200)

    for name, rec in cases.items():
        path = os.path.join(HERE, name + ".npz")
        np.savez_compressed(path, **rec)
        print(f"{name}: {os.path.getsize(path) / 1024:.1f} KiB, keys={len(rec)}, "
              f"shapes={[tuple(rec['out/' + n].shape) for n in OUT_NAMES[:3]]}")


if __name__ == "__main__":
    main()
