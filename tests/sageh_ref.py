"""CPU restatement of SAGEH in plain torch (TEST INFRASTRUCTURE: only tests
import it; the product path is ngnn.SAGEH on the device).

A GraphSAGE stack over ``oracle.pyg_ref.SAGEConv`` that returns ``(logits,
h)``: ``h`` the last hidden activation after ReLU and before dropout.  The
dropout of every hidden layer is an explicit keep mask (``keeps[i]`` for layer
i, a bool tensor; survivors scale by ``scale``) so that a test can feed it the
device's hash mask (test_gpu_fused.dropout_keep); ``keeps=None`` is no
dropout.  Works in any dtype (``.double()`` for the fp64 yardstick).  Pinned
against the reference's own model file by tests/golden/sageh_*.npz
(tests/golden/make_golden_sageh.py).
"""
from __future__ import annotations

import torch
import torch.nn as nn

from oracle import pyg_ref


class SAGEH(nn.Module):
    def __init__(self, in_size, hidden_size, out_size, num_layers, dropout=0.5, aggr="mean"):
        super().__init__()
        assert num_layers >= 2
        self.num_layers, self.dropout = num_layers, dropout
        self.act = nn.PReLU()  # (unused, as in the reference: state-dict keys only)
        sizes = [in_size] + [hidden_size] * (num_layers - 1) + [out_size]
        self.convs = nn.ModuleList(pyg_ref.SAGEConv(a, b, aggr=aggr) for a, b in zip(sizes, sizes[1:]))
        self.bnl = nn.BatchNorm1d(128)  # (unused)

    def forward(self, x, edge_index, keeps=None, scale=1.0):
        h = None
        for i, conv in enumerate(self.convs):
            x = conv(x, edge_index)
            if i < self.num_layers - 1:
                h = torch.relu(x)
                x = h if keeps is None else h * keeps[i].to(h.dtype) * scale
        return x, h


def fixture_loss(out, h, rec):
    """The scalar the fixtures differentiate (``rec``: the loaded .npz)."""
    G1, G2 = (torch.as_tensor(rec[k]).to(out.device) for k in ("G1", "G2"))
    return (out * G1).sum() + (h * G2).sum()
