"""CPU restatement of SAGEPL in plain torch (TEST INFRASTRUCTURE: only tests
import it; the product path is ngnn.SAGEPL on the device).

A GraphSAGE stack over ``oracle.pyg_ref.SAGEConv`` plus a learnable noise
table.  One call runs the stack on ``x`` and again on
``x + [sign(x) *] normalize(noise[n_id]) * noise_rate`` (the sign factor only
without ``n_id``, where the whole table is taken in row order) and returns,
for each pass, the last hidden activation (after ReLU and the optional batch
norm, before dropout), the log-softmax of the logits and the logits.  Pinned
against the reference's own model file by tests/golden/sagepl_*.npz
(tests/golden/make_golden_sagepl.py).
"""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle import pyg_ref


def noisy_input(x, noise, rate, n_id=None):
    """What the noisy pass reads (torch composition, any device)."""
    if n_id is None:
        return x + torch.sign(x) * F.normalize(noise, dim=1) * rate
    return x + F.normalize(noise[n_id], dim=1) * rate


class SAGEPL(nn.Module):
    def __init__(self, in_size, hidden_size, out_size, num_layers, nbr_nodes, dropout=0.5,
                 use_bn=False, aggr="mean"):
        super().__init__()
        assert num_layers >= 2
        self.num_layers, self.dropout, self.use_bn = num_layers, dropout, use_bn
        sizes = [in_size] + [hidden_size] * (num_layers - 1) + [out_size]
        self.convs = nn.ModuleList(pyg_ref.SAGEConv(a, b, aggr=aggr) for a, b in zip(sizes, sizes[1:]))
        self.noise = nn.Parameter(torch.randn(nbr_nodes, in_size))
        if use_bn:
            self.bn1 = nn.BatchNorm1d(in_size)
            self.bn2 = nn.BatchNorm1d(hidden_size)

    def stack(self, x, edge_index):
        if self.use_bn:
            x = self.bn1(x)
        hidden = None
        for i, conv in enumerate(self.convs):
            x = conv(x, edge_index)
            if i < self.num_layers - 1:
                x = torch.relu(x)
                if self.use_bn:
                    x = self.bn2(x)
                hidden = x
                x = F.dropout(x, p=self.dropout, training=self.training)
        return hidden, torch.log_softmax(x, dim=1), x

    def forward(self, x, edge_index, noise_rate=0.1, n_id=None):
        return self.stack(x, edge_index) + self.stack(noisy_input(x, self.noise, noise_rate, n_id), edge_index)


OUT_NAMES = ("h_pure", "logp_pure", "z_pure", "h_noisy", "logp_noisy", "z_noisy")


def fixture_loss(outs, rec):
    """The scalar the fixtures differentiate: seeded cotangents on h_noisy,
    z_noisy and z_pure (``rec``: the loaded .npz)."""
    G1, G2, G3 = (torch.as_tensor(rec[k]).to(outs[0].device) for k in ("G1", "G2", "G3"))
    return (outs[3] * G1).sum() + (outs[5] * G2).sum() + (outs[2] * G3).sum()
