"""backward_correction and CoDiLoss (forward + backward) at the seed-row
shapes B=1024, C=47 and B=512, C=40 (config_arxiv5.yml's), against the
reference's op sequences (src/utils/losses.py:51-70, :106-137) run in torch
with every tensor on the device.

Variants, same process, same GPU, alternating group by group; device events
around groups of calls, warm-up first, medians over the groups
(bench_rewire.py's method):

  bc_ngnn          ngnn.losses.backward_correction (+ backward)
  bc_torch         the reference as it stands: np.linalg.inv and a host-to-
                   device copy per call, one-hot scatter, softmax, clamp, log,
                   matmul, mean (+ autograd backward)
  bc_torch_cached  the same with the inverse kept on the device -- the
                   strongest version of what a user has without the op
  codi_ngnn        ngnn.losses.CoDiLoss (+ both backwards)
  codi_torch       the reference as it stands: two np.argsort host round trips
  codi_torch_dev   the same with torch.sort on the device (no host round trip)

At these sizes every variant is a handful of launches of a few microseconds
each, so a call's time is mostly the host's launch cost: the figures say what
a loop pays per loss, not what the kernels could stream.  Also checked: each
ngnn result against its torch variant, and bitwise repeatability.

Writes one JSON file (default profiles/noisy_losses.json) and prints it.
Needs the GPU.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "noise-gnn_amd"), ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from bench_rewire import timed_groups  # noqa: E402


def bc_torch(output, labels, C, nbr_class, device, c_inv=None):
    """losses.py:51-70; c_inv given: the inverse kept on the device."""
    if c_inv is None:
        c_inv = torch.from_numpy(np.linalg.inv(C).astype(np.float32)).to(device)
    label_oh = torch.zeros(len(labels), nbr_class, device=device)
    label_oh.scatter_(1, labels.view(-1, 1), 1)
    output = torch.softmax(output, dim=1)
    output = torch.clamp(output, min=1e-5, max=1.0 - 1e-5)
    return -torch.mean(torch.matmul(label_oh, c_inv) * torch.log(output))


def codi_torch(y_1, y_2, y_noise, forget_rate, ind, noise_or_not, co_lambda, host_sort):
    """losses.py:106-137; host_sort: np.argsort on a host copy, as it stands
    (ind and noise_or_not stay on the device: one round trip per argsort)."""
    p, q = F.softmax(y_1, dim=1), F.softmax(y_2, dim=1)
    mean = (p + q) / 2
    js = ((F.kl_div(F.log_softmax(y_1, dim=1), mean, reduction="none")
           + F.kl_div(F.log_softmax(y_2, dim=1), mean, reduction="none")) / 2).sum(1).detach()
    loss_1 = F.cross_entropy(y_1, y_noise, reduction="none") - co_lambda * js
    loss_2 = F.cross_entropy(y_2, y_noise, reduction="none") - co_lambda * js
    if host_sort:
        s1 = torch.from_numpy(np.argsort(loss_1.detach().cpu().numpy())).to(y_1.device)
        s2 = torch.from_numpy(np.argsort(loss_2.detach().cpu().numpy())).to(y_1.device)
    else:
        s1, s2 = torch.argsort(loss_1.detach()), torch.argsort(loss_2.detach())
    nr = int((1 - forget_rate) * len(loss_1)) or len(loss_1)
    k1, k2 = s1[:nr], s2[:nr]
    pr1 = torch.sum(noise_or_not[ind[k1]]) / float(nr)
    pr2 = torch.sum(noise_or_not[ind[k2]]) / float(nr)
    return F.cross_entropy(y_1[k2], y_noise[k2]), F.cross_entropy(y_2[k1], y_noise[k1]), pr1, pr2


def run_shape(B, C, args, dev):
    from ngnn.losses import CoDiLoss, backward_correction
    g = torch.Generator().manual_seed(B + C)
    x = (2 * torch.randn(B, C, generator=g)).to(dev).requires_grad_(True)
    y1 = (2 * torch.randn(B, C, generator=g)).to(dev).requires_grad_(True)
    y2 = (2 * torch.randn(B, C, generator=g)).to(dev).requires_grad_(True)
    y = torch.randint(0, C, (B,), generator=g).to(dev)
    ind = torch.randperm(3 * B, generator=g)[:B].to(dev)
    clean = (torch.rand(3 * B, generator=g) < 0.6).to(dev)
    mat = np.full((C, C), 0.3 / (C - 1))
    np.fill_diagonal(mat, 0.7)
    c_inv = torch.from_numpy(np.linalg.inv(mat).astype(np.float32)).to(dev)
    crit = CoDiLoss(dev, 0.1)

    def bwd(*losses):
        for t in (x, y1, y2):
            t.grad = None
        for l_ in losses:
            l_.backward()

    fns = {
        "bc_ngnn": lambda: bwd(backward_correction(x, y, mat, C, dev)),
        "bc_torch": lambda: bwd(bc_torch(x, y, mat, C, dev)),
        "bc_torch_cached": lambda: bwd(bc_torch(x, y, mat, C, dev, c_inv)),
        "codi_ngnn": lambda: bwd(*crit(y1, y2, y, 0.2, ind, clean)[:2]),
        "codi_torch": lambda: bwd(*codi_torch(y1, y2, y, 0.2, ind, clean, 0.1, True)[:2]),
        "codi_torch_dev": lambda: bwd(*codi_torch(y1, y2, y, 0.2, ind, clean, 0.1, False)[:2]),
    }
    # agreement and repeatability
    a, b = backward_correction(x, y, mat, C, dev), bc_torch(x, y, mat, C, dev, c_inv)
    ga, gb = torch.autograd.grad(a, x)[0].clone(), torch.autograd.grad(b, x)[0]
    o, t = crit(y1, y2, y, 0.2, ind, clean), codi_torch(y1, y2, y, 0.2, ind, clean, 0.1, False)
    go, gt = torch.autograd.grad(o[0], y1)[0].clone(), torch.autograd.grad(t[0], y1)[0]
    a2 = backward_correction(x, y, mat, C, dev)
    o2 = crit(y1, y2, y, 0.2, ind, clean)
    check = dict(
        bc_loss_rel=float((a - b).abs() / b.abs()), bc_grad_err_over_max=float((ga - gb).abs().max() / gb.abs().max()),
        codi_loss_rel=float((o[0] - t[0]).abs() / t[0].abs()),
        codi_grad_err_over_max=float((go - gt).abs().max() / gt.abs().max()),
        codi_pure_ratio_abs_diff=float(max((o[2] - t[2]).abs(), (o[3] - t[3]).abs())),
        bitwise_repeatable=bool(torch.equal(a, a2) and torch.equal(o[0], o2[0]) and torch.equal(o[1], o2[1])))
    res = timed_groups(fns, {k: args.inner for k in fns}, args.reps, args.warmup)
    us = {k: round(v["median_ms"] * 1e3, 2) for k, v in res.items()}
    ratios = {
        "bc_torch_over_ngnn": us["bc_torch"] / us["bc_ngnn"],
        "bc_torch_cached_over_ngnn": us["bc_torch_cached"] / us["bc_ngnn"],
        "codi_torch_over_ngnn": us["codi_torch"] / us["codi_ngnn"],
        "codi_torch_dev_over_ngnn": us["codi_torch_dev"] / us["codi_ngnn"],
    }
    faster = {k: bool(res[k]["min_ms"] > res[n]["max_ms"])
              for k, n in (("bc_torch", "bc_ngnn"), ("bc_torch_cached", "bc_ngnn"), ("codi_torch", "codi_ngnn"),
                           ("codi_torch_dev", "codi_ngnn"))}
    return dict(shape=dict(B=B, C=C), agreement=check, times=res, median_us_per_call=us, ratios=ratios,
                ngnn_faster_beyond_spread=faster)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "noisy_losses.json"))
    ap.add_argument("--reps", type=int, default=15, help="groups per variant")
    ap.add_argument("--inner", type=int, default=20, help="calls (forward + backward) per group")
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_noisy_losses: needs the GPU (no fallback)")
    dev = torch.device("cuda:0")
    out = {
        "device": torch.cuda.get_device_name(0),
        "method": dict(reps=args.reps, inner=args.inner, warmup=args.warmup,
                       note="forward + backward per call; device events around groups of calls, variants "
                            "alternating; medians over the groups; host-launch bound at these sizes"),
        "shapes": [run_shape(B, C, args, dev) for B, C in ((1024, 47), (512, 40))],
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
