"""shuffle_pos and contrastive_loss at the training shapes, against what a
user has without them.

shuffle_pos, N = 165,000 rows (a products [15, 10] block), F = 100 / prob 0.7
(products) and F = 128 / prob 0.9 (arxiv):

  shuffle_ngnn       ngnn.ops.shuffle_pos (one launch)
  shuffle_torch_vec  the same draw vectorised in torch on the device: rand,
                     argsort, a second rand + argsort over the selection,
                     gather, scatter (the strongest version without the op)
  shuffle_ref_loop   the reference's row loop (augmentation.py:95-100: two
                     torch.randperm and an indexed write per row) restated in
                     torch, on a 4096-row slice of the device tensor, host
                     clock around a synchronise; scaled to N rows by N / 4096
                     (the loop is linear in the rows), reported as an estimate

contrastive_loss forward + backward, N = 165,000, H in {256, 512}, M = 205
indices below 1024 (batch 1024, forget rate 0.2):

  contrast_ngnn      ngnn.losses.contrastive_loss(h, hp, hn, idx)
  contrast_ngnn_bs   the same with batch_size=1024 (zero-row gradient buffers)
  contrast_torch     the reference's op sequence in torch on the device: three
                     row gathers, two mul + sum, two BCEWithLogitsLoss, and
                     autograd's three [N, H] index backward gradients

Same process, same GPU, variants alternating group by group; device events
around groups of calls, warm-up first, medians over the groups
(bench_rewire.py's method).  The shuffle's share of HBM is the op's
algorithmic bytes (one read and one write of [N, F] floats) over its median
time, against the 8 TB/s peak.  Also checked: contrast_ngnn against the torch
composition, and the shuffle's invariants.

Writes one JSON file (default profiles/contrast.json) and prints it.  Needs
the GPU.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "noise-gnn_amd"), ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

from bench_rewire import timed_groups  # noqa: E402

HBM_PEAK = 8.0e12  # bytes / s
N_ROWS = 165_000
LOOP_ROWS = 4096


def shuffle_torch_vec(x, m):
    """A uniform m-subset per row, its values permuted uniformly: the
    reference's draw, vectorised."""
    N, F = x.shape
    sel = torch.argsort(torch.rand(N, F, device=x.device), dim=1)[:, :m]
    perm = torch.argsort(torch.rand(N, m, device=x.device), dim=1)
    out = x.clone()
    out.scatter_(1, sel, x.gather(1, sel.gather(1, perm)))
    return out


def shuffle_ref_loop(x, m):
    """augmentation.py:93-100 as it stands."""
    out = x.clone().detach()
    for i in range(out.shape[0]):
        indices = torch.randperm(out.shape[1])[:m]
        selected = out[i, indices]
        out[i, indices] = selected[torch.randperm(selected.shape[0])]
    return out


def contrast_torch(h, hp, hn, idx):
    """data_utils.py:34-64 after the three gathers of pipeline_test.py:139."""
    H, Hp, Hn = h[idx], hp[idx], hn[idx]
    lp = torch.squeeze(torch.sum(torch.mul(H, Hp), dim=1, keepdim=True))
    ln = torch.squeeze(torch.sum(torch.mul(H, Hn), dim=1, keepdim=True))
    crit = torch.nn.BCEWithLogitsLoss()
    return crit(lp, torch.ones_like(lp)) + crit(ln, torch.zeros_like(ln))


def run_shuffle(F, prob, args, dev):
    from ngnn.ops import shuffle_pos
    x = torch.randn(N_ROWS, F, device=dev)
    m = int(F * prob)
    fns = {
        "shuffle_ngnn": lambda: shuffle_pos(x, prob=prob, seed=17),
        "shuffle_torch_vec": lambda: shuffle_torch_vec(x, m),
    }
    out = shuffle_pos(x, prob=prob, seed=17)
    check = dict(
        rows_are_permutations=bool(torch.equal(out.sort(dim=1).values, x.sort(dim=1).values)),
        max_moved_per_row=int((out != x).sum(1).max()), m=m,
        repeatable=bool(torch.equal(out, shuffle_pos(x, prob=prob, seed=17))))
    res = timed_groups(fns, {"shuffle_ngnn": args.inner, "shuffle_torch_vec": max(args.inner // 4, 1)},
                       args.reps, args.warmup)
    xs = x[:LOOP_ROWS]
    shuffle_ref_loop(xs[:64], m)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    shuffle_ref_loop(xs, m)
    torch.cuda.synchronize()
    loop_ms = (time.perf_counter() - t0) * 1e3
    us = {k: round(v["median_ms"] * 1e3, 2) for k, v in res.items()}
    nbytes = 2 * N_ROWS * F * 4
    return dict(
        shape=dict(N=N_ROWS, F=F, prob=prob, m=m), checks=check, times=res, median_us_per_call=us,
        algorithmic_bytes=nbytes, ngnn_fraction_of_hbm_peak=nbytes / (res["shuffle_ngnn"]["median_ms"] * 1e-3) / HBM_PEAK,
        ref_loop=dict(rows=LOOP_ROWS, ms=loop_ms, estimated_ms_at_N=loop_ms * N_ROWS / LOOP_ROWS, runs=1),
        ratios=dict(torch_vec_over_ngnn=us["shuffle_torch_vec"] / us["shuffle_ngnn"],
                    ref_loop_estimate_over_ngnn=loop_ms * N_ROWS / LOOP_ROWS * 1e3 / us["shuffle_ngnn"]))


def run_contrast(H, args, dev):
    from ngnn.losses import contrastive_loss
    B, M = 1024, 205
    g = torch.Generator().manual_seed(H)
    h, hp, hn = (torch.relu(0.25 * torch.randn(N_ROWS, H, generator=g)).to(dev).requires_grad_(True)
                 for _ in range(3))
    idx = torch.randperm(B, generator=g)[:M].to(dev)

    def step(fn):
        for t in (h, hp, hn):
            t.grad = None
        fn().backward()

    fns = {
        "contrast_ngnn": lambda: step(lambda: contrastive_loss(h, hp, hn, idx)),
        "contrast_ngnn_bs": lambda: step(lambda: contrastive_loss(h, hp, hn, idx, batch_size=B)),
        "contrast_torch": lambda: step(lambda: contrast_torch(h, hp, hn, idx)),
    }
    a, b = contrastive_loss(h, hp, hn, idx), contrast_torch(h, hp, hn, idx)
    ga = [t.clone() for t in torch.autograd.grad(a, (h, hp, hn))]
    gb = torch.autograd.grad(b, (h, hp, hn))
    check = dict(loss_rel=float((a - b).abs() / b.abs()),
                 grad_err_over_max=[float((x - y).abs().max() / y.abs().max()) for x, y in zip(ga, gb)],
                 bitwise_repeatable=bool(torch.equal(a, contrastive_loss(h, hp, hn, idx))))
    del ga, gb
    res = timed_groups(fns, {k: args.inner for k in fns}, args.reps, args.warmup)
    us = {k: round(v["median_ms"] * 1e3, 2) for k, v in res.items()}
    return dict(shape=dict(N=N_ROWS, H=H, M=M, batch_size=B), agreement=check, times=res, median_us_per_call=us,
                ratios=dict(torch_over_ngnn=us["contrast_torch"] / us["contrast_ngnn"],
                            torch_over_ngnn_bs=us["contrast_torch"] / us["contrast_ngnn_bs"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "contrast.json"))
    ap.add_argument("--reps", type=int, default=15, help="groups per variant")
    ap.add_argument("--inner", type=int, default=20, help="calls per group")
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_contrast: needs the GPU (no fallback)")
    dev = torch.device("cuda:0")
    out = {
        "device": torch.cuda.get_device_name(0),
        "method": dict(reps=args.reps, inner=args.inner, warmup=args.warmup,
                       note="device events around groups of calls, variants alternating; medians over the "
                            "groups; contrastive_loss is forward + backward per call; the reference's row "
                            "loop is one host-clocked run on a 4096-row slice"),
        "shuffle_pos": [run_shuffle(F, prob, args, dev) for F, prob in ((100, 0.7), (128, 0.9))],
        "contrastive_loss": [run_contrast(H, args, dev) for H in (256, 512)],
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
