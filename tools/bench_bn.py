"""The fused ReLU-BatchNorm-dropout op (ngnn.ops.batch_norm_act) against the
torch composition it replaces, and one eager SAGE(use_bn=True) step with and
without it.

Op shapes (forward + backward per call, and the forward alone):
  hidden  169,984 x 256, relu=True, p=0.5, x needs a gradient (bn2 of the
          products block)
  input   169,984 x 100, relu=False, p=0, x needs no gradient (bn1: the
          backward's dx pass is skipped)
Variants: a_torch = x.relu() / F.batch_norm(training=True) / F.dropout on
the device; b_ngnn = batch_norm_act.  Same process, same GPU, device events
around groups of calls, warm-up first, the variants alternating group by
group, medians and the min-max spread over the groups
(bench_rewire.py's timed_groups).  Bytes: the algorithmic count
3 N F 4 (forward) + 4 N F 4 (backward, 2 N F 4 without dx) and the count the
kernels move as built (the backward with dx reads dout and x twice and writes
dx: 5 N F 4), each over the median time as a fraction of the 8 TB/s HBM peak.

Model step: SAGE(100, 256, 47, 2, use_bn=True, dropout=0.5), forward,
cross-entropy on the seed rows, backward and an Adam step on the sampled
products [15, 10] batch-1024 block.  b_ngnn is the tree as it stands;
a_parent runs the op sequence the models ran before batch_norm_act existed
(bn1, conv, relu, bn2, F.dropout: the op's torch route, forced), in the same
process, alternating.

Writes one JSON file (default profiles/bn_bench.json) and prints it.  Needs
the GPU.
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

import torch  # noqa: E402
import torch.nn as nn  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from bench_consistency import count_kernels  # noqa: E402
from bench_rewire import timed_groups  # noqa: E402

HBM_PEAK = 8.0e12  # bytes / s


def spread(res):
    us = {k: round(v["median_ms"] * 1e3, 2) for k, v in res.items()}
    mm = {k: [round(v["min_ms"] * 1e3, 2), round(v["max_ms"] * 1e3, 2)] for k, v in res.items()}
    return us, mm


def verdict(res, a, b):
    """b against a: beyond the spread means the two min-max ranges do not overlap."""
    return dict(a_over_b=res[a]["median_ms"] / res[b]["median_ms"],
                b_faster_beyond_spread=bool(res[a]["min_ms"] > res[b]["max_ms"]),
                b_slower_beyond_spread=bool(res[b]["min_ms"] > res[a]["max_ms"]))


def run_op(name, N, Fw, relu, p, need_dx, args, dev):
    from ngnn import ops
    gen = torch.Generator().manual_seed(Fw)
    x = torch.randn(N, Fw, generator=gen).to(dev).requires_grad_(need_dx)
    dout = torch.randn(N, Fw, generator=gen).to(dev)
    bn = nn.BatchNorm1d(Fw).to(dev).train()

    def fwd(kind):
        if kind == "a":
            y = F.batch_norm(x.relu() if relu else x, bn.running_mean, bn.running_var, bn.weight, bn.bias, True,
                             0.1, bn.eps)
            return F.dropout(y, p=p, training=True)
        return ops.batch_norm_act(x, bn, relu=relu, p=p, seed=12345)

    def step(kind):
        x.grad = bn.weight.grad = bn.bias.grad = None
        out = fwd(kind)
        out.backward(dout)
        return out

    def fwd_only(kind):
        with torch.no_grad():
            return fwd(kind)

    # agreement without dropout (the masks differ by construction)
    p_keep, p = p, 0.0
    oa = step("a").detach().clone()
    ga = [t.grad.clone() for t in ((x, bn.weight, bn.bias) if need_dx else (bn.weight, bn.bias))]
    ob = step("b").detach()
    gb = [t.grad for t in ((x, bn.weight, bn.bias) if need_dx else (bn.weight, bn.bias))]
    agree = dict(out_err_over_max=float((ob - oa).abs().max() / oa.abs().max()),
                 grads_err_over_max=[float((b - a).abs().max() / a.abs().max()) for a, b in zip(ga, gb)])
    p = p_keep
    names = {"a": "a_torch", "b": "b_ngnn"}
    res = timed_groups({names[k]: (lambda k=k: step(k)) for k in "ab"}, {n: args.inner for n in names.values()},
                       args.reps, args.warmup)
    resf = timed_groups({names[k]: (lambda k=k: fwd_only(k)) for k in "ab"}, {n: args.inner for n in names.values()},
                        args.reps, args.warmup)
    us, mm = spread(res)
    usf, mmf = spread(resf)
    unit = N * Fw * 4
    alg_f, alg_b, moved_b = 3 * unit, (4 if need_dx else 2) * unit, (5 if need_dx else 2) * unit
    tf = resf["b_ngnn"]["median_ms"] * 1e-3
    tb = (res["b_ngnn"]["median_ms"] - resf["b_ngnn"]["median_ms"]) * 1e-3
    return dict(
        case=name, N=N, F=Fw, relu=relu, p=p, dx=need_dx,
        fwd_bwd_median_us=us, fwd_bwd_spread_us_min_max=mm, fwd_bwd=verdict(res, "a_torch", "b_ngnn"),
        fwd_median_us=usf, fwd_spread_us_min_max=mmf, fwd=verdict(resf, "a_torch", "b_ngnn"),
        kernel_launches_per_call={names[k]: count_kernels(lambda k=k: step(k)) for k in "ab"},
        ngnn_bytes=dict(
            fwd_algorithmic=alg_f, fwd_fraction_of_hbm_peak=alg_f / tf / HBM_PEAK,
            bwd_algorithmic=alg_b, bwd_moved=moved_b, bwd_us_by_difference=round(tb * 1e6, 2),
            bwd_algorithmic_fraction_of_hbm_peak=alg_b / tb / HBM_PEAK,
            bwd_moved_fraction_of_hbm_peak=moved_b / tb / HBM_PEAK),
        agreement_with_a_no_dropout=agree)


def run_model(args, dev):
    import ngnn
    from ngnn import models, ops
    from ngnn.loader import sample_block, synthetic_graph
    g = synthetic_graph("ogbn-products", dev, seed=1)
    B = 1024
    batch = sample_block(g, g.train_idx[:B], [15, 10], seed=3, gather_features=False)
    del g
    ei, N = batch.edge_index, int(batch.num_nodes)
    gen = torch.Generator().manual_seed(7)
    x = torch.randn(N, 100, generator=gen).to(dev)
    y = torch.randint(0, 47, (B,), generator=gen).to(dev)
    torch.manual_seed(0)
    model = ngnn.SAGE(100, 256, 47, 2, dropout=0.5, use_bn=True).to(dev).train()
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    real = ops.batch_norm_act_supported

    def step(parent):
        # the parent's op sequence is the op's torch route: bn(x.relu()), F.dropout
        models.batch_norm_act_supported = ops.batch_norm_act_supported = (lambda *a: False) if parent else real
        try:
            opt.zero_grad(set_to_none=True)
            loss = F.cross_entropy(model(x, ei)[:B], y)
            loss.backward()
            opt.step()
        finally:
            models.batch_norm_act_supported = ops.batch_norm_act_supported = real
        return loss

    fns = {"a_parent": lambda: step(True), "b_ngnn": lambda: step(False)}
    res = timed_groups(fns, {k: args.inner for k in fns}, args.reps, args.warmup)
    us, mm = spread(res)
    return dict(model="SAGE(100, 256, 47, 2, use_bn=True, dropout=0.5)", block="ogbn-products [15, 10], 1024 seeds",
                N=N, E=int(ei.size(1)), step_median_us=us, step_spread_us_min_max=mm,
                step=verdict(res, "a_parent", "b_ngnn"),
                kernel_launches_per_step={k: count_kernels(fn) for k, fn in fns.items()})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bn_bench.json"))
    ap.add_argument("--reps", type=int, default=15, help="groups per variant")
    ap.add_argument("--inner", type=int, default=20, help="calls per group")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rows", type=int, default=169984)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_bn: needs the GPU (no fallback)")
    dev = torch.device("cuda:0")
    ops_res = [run_op("hidden", args.rows, 256, True, 0.5, True, args, dev),
               run_op("input", args.rows, 100, False, 0.0, False, args, dev)]
    out = {
        "device": torch.cuda.get_device_name(0),
        "method": dict(reps=args.reps, inner=args.inner, warmup=args.warmup, hbm_peak_bytes_per_s=HBM_PEAK,
                       note="device events around groups of calls; the variants alternating group by group; "
                            "medians and min-max over the groups; one run, one process"),
        "ops": ops_res,
        "model_step": run_model(args, dev),
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
