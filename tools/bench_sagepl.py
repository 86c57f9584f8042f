"""SAGEPL's noise path at the ogbn-arxiv shape of the reference's
config_arxiv.yml: table 169,343 x 128, 3 layers, hidden 256, 40 classes,
fanout [10, 5], batch 512, on the project's synthetic arxiv graph with n_id
from ngnn.loader.NeighborLoader.

(a) ngnn.ops.add_node_noise forward + backward against the torch composition
    x + F.normalize(noise[n_id]) * rate forward + backward -- same process,
    same GPU, alternating, both paying the dense [N, F] gradient's zero fill.
(b) a full SAGEPL forward + backward of cross_entropy(z_pure[:B]) +
    mean(h_noisy), with the op and with the torch composition swapped in.

Device events around groups of calls, warm-up first, medians over the groups.
Kernel-only times (events around the launch alone, ngnn._timing) give the
achieved share of the 8 TB/s peak over the algorithmic bytes.  Writes one JSON
file (default profiles/sagepl_arxiv.json) and prints it.  Needs the GPU.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "noise-gnn_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

PEAK_BPS = 8e12  # HBM3E peak (spec)


def torch_noise(x, noise, n_id, rate):
    return x + F.normalize(noise[n_id]) * rate


def timed_groups(fns, reps, inner, warmup):
    """Median ms per call of each fn: groups of `inner` calls between two
    events, the fns alternating group by group, `reps` groups each."""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(inner):
                fn()
            e.record()
            e.synchronize()
            ms[k].append(s.elapsed_time(e) / inner)
    return {k: dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v)) for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sagepl_arxiv.json"))
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--scale", type=float, default=1.0, help="shrink the graph (rehearsal)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_sagepl: needs the GPU (no fallback)")
    import ngnn
    from ngnn import _timing
    from ngnn.loader import NeighborLoader, synthetic_graph
    from ngnn.ops import add_node_noise, node_noise_bad_ids

    dev = torch.device("cuda:0")
    g = synthetic_graph("ogbn-arxiv", dev, seed=0, scale=args.scale)
    N, Fw, B, rate = g.num_nodes, g.x.size(1), 512, 0.1
    loader = NeighborLoader(g, g.train_idx, num_neighbors=[10, 5], batch_size=B, shuffle=True, seed=1)
    for i, b in enumerate(loader):  # (the pass runs to its end: the loader samples one batch ahead)
        if i == 0:
            batch = b
    x, n_id, ei = batch.x, batch.n_id, batch.edge_index
    n_sub = x.size(0)
    torch.manual_seed(0)
    model = ngnn.SAGEPL(Fw, 256, g.num_classes, 3, nbr_nodes=N, dropout=0.5).to(dev).train()
    noise = model.noise
    G = torch.randn(n_sub, Fw, device=dev)
    y = g.y[n_id[:B]]

    # the two must agree before either is timed
    a = add_node_noise(x, noise, n_id, rate)
    b = torch_noise(x, noise, n_id, rate)
    ga, = torch.autograd.grad(a, noise, G)
    gb, = torch.autograd.grad(b, noise, G)
    a, b = a.detach(), b.detach()
    agree = dict(out_max_abs_diff=float((a - b).abs().max()), dnoise_max_abs_diff=float((ga - gb).abs().max()),
                 dnoise_max_abs=float(gb.abs().max()), bad_ids=node_noise_bad_ids(dev))
    del a, b, ga, gb

    def fb(fn):
        return lambda: torch.autograd.grad(fn(x, noise, n_id, rate), noise, G)

    res_a = timed_groups({"op_fwd": lambda: add_node_noise(x, noise, n_id, rate),
                          "torch_fwd": lambda: torch_noise(x, noise, n_id, rate),
                          "op_fwd_bwd": fb(add_node_noise), "torch_fwd_bwd": fb(torch_noise),
                          "table_zero_fill": lambda: torch.zeros(N, Fw, device=dev)},
                         args.reps, args.inner, args.warmup)

    # kernel-only: events around each launch
    with _timing.KernelTimer(only={"node_noise_fwd", "node_noise_bwd"}) as kt:
        for _ in range(50):
            torch.autograd.grad(add_node_noise(x, noise, n_id, rate), noise, G)
        torch.cuda.synchronize()
    per = {}
    for r in kt.recs:
        per.setdefault(r.name, []).append(r.start.elapsed_time(r.end))
    row_bytes = n_sub * Fw * 4
    alg = {"fwd_bytes": 3 * row_bytes, "bwd_read_bytes": 2 * row_bytes, "bwd_atomic_bytes": row_bytes,
           "table_zero_fill_bytes": N * Fw * 4}
    kern = {}
    for name, nbytes in (("node_noise_fwd", alg["fwd_bytes"]),
                         ("node_noise_bwd", alg["bwd_read_bytes"] + alg["bwd_atomic_bytes"])):
        ms = statistics.median(per[name][10:])
        kern[name] = dict(median_ms=ms, bytes=nbytes, achieved_Bps=nbytes / (ms * 1e-3),
                          share_of_8TBps=nbytes / (ms * 1e-3) / PEAK_BPS)
    zf = res_a["table_zero_fill"]["median_ms"]
    kern["table_zero_fill"] = dict(median_ms=zf, bytes=alg["table_zero_fill_bytes"],
                                   share_of_8TBps=alg["table_zero_fill_bytes"] / (zf * 1e-3) / PEAK_BPS)

    # (b) the whole model, the op against the torch composition swapped in
    def step():
        model.zero_grad(set_to_none=True)
        out = model(x, ei, noise_rate=rate, n_id=n_id)
        (F.cross_entropy(out[2][:B], y, reduction="sum") + out[3].mean()).backward()

    def step_torch():
        model.adding_noise = lambda xx, noise_rate, n_id=None: torch_noise(xx, model.noise, n_id, noise_rate)
        try:
            step()
        finally:
            del model.adding_noise

    res_b = timed_groups({"model_op": step, "model_torch": step_torch}, args.reps, max(args.inner // 4, 1),
                         args.warmup)

    out = {
        "device": torch.cuda.get_device_name(0),
        "shape": dict(table_rows=N, F=Fw, n_sub=n_sub, edges=int(ei.size(1)), batch=B, fanout=[10, 5], layers=3,
                      hidden=256, classes=g.num_classes, scale=args.scale),
        "method": dict(reps=args.reps, inner=args.inner, warmup=args.warmup,
                       note="device events around groups of `inner` calls, variants alternating; medians"),
        "agreement": agree,
        "a_noise_op": res_a,
        "a_ratio_torch_over_op_fwd_bwd": res_a["torch_fwd_bwd"]["median_ms"] / res_a["op_fwd_bwd"]["median_ms"],
        "a_ratio_torch_over_op_fwd": res_a["torch_fwd"]["median_ms"] / res_a["op_fwd"]["median_ms"],
        "a_algorithmic_bytes": alg,
        "a_kernels": kern,
        "b_model_fwd_bwd": res_b,
        "b_ratio_torch_over_op": res_b["model_torch"]["median_ms"] / res_b["model_op"]["median_ms"],
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
