"""One GCNConv(normalize=True) layer, forward + backward, on two sampled
blocks of the project's synthetic graphs: the products [15, 10] batch-1024
block (100 -> 256 and 256 -> 47) and the arxiv one (128 -> 256, 256 -> 40),
against PyG's op sequence restated in torch on the device (the self-loop
rewrite, scatter_add_ degree, pow, two index_select, mul, the [E, F]
messages, index_add_, F.linear).

Variants, same process, same GPU; device events around groups of calls,
warm-up first, the variants alternating group by group, medians and the
min-max spread over the groups (bench_rewire.py's timed_groups):

  a_torch   the PyG sequence in torch, norm recomputed per call as PyG does
            (cached=False), library GEMM
  b_ngnn    ngnn.GCNConv(normalize=True): ngnn_gcn_norm + ngnn_gcn_wagg +
            the hand-written GEMM kernels; the block is built once (as the
            model wrappers do per mini-batch), the norm record per call
  c_ngnn_cached  the same with the block's cached norm record (every layer
            after the first of a forward)

Also recorded: kernel launches per call (torch.profiler, when it reports
device kernels), the aggregate kernel alone at the layer's aggregation width
(device events around groups of launches) with its fraction of the HBM peak
from the byte formula E (4F + 8 [+4 weighted]) + N (8F + 12), and each
variant's agreement with (a).

Writes one JSON file (default profiles/gcn_norm_bench.json) and prints it.
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

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from bench_consistency import count_kernels  # noqa: E402
from bench_rewire import timed_groups  # noqa: E402

HBM_PEAK = 8.0e12  # bytes / s


def torch_gcn(x, ei, W, b):
    """PyG 2.5.1 gcn_norm + GCNConv.forward, unweighted, add_self_loops."""
    N = x.size(0)
    src, dst = ei[0], ei[1]
    mask = src != dst
    ar = torch.arange(N, device=x.device)
    src, dst = torch.cat([src[mask], ar]), torch.cat([dst[mask], ar])
    w = torch.ones(src.numel(), device=x.device)
    deg = torch.zeros(N, device=x.device).scatter_add_(0, dst, w)
    dinv = deg.pow(-0.5)
    dinv.masked_fill_(dinv == float("inf"), 0)
    coef = dinv.index_select(0, src) * w * dinv.index_select(0, dst)
    z = F.linear(x, W)
    out = torch.zeros(N, W.size(0), device=x.device).index_add_(0, dst, z.index_select(0, src) * coef.unsqueeze(1))
    return out + b


def run_layer(name, batch, Fi, Fo, args, dev):
    import ngnn
    from ngnn import ops
    from ngnn.block import get_block
    ei, N = batch.edge_index, int(batch.num_nodes)
    E = int(ei.size(1))
    gen = torch.Generator().manual_seed(Fi + Fo)
    x = torch.randn(N, Fi, generator=gen).to(dev).requires_grad_(True)
    dout = torch.randn(N, Fo, generator=gen).to(dev)
    conv = ngnn.GCNConv(Fi, Fo, normalize=True).to(dev)
    with torch.no_grad():
        conv.bias.copy_(torch.randn(Fo, generator=gen) * 0.1)
    W, b = conv.lin.weight, conv.bias
    block = get_block(ei, N)

    def step(kind):
        x.grad = W.grad = b.grad = None
        if kind == "a":
            out = torch_gcn(x, ei, W, b)
        else:
            if kind == "b":
                block._gcn_norm.clear()
            out = conv(x, block)
        out.backward(dout)
        return out

    names = {"a": "a_torch", "b": "b_ngnn", "c": "c_ngnn_cached"}
    oa = step("a").detach().clone()
    ga = [t.grad.clone() for t in (x, W, b)]
    agree = {}
    for k in ("b", "c"):
        o = step(k).detach()
        agree[names[k]] = dict(
            out_err_over_max=float((o - oa).abs().max() / oa.abs().max()),
            **{n: float((t.grad - g).abs().max() / g.abs().max()) for n, t, g in zip(("dx", "dW", "db"), (x, W, b), ga)})
    fns = {names[k]: (lambda k=k: step(k)) for k in ("a", "b", "c")}
    res = timed_groups(fns, {k: args.inner for k in fns}, args.reps, args.warmup)
    # the aggregate kernel alone, at the width this layer aggregates at (F_in: aggregate-first)
    norm = ops.gcn_norm(block)
    xs = x.detach()
    agg = torch.empty(N, Fi, device=dev)
    res.update(timed_groups({"wagg_kernel": lambda: ops.wagg_fwd(xs, block, norm, None, out=agg)},
                            {"wagg_kernel": args.inner}, args.reps, args.warmup))
    res.update(timed_groups({"norm_kernel": lambda: (block._gcn_norm.clear(), ops.gcn_norm(block))},
                            {"norm_kernel": args.inner}, args.reps, args.warmup))
    nbytes = E * (4 * Fi + 8) + N * (8 * Fi + 12)
    t = res["wagg_kernel"]["median_ms"] * 1e-3
    us = {k: round(v["median_ms"] * 1e3, 2) for k, v in res.items()}
    return dict(
        layer=f"{Fi}->{Fo}", graph=name, N=N, E=E, aggregate_width=Fi,
        in_degree=dict(max=int(block.csr.degree().max()), median=float(block.csr.degree().float().median())),
        median_us_per_call=us,
        spread_us_min_max={k: [round(v["min_ms"] * 1e3, 2), round(v["max_ms"] * 1e3, 2)] for k, v in res.items()},
        torch_over_ngnn=us["a_torch"] / us["b_ngnn"],
        ngnn_faster_beyond_spread=bool(res["a_torch"]["min_ms"] > res["b_ngnn"]["max_ms"]),
        ngnn_slower_beyond_spread=bool(res["b_ngnn"]["min_ms"] > res["a_torch"]["max_ms"]),
        kernel_launches_per_call={names[k]: count_kernels(lambda k=k: step(k)) for k in ("a", "b", "c")},
        wagg=dict(algorithmic_bytes=nbytes, median_us=us["wagg_kernel"], bytes_per_s=nbytes / t,
                  fraction_of_hbm_peak=nbytes / t / HBM_PEAK),
        agreement_with_a=agree)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gcn_norm_bench.json"))
    ap.add_argument("--reps", type=int, default=15, help="groups per variant")
    ap.add_argument("--inner", type=int, default=20, help="calls (forward + backward) per group")
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_gcn_norm: needs the GPU (no fallback)")
    from ngnn.loader import sample_block, synthetic_graph
    dev = torch.device("cuda:0")
    layers = []
    for name, B, shapes in (("ogbn-products", 1024, ((100, 256), (256, 47))),
                            ("ogbn-arxiv", 1024, ((128, 256), (256, 40)))):
        print(f"bench_gcn_norm: {name}: building the graph", file=sys.stderr, flush=True)
        g = synthetic_graph(name, dev, seed=1)
        batch = sample_block(g, g.train_idx[:B], [15, 10], seed=3, gather_features=False)
        del g
        for Fi, Fo in shapes:
            print(f"bench_gcn_norm: {name} {Fi}->{Fo}", file=sys.stderr, flush=True)
            layers.append(run_layer(name, batch, Fi, Fo, args, dev))
    out = {
        "device": torch.cuda.get_device_name(0),
        "method": dict(reps=args.reps, inner=args.inner, warmup=args.warmup, hbm_peak_bytes_per_s=HBM_PEAK,
                       note="forward + backward of one layer per call, every row carrying a gradient; device "
                            "events around groups of calls; a, b, c alternating group by group; medians and "
                            "min-max over the groups; one run, one process; fanout [15, 10], 1024 seeds"),
        "layers": layers,
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(compact(out))
    print(json.dumps(out))


def compact(out) -> str:
    """The result with one line per field of a layer (a reviewable file)."""
    def fields(d, pad):
        return ",\n".join(f"{pad}{json.dumps(k)}: {json.dumps(v)}" for k, v in d.items())
    head = {k: v for k, v in out.items() if k != "layers"}
    layers = ",\n".join("  {\n" + fields(L, "   ") + "\n  }" for L in out["layers"])
    return "{\n" + fields(head, " ") + ',\n "layers": [\n' + layers + "\n ]\n}\n"


if __name__ == "__main__":
    main()
