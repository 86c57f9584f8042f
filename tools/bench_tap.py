"""The hidden-state tap at the ogbn-arxiv block of DESIGN section 5f: the
project's synthetic arxiv graph, fanout [10, 5], batch 512, layers
(128, 256, 256, 40), n_id from ngnn.loader.NeighborLoader.

  kernels  ngnn_dropout_rows and ngnn_tap_grad alone on the block's [n_sub, 256]
           hidden state, and on a 2^20-row tensor no cache holds, against their
           algorithmic bytes (2 N F 4 and 5 N F 4) as a share of the 8 TB/s
           HBM peak.  Time per call from device events around groups of calls
           (at the block's size that is mostly the launch, and says so).
  sageh    ngnn.SAGEH forward + backward of cross_entropy(out[:B]) + mean(h)
           against the torch composition: the per-conv path with relu and
           F.dropout as torch ops.
  sagepl   ngnn.SAGEPL forward + backward (the loss of tools/bench_sagepl.py)
           with fused_stack=True against fused_stack=False.

Device events around groups of calls, the variants alternating in one process,
warm-up first, medians over the groups.  `--part all` (the default) runs each
part as a fresh child process under a time limit of its own, stops at the first
that fails, and writes one JSON file (default profiles/tap_bench.json).  Needs
the GPU.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "noise-gnn_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

PEAK_BPS = 8e12  # HBM3E peak (spec)
PARTS = {"kernels": 240, "sageh": 300, "sagepl": 300}  # seconds each child may take
HID, LAYERS, B, FANOUT = 256, 3, 512, [10, 5]


def timed_groups(fns, reps, inner, warmup):
    """Median ms per call of each fn: groups of `inner` calls between two
    events, the fns alternating group by group, `reps` groups each."""
    import torch
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


def arxiv_block(args):
    import torch
    from ngnn.loader import NeighborLoader, synthetic_graph
    dev = torch.device("cuda:0")
    g = synthetic_graph("ogbn-arxiv", dev, seed=0, scale=args.scale)
    loader = NeighborLoader(g, g.train_idx, num_neighbors=FANOUT, batch_size=B, shuffle=True, seed=1)
    for i, b in enumerate(loader):  # (the pass runs to its end: the loader samples one batch ahead)
        if i == 0:
            batch = b
    return dev, g, batch


def part_kernels(args):
    import torch
    from ngnn import _lib
    dev, g, batch = arxiv_block(args)
    lib = _lib.load()
    res = {}
    for tag, n in (("block", batch.x.size(0)), ("rows_2e20", 1 << 20)):
        n = max(int(n * (args.scale if tag != "block" else 1.0)), 64)
        h = torch.randn(n, HID, device=dev).relu_()
        out, dy, dh = torch.empty_like(h), torch.randn_like(h), torch.randn_like(h)
        dz = torch.empty_like(h)
        st = _lib.stream_handle(dev)
        args5 = (_lib.ptr(h), HID, n, None, HID)

        def drop(p):
            return lambda: lib.ngnn_dropout_rows(*args5, p, 12345, None, _lib.ptr(out), HID, st)

        def grad(xd, a):
            return lambda: lib.ngnn_tap_grad(_lib.ptr(a), HID, _lib.ptr(xd), HID, 2.0, _lib.ptr(dh), HID,
                                             _lib.ptr(h), HID, n, None, HID, _lib.ptr(dz), HID, st)

        assert drop(0.5)() == 0 and grad(out, dy)() == 0
        t = timed_groups({"dropout_rows_bit": drop(0.5), "dropout_rows_byte": drop(0.3),
                          "tap_grad": grad(out, dy), "tap_grad_no_xd": grad(None, dy),
                          "torch_dropout": lambda: torch.nn.functional.dropout(h, 0.5, True)},
                         args.reps, args.inner, args.warmup)
        unit = n * HID * 4
        nbytes = dict(dropout_rows_bit=2 * unit, dropout_rows_byte=2 * unit, tap_grad=5 * unit,
                      tap_grad_no_xd=4 * unit, torch_dropout=2 * unit)
        for k, v in t.items():
            v["bytes"] = nbytes[k]
            v["share_of_8TBps"] = nbytes[k] / (v["median_ms"] * 1e-3) / PEAK_BPS
        res[tag] = dict(rows=n, F=HID, per_call=t)
    res["note"] = ("ms per call between device events over groups of back-to-back calls (launch included); "
                   "bytes are algorithmic: 2 N F 4 (read h, write xd) and 5 N F 4 (dy, xd, dh, h, dz)")
    return res


def _fwd_bwd(model, call, y, params):
    import torch.nn.functional as F

    def step():
        for q in params:
            q.grad = None
        out, h = call()
        (F.cross_entropy(out[:B], y, reduction="sum") + h.mean()).backward()
    return step


def part_sageh(args):
    import torch
    import ngnn
    from ngnn import models
    from ngnn.block import get_block
    dev, g, batch = arxiv_block(args)
    x, ei = batch.x, batch.edge_index
    y = g.y[batch.n_id[:B]]
    torch.manual_seed(0)
    m = ngnn.SAGEH(x.size(1), HID, g.num_classes, LAYERS, dropout=0.5).to(dev).train()
    params = list(m.convs.parameters())

    def composition():
        return models._tapped_composition(m.convs, x, get_block(ei, x.size(0)), m.dropout, True)

    # the two must agree before either is timed (no dropout: the masks differ)
    with torch.no_grad():
        a = m(x, ei, training=False)
        b = models._tapped_composition(m.convs, x, get_block(ei, x.size(0)), m.dropout, False)
    agree = dict(out_max_abs_diff=float((a[0] - b[0]).abs().max()), h_max_abs_diff=float((a[1] - b[1]).abs().max()))
    t = timed_groups({"tap": _fwd_bwd(m, lambda: m(x, ei), y, params),
                      "composition": _fwd_bwd(m, composition, y, params)},
                     args.reps, max(args.inner // 4, 1), args.warmup)
    return dict(fwd_bwd=t, agreement=agree,
                ratio_composition_over_tap=t["composition"]["median_ms"] / t["tap"]["median_ms"])


def part_sagepl(args):
    import torch
    import torch.nn.functional as F
    import ngnn
    dev, g, batch = arxiv_block(args)
    x, ei, n_id = batch.x, batch.edge_index, batch.n_id
    y = g.y[n_id[:B]]
    torch.manual_seed(0)
    base = ngnn.SAGEPL(x.size(1), HID, g.num_classes, LAYERS, nbr_nodes=g.num_nodes, dropout=0.5).to(dev).train()
    tap = ngnn.SAGEPL(x.size(1), HID, g.num_classes, LAYERS, nbr_nodes=g.num_nodes, dropout=0.5,
                      fused_stack=True).to(dev).train()
    tap.load_state_dict(base.state_dict())

    def step(model):
        def run():
            model.zero_grad(set_to_none=True)
            out = model(x, ei, noise_rate=0.1, n_id=n_id)
            (F.cross_entropy(out[2][:B], y, reduction="sum") + out[3].mean()).backward()
        return run

    base.eval(), tap.eval()
    with torch.no_grad():
        a, b = base(x, ei, noise_rate=0.1, n_id=n_id), tap(x, ei, noise_rate=0.1, n_id=n_id)
    agree = {f"out{i}_max_abs_diff": float((u - v).abs().max()) for i, (u, v) in enumerate(zip(a, b))}
    base.train(), tap.train()
    t = timed_groups({"fused_stack": step(tap), "per_conv": step(base)}, args.reps, max(args.inner // 4, 1),
                     args.warmup)
    return dict(fwd_bwd=t, agreement=agree,
                ratio_per_conv_over_fused_stack=t["per_conv"]["median_ms"] / t["fused_stack"]["median_ms"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tap_bench.json"))
    ap.add_argument("--part", default="all", choices=["all", *PARTS])
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--scale", type=float, default=1.0, help="shrink the graph (rehearsal)")
    args = ap.parse_args()
    if args.part != "all":
        import torch
        if not torch.cuda.is_available():
            sys.exit("bench_tap: needs the GPU (no fallback)")
        res = {"kernels": part_kernels, "sageh": part_sageh, "sagepl": part_sagepl}[args.part](args)
        res["device"] = torch.cuda.get_device_name(0)
        print(json.dumps(res))
        return
    out = {"shape": dict(graph="synthetic ogbn-arxiv", fanout=FANOUT, batch=B, layers=LAYERS, hidden=HID,
                         scale=args.scale),
           "method": dict(reps=args.reps, inner=args.inner, warmup=args.warmup,
                          note="device events around groups of calls, variants alternating; medians; "
                               "one child process per part")}
    for part, limit in PARTS.items():  # a fresh process per part, each under its own time limit
        cmd = [sys.executable, os.path.abspath(__file__), "--part", part, "--reps", str(args.reps), "--inner",
               str(args.inner), "--warmup", str(args.warmup), "--scale", str(args.scale)]
        try:
            r = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=limit, text=True)
        except subprocess.TimeoutExpired:
            sys.exit(f"bench_tap: part {part} passed its {limit} s limit; nothing further was started")
        if r.returncode != 0:
            sys.exit(f"bench_tap: part {part} ended with status {r.returncode}; nothing further was started")
        out[part] = json.loads(r.stdout.strip().splitlines()[-1])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
