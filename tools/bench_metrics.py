"""ngnn.metrics at the products shapes, against what a user has without it.

1. epoch: one ogbn-products [15, 10] batch-1024 epoch of GraphedTrainStep on
   the sync-free NeighborLoader (193 steps), taken three ways in one process,
   the variants alternating over ROUNDS rounds, each epoch between a host
   clock start and a device synchronise:
     plain       the steps alone, nothing reported
     meter       + EpochMeter.update(step.out, batch.y, step.loss) per step
                 and one result() at the end
     host_reads  + the reference's per-step lines (pipeline.py:164-165):
                 total_loss += float(loss);
                 total_correct += int(out.argmax(dim=-1).eq(y).sum())
   One more epoch, untimed, runs meter and host_reads together and checks
   that they report the same counts and the same loss sum.

2. split: split_accuracy at N = 2,449,029, C = 47 with the products split
   sizes 196,615 / 39,323 / 2,213,091 (a random partition of the nodes):
     kernel        ngnn_split_accuracy alone at the C ABI, device events
                   around LAUNCHES launches
     fused         the whole Python call (list cached, one launch, one host
                   copy of the counts)
     torch_device  the same three accuracies from torch ops on the device:
                   argmax, three index gathers, eq, sum, .item()
     host_lines    the lines as written on the HOST (pipeline.py:182-195:
                   the logits copied to the CPU, argmax and the three
                   compares there); one run, a host number
   Bytes read by the kernel: M (4 C + 16) (a logits row, the id and the
   label per entry); the share of HBM is those bytes over the kernel's time
   against the 8 TB/s peak.

Writes one JSON file (default profiles/metrics_bench.json) and prints it.
Needs the GPU.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "noise-gnn_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

HBM_PEAK = 8.0e12  # bytes / s
N_PRODUCTS, C_PRODUCTS = 2_449_029, 47
SPLIT_SIZES = (("train", 196_615), ("valid", 39_323), ("test", 2_213_091))
LAUNCHES = 20


def bench_epoch(args, dev):
    import ngnn
    from ngnn.graphs import GraphedTrainStep, slot_size
    from ngnn.loader import DATASETS, NeighborLoader, synthetic_graph
    from ngnn.metrics import EpochMeter
    from ngnn.optim import Adam
    fanout, B = [15, 10], 1024
    _, _, F_in, C, _ = DATASETS["ogbn-products"]
    graph = synthetic_graph("ogbn-products", dev, seed=0)
    torch.manual_seed(1234)
    model = ngnn.SAGE(F_in, 256, C, 2, dropout=0.5).to(dev).train()
    opt = Adam(model.parameters(), lr=1e-3)
    b0 = next(iter(NeighborLoader(graph, graph.train_idx, fanout, B, shuffle=True, seed=7)))
    n_cap, e_cap = slot_size(B, fanout)
    step = GraphedTrainStep(model, opt, B, n_cap, e_cap, b0.x.size(1), dev)
    step.capture(b0.x, b0.edge_index, b0.y)
    del b0
    loader = NeighborLoader(graph, graph.train_idx, fanout, B, shuffle=True, seed=7, sync_free=True)
    meter = EpochMeter(dev, names=("loss",))
    n_train = int(graph.train_idx.numel())

    def plain():
        for b in loader:
            step(b.x, b.edge_index, b.y, b.batch_size)
        return None

    def with_meter():
        meter.reset()
        for b in loader:
            step(b.x, b.edge_index, b.y, b.batch_size)
            meter.update(step.out, b.y, step.loss, batch_size=b.batch_size)
        r = meter.result()
        return r["means"]["loss"], r["correct"] / n_train

    def host_reads():
        total_loss = total_correct = 0
        for b in loader:
            loss = step(b.x, b.edge_index, b.y, b.batch_size)
            bs = b.batch_size
            total_loss += float(loss)
            total_correct += int(step.out[:bs].argmax(dim=-1).eq(b.y[:bs].view(-1)).sum())
        return total_loss / len(loader), total_correct / n_train

    def both():  # (untimed) the two reports of one and the same epoch
        meter.reset()
        total_loss = total_correct = 0
        for b in loader:
            loss = step(b.x, b.edge_index, b.y, b.batch_size)
            bs = b.batch_size
            meter.update(step.out, b.y, loss, batch_size=bs)
            total_loss += float(loss)
            total_correct += int(step.out[:bs].argmax(dim=-1).eq(b.y[:bs].view(-1)).sum())
        r = meter.result()
        return dict(steps=r["steps"], rows=r["rows"], correct_meter=r["correct"], correct_host=total_correct,
                    loss_sum_meter=r["sums"]["loss"], loss_sum_host=total_loss,
                    equal=bool(r["correct"] == total_correct and r["sums"]["loss"] == total_loss
                               and r["steps"] == len(loader) and r["rows"] == n_train))

    variants = {"plain": plain, "meter": with_meter, "host_reads": host_reads}

    def clocked(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    for fn in variants.values():  # warm-up: one epoch each
        fn()
    rounds = [{k: clocked(fn) for k, fn in variants.items()} for _ in range(args.rounds)]
    agree = both()
    step.check_inputs()
    med = {k: statistics.median(r[k] for r in rounds) for k in variants}
    steps = len(loader)
    return dict(dataset="ogbn-products (synthetic)", fanout=fanout, batch_size=B, steps_per_epoch=steps,
                rounds_ms=rounds, median_epoch_ms=med,
                median_ms_per_step={k: v / steps for k, v in med.items()},
                meter_cost_us_per_step=(med["meter"] - med["plain"]) / steps * 1e3,
                host_reads_cost_us_per_step=(med["host_reads"] - med["plain"]) / steps * 1e3,
                meter_won=[r["meter"] < r["host_reads"] for r in rounds],
                same_epoch_two_reports=agree)


def bench_split(args, dev):
    from ngnn import _lib
    from ngnn.metrics import split_accuracy
    N, C = N_PRODUCTS, C_PRODUCTS
    gen = torch.Generator(device=dev).manual_seed(5)
    out = torch.randn(N, C, device=dev, generator=gen)
    y = torch.randint(0, C, (N,), device=dev, generator=gen)
    hit = torch.rand(N, device=dev, generator=gen) < 0.7  # (a trained model's ~70 %)
    y = torch.where(hit, out.argmax(dim=-1), y)
    perm = torch.randperm(N, device=dev, generator=gen)
    split, at = {}, 0
    for name, n in SPLIT_SIZES:
        split[name] = perm[at:at + n].contiguous()
        at += n
    M = at
    nbytes = M * (4 * C + 16)

    def fused():
        return split_accuracy(out, y, split)

    def torch_device():
        y_pred = out.argmax(dim=-1, keepdim=True)
        yy = y.view(-1, 1)
        return {k: (y_pred[idx] == yy[idx]).sum().item() / idx.numel() for k, idx in split.items()}

    def host_lines():
        o = out.cpu()
        y_pred = o.argmax(dim=-1, keepdim=True)
        yy, sp = y.cpu().view(-1, 1), {k: v.cpu() for k, v in split.items()}
        return {k: float((y_pred[idx] == yy[idx]).sum()) / idx.numel() for k, idx in sp.items()}

    a, b = fused(), torch_device()
    assert a == b, (a, b)

    # the kernel alone
    lib = _lib.load()
    rows = torch.cat(list(split.values()))
    bounds = (ctypes.c_int64 * 4)(0, SPLIT_SIZES[0][1], SPLIT_SIZES[0][1] + SPLIT_SIZES[1][1], M)
    counts = torch.empty(3, 4, dtype=torch.int64, device=dev)
    st = _lib.stream_handle(dev)

    def kernel_ms(rows_t, conf):
        def launch():
            _lib.check(lib.ngnn_split_accuracy(out.data_ptr(), C, _lib.F32, N, C, y.data_ptr(), -100,
                                               _lib.ptr(rows_t), M, 3, bounds, counts.data_ptr(), None,
                                               _lib.ptr(conf), st), "ngnn_split_accuracy")
        for _ in range(3):
            launch()
        torch.cuda.synchronize()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(LAUNCHES):
            launch()
        e.record()
        e.synchronize()
        return s.elapsed_time(e) / LAUNCHES

    k_list = kernel_ms(rows, None)
    k_seq = kernel_ms(None, None)  # rows = NULL: every node in order (a contiguous read of the logits)
    k_conf = kernel_ms(rows, torch.empty(C, C, dtype=torch.int64, device=dev))

    def clocked(fn, inner):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(inner):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / inner * 1e3

    fns = {"fused": (fused, args.inner), "torch_device": (torch_device, args.inner)}
    for fn, _ in fns.values():
        fn()
    pairs = [{k: clocked(fn, inner) for k, (fn, inner) in fns.items()} for _ in range(args.rounds)]
    med = {k: statistics.median(p[k] for p in pairs) for k in fns}
    t0 = time.perf_counter()
    h = host_lines()
    host_ms = (time.perf_counter() - t0) * 1e3
    assert h == a, (h, a)
    return dict(N=N, C=C, M=M, split_sizes=dict(SPLIT_SIZES), accuracies=a,
                kernel_ms=dict(permuted_list=k_list, rows_null_in_order=k_seq, permuted_list_with_confusion=k_conf,
                               launches=LAUNCHES),
                bytes_per_call=nbytes, ideal_us_at_hbm_peak=nbytes / HBM_PEAK * 1e6,
                kernel_fraction_of_hbm_peak=dict(permuted_list=nbytes / (k_list * 1e-3) / HBM_PEAK,
                                                 rows_null_in_order=M * (4 * C + 8) / (k_seq * 1e-3) / HBM_PEAK),
                pairs_ms=pairs, median_ms=med, fused_won=[p["fused"] < p["torch_device"] for p in pairs],
                host_lines_ms=host_ms, host_lines_note="one run; the 460 MB logits copied to the host CPU, "
                                                       "argmax and compares there: a host number",
                ratios=dict(torch_device_over_fused=med["torch_device"] / med["fused"],
                            host_lines_over_fused=host_ms / med["fused"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "metrics_bench.json"))
    ap.add_argument("--rounds", type=int, default=5, help="alternating rounds of each comparison")
    ap.add_argument("--inner", type=int, default=10, help="split_accuracy calls per group of a pair")
    ap.add_argument("--only", choices=("epoch", "split"), default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_metrics: needs the GPU (no fallback)")
    dev = torch.device("cuda:0")
    out = {"device": torch.cuda.get_device_name(0),
           "method": dict(rounds=args.rounds, inner=args.inner, launches=LAUNCHES,
                          note="epoch: ms per whole epoch, host clock from the first enqueue to a device "
                               "synchronise, the three variants alternating; split kernel_ms: device events "
                               "around 20 launches at the C ABI; split pairs_ms: ms per whole call, host clock "
                               "around a group of calls ending in a synchronise, the variants alternating")}
    if args.only != "split":
        out["epoch"] = bench_epoch(args, dev)
    if args.only != "epoch":
        out["split"] = bench_split(args, dev)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
