"""flip_label at the datasets' shapes, against what a user has without it.

Shapes: ogbn-products (N = 2,449,029 labels, C = 47) and ogbn-arxiv
(N = 169,343, C = 40), `sym` noise at rate 0.3, uniform random clean labels.

  kernel_stats / kernel_labels_only
                   ngnn_flip_labels alone, called at the C ABI on prepared
                   buffers with / without noise_or_not and counts: device
                   events around 100 launches after a warm-up
  flip_label       the whole Python call ngnn.noise.flip_label(y, C, 'sym',
                   0.3, seed=k): matrix, cached table, output allocation,
                   launch
  torch_multinomial
                   what a user would write on the device without it:
                   torch.multinomial(M_dev[y], 1) -- a gathered [N, C] float
                   matrix and one draw per row
  reference_loop   the reference's per-node loop (noise.py:54-58: .item(),
                   np.random.multinomial, np.where per node) restated, on the
                   HOST CPU over 100,000 nodes; a host number, reported per
                   node and scaled to N as an estimate

flip_label and torch_multinomial run in the same process in five alternating
pairs, each a group of calls between a host clock start and a device
synchronise (the whole call, host work included); `flip_label_won` says for
each pair whether flip_label was the faster.  Bytes per call: 17 N (label in,
label out, noise_or_not) plus the table; the share of HBM is those bytes over
the kernel's time against the 8 TB/s peak -- at these sizes the call may be
bound by the launch, not by bytes.

Writes one JSON file (default profiles/label_noise_bench.json) and prints it.
Needs the GPU.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "noise-gnn_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

HBM_PEAK = 8.0e12  # bytes / s
SHAPES = (("ogbn-products", 2_449_029, 47), ("ogbn-arxiv", 169_343, 40))
PAIRS = 5
LAUNCHES = 100


def kernel_ms(y, C, tab, stats, warmup):
    """ms per launch of ngnn_flip_labels alone: events around LAUNCHES launches."""
    from ngnn import _lib
    lib, N, dev = _lib.load(), y.numel(), y.device
    out = torch.empty_like(y)
    clean = torch.empty(N, dtype=torch.bool, device=dev) if stats else None
    counts = torch.zeros(C, C, dtype=torch.int64, device=dev) if stats else None
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    st = _lib.stream_handle(dev)

    def launch(seed):
        _lib.check(lib.ngnn_flip_labels(_lib.ptr(y), N, C, tab.data_ptr(), tab.data_ptr() + 4 * C * C, seed, 0,
                                        _lib.ptr(out), _lib.ptr(clean), _lib.ptr(counts), _lib.ptr(bad), st),
                   "ngnn_flip_labels")

    for k in range(warmup):
        launch(k)
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for k in range(LAUNCHES):
        launch(1000 + k)
    e.record()
    e.synchronize()
    if stats:
        assert int(counts.sum()) == (warmup + LAUNCHES) * N and int(bad) == 0
    return s.elapsed_time(e) / LAUNCHES


def host_clocked(fn, inner):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k in range(inner):
        fn(k)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / inner * 1e3


def reference_loop_us_per_node(C, n, prob=0.3):
    """The reference's loop over the nodes, restated, on the host."""
    from ngnn.noise import noise_matrix
    M = noise_matrix(C, "sym", prob)
    labels = torch.from_numpy(np.random.RandomState(5).randint(0, C, n))
    noisy = np.copy(labels.numpy())
    np.random.seed(0)
    t0 = time.perf_counter()
    for i in range(n):
        lbl = labels[i].item()
        flipped = np.random.multinomial(1, M[lbl, :], 1)[0]
        noisy[i] = np.where(flipped == 1)[0][0]
    dt = time.perf_counter() - t0
    assert abs(float((noisy == labels.numpy()).mean()) - (1 - prob)) < 0.02
    return dt / n * 1e6


def run_shape(name, N, C, args, dev, loop_us):
    from ngnn.noise import _device_table, flip_label, noise_matrix
    gen = torch.Generator(device=dev).manual_seed(5)
    y = torch.randint(0, C, (N,), device=dev, generator=gen)
    M = noise_matrix(C, "sym", 0.3)
    tab = _device_table(M, dev)
    M_dev = torch.from_numpy(M).to(dev, torch.float32)
    nbytes = 17 * N + 4 * C * (C + 1)

    k_stats = kernel_ms(y, C, tab, True, args.warmup)
    k_plain = kernel_ms(y, C, tab, False, args.warmup)

    fns = {"flip_label": (lambda k: flip_label(y, C, "sym", 0.3, seed=k), args.inner),
           "flip_label_stats": (lambda k: flip_label(y, C, "sym", 0.3, seed=k, return_stats=True), args.inner),
           "torch_multinomial": (lambda k: torch.multinomial(M_dev[y], 1), max(args.inner // 4, 1))}
    for fn, _ in fns.values():
        for k in range(3):
            fn(k)
    pairs = []
    for _ in range(PAIRS):
        pairs.append({k: host_clocked(fn, inner) for k, (fn, inner) in fns.items()})
    # the composition draws from the same rows: its kept-label rate is the matrix's diagonal too
    kept = float((torch.multinomial(M_dev[y], 1)[:, 0] == y).float().mean())
    kept_ngnn = float((flip_label(y, C, "sym", 0.3, seed=1)[0] == y).float().mean())
    med = {k: statistics.median(p[k] for p in pairs) for k in fns}
    return dict(
        dataset=name, N=N, C=C, noise_type="sym", prob=0.3,
        kernel_ms=dict(with_stats=k_stats, labels_only=k_plain, launches=LAUNCHES),
        pairs_ms=pairs, median_ms=med,
        flip_label_won=[p["flip_label"] < p["torch_multinomial"] for p in pairs],
        flip_label_stats_won=[p["flip_label_stats"] < p["torch_multinomial"] for p in pairs],
        bytes_per_call=nbytes, composition_gathered_bytes=4 * N * C,
        kernel_fraction_of_hbm_peak=dict(with_stats=nbytes / (k_stats * 1e-3) / HBM_PEAK,
                                         labels_only=(16 * N + 4 * C * (C + 1)) / (k_plain * 1e-3) / HBM_PEAK),
        kept_label_rate=dict(flip_label=kept_ngnn, torch_multinomial=kept),
        reference_loop_host_cpu=dict(us_per_node=loop_us, estimate_s_for_N=loop_us * N * 1e-6,
                                     note="measured on the host CPU, not on the GPU"),
        ratios=dict(torch_multinomial_over_flip_label=med["torch_multinomial"] / med["flip_label"],
                    reference_loop_estimate_over_flip_label=loop_us * N * 1e-3 / med["flip_label"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "label_noise_bench.json"))
    ap.add_argument("--inner", type=int, default=20, help="calls per group of a pair")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--loop-nodes", type=int, default=100_000, help="nodes of the host loop")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_label_noise: needs the GPU (no fallback)")
    dev = torch.device("cuda:0")
    loop_us = reference_loop_us_per_node(47, args.loop_nodes)
    out = {
        "device": torch.cuda.get_device_name(0),
        "method": dict(pairs=PAIRS, inner=args.inner, warmup=args.warmup, launches=LAUNCHES, loop_nodes=args.loop_nodes,
                       note="kernel_ms: device events around 100 launches at the C ABI; pairs_ms: ms per whole "
                            "call, host clock around a group of calls ending in a synchronise, the variants "
                            "alternating; reference_loop_host_cpu: one host-clocked run of the restated loop"),
        "shapes": [run_shape(name, N, C, args, dev, loop_us) for name, N, C in SHAPES],
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
