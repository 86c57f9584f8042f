"""topk_rewire at the block shape of the reference's config_arxiv.yml /
config_test.yml (fanout [10, 5], batch 512, hidden 256: about 21.6 k nodes,
60 k edges, k_percent 0.2), on a synthetic ReLU'd hidden state.

(a) ngnn.ops.topk_rewire against the reference's op sequence restated with
    every tensor created on the device (dense similarity matrix, dense masks,
    four torch.topk over N*N keys, two torch.nonzero) -- the strongest version
    of what a user has without the op.  Same process, same GPU, alternating;
    device events around groups of calls, warm-up first, medians over the
    groups.
(b) the two outputs under the admissibility rule of tests/rewire_ref.py,
    restated here with device tensors in fp64 (N*N does not fit the rule's CPU
    form at this size): every selection of the op holds all decided-in and no
    decided-out entries, its edge lists follow from its selections exactly,
    and the composition's edge lists differ from them only in undecided
    entries.
(c) workspace bytes against the composition's peak allocation.
(d) per-kernel times of the two dense passes against the fp32 GEMM roof, from
    a rocprofv3 kernel_stats.csv of `bench_rewire.py --driver` given with
    --kernel-stats (counters and timing never share a run).

Writes one JSON file (default profiles/rewire_arxiv.json) and prints it.
Needs the GPU.
"""
from __future__ import annotations

import argparse
import csv
import glob
import json
import os
import re
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "noise-gnn_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

GEMM_UNTUNED_FLOPS = 122e12  # what an untuned 4096^3 GEMM on the exact-fp32 MFMA reaches on an MI355X
MFMA_F32_PEAK_FLOPS = 155e12


def make_inputs(n, f, e, dev, seed=0):
    """A ReLU'd hidden state with some low-rank structure (similarities spread
    over (0, 1) as after a trained layer) and e random edges."""
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(n, 24, generator=g)
    w = torch.randn(24, f, generator=g) / 24 ** 0.5
    h = torch.relu(z @ w + 0.7 * torch.randn(n, f, generator=g))
    ei = torch.randint(0, n, (2, e), generator=g)
    return h.to(dev), ei.to(dev)


def dense_rewire(h, edge_index, k_percent):
    """src/utils/augmentation.py:36-86 as it stands, every tensor on h's device."""
    dev = h.device
    n = h.size(0)
    k = int(n * k_percent)
    sim = F.normalize(h, dim=1)
    sim = torch.mm(sim, sim.t())
    eye = torch.eye(n, device=dev)
    adj = torch.zeros((n, n), device=dev)
    adj[edge_index[0], edge_index[1]] = 1
    adj_pot = adj - eye
    adj_pot[adj_pot <= 0] = 1000
    _, idx = torch.topk(torch.mul(sim, adj_pot).view(-1), k=2 * k, largest=False)
    mask = torch.ones((n, n), device=dev)
    mask.view(-1)[idx] = 0
    adj_removed = adj * mask
    _, idx = torch.topk((sim - adj_removed * 100 - eye * 100).view(-1), k=2 * k)
    add = torch.zeros((n, n), device=dev)
    add.view(-1)[idx] = 1
    pos_adj = adj_removed + add
    adj_pot = torch.zeros((n, n), device=dev)
    adj_pot[edge_index[0], edge_index[1]] = 1
    adj_pot = adj_pot - eye * 1000
    _, idx = torch.topk(torch.mul(sim, adj_pot).view(-1), k=2 * k)
    mask = torch.ones((n, n), device=dev)
    mask.view(-1)[idx] = 0
    adj_removed = adj * mask
    adj_pot = torch.ones((n, n), device=dev)
    adj_pot[edge_index[0], edge_index[1]] = 1000
    adj_pot = adj_pot + eye * 1000
    _, idx = torch.topk(torch.mul(sim, adj_pot).view(-1), k=2 * k, largest=False)
    add = torch.zeros((n, n), device=dev)
    add.view(-1)[idx] = 1
    neg_adj = adj_removed + add
    return torch.stack(torch.nonzero(pos_adj, as_tuple=True)), torch.stack(torch.nonzero(neg_adj, as_tuple=True))


def rule_on_device(h, ei, k2, pos, neg, sel, dpos, dneg):
    """tests/rewire_ref.check_result with device tensors (fp64 keys over N*N),
    plus the composition's edge lists against the op's."""
    n = h.size(0)
    dev = h.device
    hn = F.normalize(h.double(), dim=1)
    s64 = hn @ hn.t()
    hn = F.normalize(h, dim=1)
    delta = 4.0 * float(((hn @ hn.t()).double() - s64).abs().max())
    a = torch.zeros(n, n, dtype=torch.bool, device=dev)
    a[ei[0], ei[1]] = True
    d = torch.eye(n, dtype=torch.bool, device=dev)
    largest = (False, True, True, False)
    rep = {"delta": delta, "undecided": [], "violations": 0}
    und_idx = []
    for w in range(4):
        if w == 0:
            mult = torch.where(a & ~d, 1.0, 1000.0).double()
        elif w == 2:
            mult = a.double() - 1000.0 * d.double()
        elif w == 3:
            mult = torch.where(a, 1000.0, 1.0).double() + 1000.0 * d.double()
        if w == 1:
            kept = a.clone().view(-1)
            kept[sel[0]] = False
            key = (s64 - 100.0 * kept.view(n, n).double() - 100.0 * d.double()).view(-1)
            mult = torch.ones(1, dtype=torch.float64, device=dev)
        else:
            key = (s64 * mult).view(-1) + 0.0
        t = torch.topk(key, k2, largest=largest[w]).values[-1]
        und = (key - t).abs() <= delta * mult.abs().expand(n, n).reshape(-1)
        better = (key > t) if largest[w] else (key < t)
        chosen = torch.zeros(n * n, dtype=torch.bool, device=dev)
        chosen[sel[w]] = True
        bad = int((better & ~und & ~chosen).sum()) + int((~better & ~und & chosen).sum())
        bad += int(torch.unique(sel[w]).numel() != k2)
        rep["violations"] += bad
        rep["undecided"].append(int(und.sum()))
        und_idx.append(torch.nonzero(und).flatten())
        del key, und, better, chosen
    rep["outputs_follow_from_selections"] = True
    for name, got, rem, add, dense, free in (("pos", pos, sel[0], sel[1], dpos, torch.cat(und_idx[:2])),
                                             ("neg", neg, sel[2], sel[3], dneg, torch.cat(und_idx[2:]))):
        m = a.clone().view(-1)
        m[rem] = False
        m[add] = True
        want = torch.stack(torch.nonzero(m.view(n, n), as_tuple=True))
        if want.shape != got.shape or not torch.equal(want, got):
            rep["outputs_follow_from_selections"] = False
        fa, fb = got[0] * n + got[1], dense[0] * n + dense[1]
        both = torch.cat([fa, fb])
        u, c = torch.unique(both, return_counts=True)
        diff = u[c == 1]
        rep[name + "_entries"] = int(got.size(1))
        rep[name + "_dense_entries"] = int(dense.size(1))
        rep[name + "_differ_from_dense"] = int(diff.numel())
        rep[name + "_differ_outside_undecided"] = int((~torch.isin(diff, free)).sum())
    rep["pass"] = (rep["violations"] == 0 and rep["outputs_follow_from_selections"]
                   and rep["pos_differ_outside_undecided"] == 0 and rep["neg_differ_outside_undecided"] == 0)
    return rep


def timed_groups(fns, inner, reps, warmup):
    """Median ms per call of each fn: groups of inner[k] calls between two
    device events, the fns alternating group by group, `reps` groups each."""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(inner[k]):
                fn()
            e.record()
            e.synchronize()
            ms[k].append(s.elapsed_time(e) / inner[k])
    return {k: dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v), groups=len(v), inner=inner[k])
            for k, v in ms.items()}


def kernel_stats(path, n, f):
    """The op's kernels from a rocprofv3 kernel_stats.csv (a file or a directory holding one)."""
    if os.path.isdir(path):
        path = glob.glob(os.path.join(path, "**", "*kernel_stats.csv"), recursive=True)[0]
    pat = re.compile(r"ngnn::(?:\(anonymous namespace\)::)?(\w+(?:<[^()]*>)?)")
    # what a pass executes: the 128 x 128 tiles (I, J) with I <= J, K padded to 16
    nt = -(-n // 128)
    flop = 2.0 * (nt * (nt + 1) // 2) * 128 * 128 * (-(-f // 16) * 16)
    out = {"gemm_flop_per_pass": flop, "full_n_by_n_flop": 2.0 * n * n * f, "roof_ms_untuned_gemm_122TF": flop / GEMM_UNTUNED_FLOPS * 1e3,
           "roof_ms_mfma_peak_155TF": flop / MFMA_F32_PEAK_FLOPS * 1e3, "us_per_op_call": {}}
    rows = list(csv.DictReader(open(path)))
    # op calls in the profiled run: the histogram pass runs once per call
    calls = next(int(r["Calls"]) for r in rows if "k_dense<0>" in r["Name"])
    per = out["us_per_op_call"]
    for r in rows:
        tot = float(r["TotalDurationNs"]) / 1e3 / calls
        m = pat.search(r["Name"])
        if m:
            per[m.group(1)] = per.get(m.group(1), 0.0) + tot
        elif "rocprim" in r["Name"]:
            per["rocprim radix sorts (all kernels)"] = per.get("rocprim radix sorts (all kernels)", 0.0) + tot
        elif "fillBuffer" in r["Name"]:
            per["fills (the op's and rocprim's)"] = per.get("fills (the op's and rocprim's)", 0.0) + tot
    out["sum_us_per_op_call"] = sum(per.values())
    out["dense_passes"] = {}
    for name, label in (("k_dense<0>", "histogram"), ("k_dense<2>", "emit")):
        ms = per[name] * 1e-3
        out["dense_passes"][label] = dict(ms=ms, achieved_TFLOPS=flop / (ms * 1e-3) / 1e12,
                                          times_the_122TF_roof=ms / out["roof_ms_untuned_gemm_122TF"],
                                          share_of_155TF_peak=flop / (ms * 1e-3) / MFMA_F32_PEAK_FLOPS)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rewire_arxiv.json"))
    ap.add_argument("--n", type=int, default=21600)
    ap.add_argument("--f", type=int, default=256)
    ap.add_argument("--e", type=int, default=60000)
    ap.add_argument("--k-percent", type=float, default=0.2)
    ap.add_argument("--reps", type=int, default=12, help="groups per variant")
    ap.add_argument("--inner", type=int, default=4, help="op calls per group (the composition: 1)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--driver", action="store_true", help="only run the op 12 times (under a profiler)")
    ap.add_argument("--kernel-stats", default=None, help="rocprofv3 kernel_stats.csv (or its directory) of --driver")
    ap.add_argument("--no-dense", action="store_true", help="skip the composition and the rule (rehearsal)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_rewire: needs the GPU (no fallback)")
    from ngnn import _lib
    from ngnn.ops import rewire_bad_endpoints, topk_rewire

    dev = torch.device("cuda:0")
    n, f, e, kp = args.n, args.f, args.e, args.k_percent
    h, ei = make_inputs(n, f, e, dev)
    k2 = 2 * int(n * kp)
    if args.driver:
        for _ in range(12):
            topk_rewire(h, ei, dev, kp)
        torch.cuda.synchronize()
        return

    pos, neg, sel = topk_rewire(h, ei, dev, kp, return_selections=True)
    p2, n2, s2 = topk_rewire(h, ei, dev, kp, return_selections=True)
    out = {
        "device": torch.cuda.get_device_name(0),
        "shape": dict(N=n, F=f, E=e, k_percent=kp, k2=k2),
        "method": dict(reps=args.reps, inner_op=args.inner, inner_dense=1, warmup=args.warmup,
                       note="device events around groups of calls, variants alternating; medians over the groups"),
        "bitwise_repeatable": bool(torch.equal(pos, p2) and torch.equal(neg, n2) and torch.equal(sel, s2)),
        "bad_endpoints": rewire_bad_endpoints(dev),
    }
    ws = int(_lib.load().ngnn_topk_rewire_workspace_bytes(n, f, e, k2))
    out["memory"] = dict(op_workspace_bytes=ws, op_output_capacity_bytes=2 * 2 * (e + k2) * 8,
                         one_dense_fp32_matrix_bytes=n * n * 4)
    fns = {"op": lambda: topk_rewire(h, ei, dev, kp)}
    inner = {"op": args.inner}
    if not args.no_dense:
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        dpos, dneg = dense_rewire(h, ei, kp)
        torch.cuda.synchronize()
        out["memory"]["dense_composition_peak_bytes"] = int(torch.cuda.max_memory_allocated() - base)
        out["memory"]["dense_peak_over_op_workspace"] = out["memory"]["dense_composition_peak_bytes"] / ws
        out["agreement"] = rule_on_device(h, ei, k2, pos, neg, sel, dpos, dneg)
        del dpos, dneg
        fns["dense_on_device"] = lambda: dense_rewire(h, ei, kp)
        inner["dense_on_device"] = 1
    del p2, n2, s2
    res = timed_groups(fns, inner, args.reps, args.warmup)
    out["times"] = res
    if "dense_on_device" in res:
        a, b = res["op"], res["dense_on_device"]
        out["ratio_dense_over_op"] = b["median_ms"] / a["median_ms"]
        # the margin asked for: the medians apart by more than both run-to-run spreads
        out["spread_ms"] = dict(op=a["max_ms"] - a["min_ms"], dense=b["max_ms"] - b["min_ms"])
        out["op_faster_beyond_spread"] = bool(b["min_ms"] > a["max_ms"])
    if args.kernel_stats:
        out["kernels"] = kernel_stats(args.kernel_stats, n, f)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
