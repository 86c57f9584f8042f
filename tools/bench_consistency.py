"""get_uncertainty_batch + fix_cr (forward + backward of the pair) on one
sampled block: the products [15, 10] batch-1024 block (C = 47, B = 1024) and
the arxiv one (C = 40, B = 512) from the project's synthetic graph and
sampler, against the reference's op sequence (src/utils/losses.py:185-246)
restated here in torch.

Variants, same process, same GPU; device events around groups of calls,
warm-up first, medians and the min-max spread over the groups
(bench_rewire.py's timed_groups); (b), (c) and (d) alternate group by group
in one call, (a) is timed in a call of its own (its host round trip would
sit between the others' groups):

  a_reference   the reference as written: edge_index.cpu(), a scipy COO
                build, torch.sparse_coo_tensor, its upload, torch.sparse.mm
                on the device, the sparse row sum, the elementwise chain;
                fix_cr with its host mask from ind_noisy
  b_torch_dev   a vectorised all-device composition (index_add_ by
                edge_index[0]): the strongest version a user has without the op
  c_ngnn        ngnn.losses, rows=None (w for every node, as the reference)
  d_ngnn_rows   ngnn.losses, rows=B (all the pipeline reads)

(c) and (d) take the block's by-source CSR from the block cache, as a
training step does (the model's backward builds it); its build is timed on
its own (by_source_csr_build).  Also recorded: kernel launches per call
(torch.profiler, when it reports device kernels), the host waits per call
that each variant has by construction, each variant's agreement with (b),
and bitwise repeatability.

Writes one JSON file (default profiles/consist_bench.json) and prints it.
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


def uncertainty_reference(edge_index, y_pure, nbr_classes, device, epsilon=1e-16):
    """losses.py:185-204 as written (scipy on the host, sparse.mm on the device)."""
    import scipy.sparse as sp
    p = torch.exp(y_pure)
    n = y_pure.shape[0]
    ei = edge_index.cpu()
    row, col = ei[0].numpy(), ei[1].numpy()
    coo = sp.coo_matrix((np.ones(len(row)), (row, col)), shape=(n, n))
    indices = np.vstack((np.array(coo.row), np.array(coo.col)))
    adj = torch.sparse_coo_tensor(torch.LongTensor(indices), torch.FloatTensor(np.array(coo.data)),
                                  torch.Size(coo.shape)).to(device)
    ptc = torch.sparse.mm(adj, p)
    ptc = ptc / (adj.sum(dim=1).to_dense().view(-1, 1) + epsilon)
    hpt = -torch.sum(ptc * torch.log2(ptc + 1e-5), dim=1)
    return torch.exp(-hpt / torch.log2(torch.tensor(nbr_classes)))


def uncertainty_torch_dev(edge_index, y_pure, nbr_classes, epsilon=1e-16):
    """The same numbers without leaving the device."""
    p = torch.exp(y_pure)
    s = torch.zeros_like(p).index_add_(0, edge_index[0], p[edge_index[1]])
    deg = torch.bincount(edge_index[0], minlength=p.size(0)).to(p.dtype)
    ptc = s / (deg.view(-1, 1) + epsilon)
    hpt = -torch.sum(ptc * torch.log2(ptc + 1e-5), dim=1)
    return torch.exp(-hpt / float(np.log2(nbr_classes)))


def fix_cr_torch(y_pure, y_noisy, ind_noisy, batch_size, p_cutoff, w, host_mask):
    """losses.py:206-246, name='ce', hard labels; host_mask: the mask the
    reference builds from ind_noisy on the host (and never reads)."""
    if host_mask:
        mask_noisy = np.zeros(y_pure.shape[0]).astype(bool)
        mask_noisy[ind_noisy] = True
    y_pure, y_noisy = y_pure[:batch_size], y_noisy[:batch_size]
    pseudo_pure, pseudo_noisy = torch.exp(y_pure), torch.exp(y_noisy)
    max_probs, max_idx = torch.max(pseudo_pure, dim=-1)
    mask = max_probs.ge(p_cutoff).float()
    masked = F.cross_entropy(pseudo_noisy, max_idx, reduction="none") * mask
    return (w[:batch_size] * masked).mean()


def count_kernels(fn):
    """Device kernels of one call, or None when the profiler reports none."""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(e.device_type).endswith("CUDA") and "memcpy" not in e.name.lower()
                and "memset" not in e.name.lower())
        return n or None
    except Exception:  # noqa: BLE001 -- the count is an extra, the times are the result
        return None


def run_shape(name, B, args, dev):
    from ngnn.block import build_csr, get_block
    from ngnn.loader import sample_block, synthetic_graph
    from ngnn.losses import fix_cr, get_uncertainty_batch
    print(f"bench_consistency: {name}: building the graph", file=sys.stderr, flush=True)
    g = synthetic_graph(name, dev, seed=1)
    C = int(g.num_classes)
    batch = sample_block(g, g.train_idx[:B], [15, 10], seed=3, gather_features=False)
    ei, N = batch.edge_index, int(batch.num_nodes)
    del g
    gen = torch.Generator().manual_seed(B + C)
    yp = torch.log_softmax(2 * torch.randn(N, C, generator=gen), 1).to(dev).requires_grad_(True)
    yn = torch.log_softmax(2 * torch.randn(N, C, generator=gen), 1).to(dev).requires_grad_(True)
    ind_noisy = np.arange(0, B, 3)
    cutoff = 0.5
    blk = get_block(ei, N)
    deg = blk.transposed().degree()
    seed_deg = deg[:B]

    def pair(kind):
        yp.grad = yn.grad = None
        if kind == "a":
            with torch.no_grad():
                w = uncertainty_reference(ei, yp, C, dev)
            loss = fix_cr_torch(yp, yn, ind_noisy, B, cutoff, w, True)
        elif kind == "b":
            with torch.no_grad():
                w = uncertainty_torch_dev(ei, yp, C)
            loss = fix_cr_torch(yp, yn, None, B, cutoff, w, False)
        else:
            w = get_uncertainty_batch(ei, yp, C, dev, rows=B if kind == "d" else None)
            loss = fix_cr(yp, yn, None, batch_size=B, p_cutoff=cutoff, w=w)
        loss.backward()
        return w, loss

    out = dict(shape=dict(graph=name, fanouts=[15, 10], B=B, C=C, N=N, E=int(ei.size(1))),
               by_source_degree=dict(max=int(deg.max()), median=float(deg.float().median()),
                                     seed_rows_max=int(seed_deg.max()), seed_rows_median=float(seed_deg.float().median())))
    # agreement with (b), and repeatability
    wb, lb = pair("b")
    gb = yn.grad.clone()
    agree = {}
    kinds = ["c", "d"]
    try:
        pair("a")
        kinds.insert(0, "a")
    except Exception as exc:  # noqa: BLE001 -- recorded: (a) needs scipy and sparse.mm on the device
        out["a_reference_error"] = f"{type(exc).__name__}: {exc}"[:300]
    for k in kinds:
        w, l_ = pair(k)
        agree[k] = dict(w_max_abs_diff=float((w - wb[:w.numel()]).abs().max()),
                        loss_rel=float(((l_ - lb).abs() / lb.abs()).detach()),
                        grad_err_over_max=float((yn.grad - gb).abs().max() / gb.abs().max()))
    w1, l1 = pair("d")
    g1 = yn.grad.clone()
    w2, l2 = pair("d")
    agree["d_bitwise_repeatable"] = bool(torch.equal(w1, w2) and torch.equal(l1, l2) and torch.equal(g1, yn.grad))
    out["agreement_with_b"] = agree
    print(f"bench_consistency: {name}: N={N} E={int(ei.size(1))}, timing", file=sys.stderr, flush=True)
    names = {"a": "a_reference", "b": "b_torch_dev", "c": "c_ngnn", "d": "d_ngnn_rows"}
    fns = {names[k]: (lambda k=k: pair(k)) for k in ("b", "c", "d")}
    res = timed_groups(fns, {k: args.inner for k in fns}, args.reps, args.warmup)
    if "a" in kinds:
        res.update(timed_groups({"a_reference": lambda: pair("a")}, {"a_reference": args.inner_ref}, args.reps,
                                max(1, args.warmup // 2)))
    res.update(timed_groups({"by_source_csr_build": lambda: build_csr(ei[0], ei[1], N, False)},
                            {"by_source_csr_build": args.inner}, args.reps, args.warmup))
    out["times"] = res
    out["median_us_per_call"] = {k: round(v["median_ms"] * 1e3, 2) for k, v in res.items()}
    out["spread_us_min_max"] = {k: [round(v["min_ms"] * 1e3, 2), round(v["max_ms"] * 1e3, 2)] for k, v in res.items()}
    us = out["median_us_per_call"]
    out["ratios"] = {f"{names[k]}_over_d_ngnn_rows": us[names[k]] / us["d_ngnn_rows"] for k in kinds + ["b"] if k != "d"}
    out["ngnn_faster_than_b_beyond_spread"] = bool(res["b_torch_dev"]["min_ms"] > res["d_ngnn_rows"]["max_ms"])
    out["kernel_launches_per_call"] = {names[k]: count_kernels(lambda k=k: pair(k)) for k in kinds + ["b"]}
    # what each variant waits for on the host, by construction
    out["host_waits_per_call"] = {"a_reference": "1 blocking copy (edge_index.cpu()) + 1 pageable upload of the "
                                                 "COO indices and values", "b_torch_dev": 0, "c_ngnn": 0,
                                  "d_ngnn_rows": 0}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "consist_bench.json"))
    ap.add_argument("--reps", type=int, default=15, help="groups per variant")
    ap.add_argument("--inner", type=int, default=20, help="calls (forward + backward of the pair) per group")
    ap.add_argument("--inner-ref", type=int, default=3, help="calls per group of the reference as written")
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_consistency: needs the GPU (no fallback)")
    dev = torch.device("cuda:0")
    out = {
        "device": torch.cuda.get_device_name(0),
        "method": dict(reps=args.reps, inner=args.inner, inner_ref=args.inner_ref, warmup=args.warmup,
                       note="forward + backward of get_uncertainty_batch + fix_cr per call (hard labels, "
                            "p_cutoff 0.5, w given); device events around groups of calls; b, c, d alternating "
                            "group by group; medians and min-max over the groups; one run, one process"),
        "shapes": [run_shape(n, B, args, dev) for n, B in (("ogbn-products", 1024), ("ogbn-arxiv", 512))],
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
