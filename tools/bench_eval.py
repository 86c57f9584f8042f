#!/usr/bin/env python
"""Times whole-graph evaluation: ``SAGE.inference`` over every node.

The reference evaluates after each epoch (``test_ogb`` ->
``model.inference(data.x, subgraph_loader)``, pipeline.py:85-92,179,291):
the synthetic ogbn-products graph at full scale, an in-order NeighborLoader
(batch size 4092, fanout [15, 10]) and SAGE(100, 256, 47, 2), features
resident on the device.  One ``inference`` call on the block-free plan
(ngnn.infer) is timed against one with the loader wrapped in a plain
iterable, which forces the reference loop.  Device events, one warm-up call
each.  Prints one JSON line.

    python tools/bench_eval.py                # full scale
    python tools/bench_eval.py --scale 0.01   # a small graph
    python tools/bench_eval.py --skip-loop
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "noise-gnn_amd"))

import torch  # noqa: E402

import ngnn  # noqa: E402
from ngnn import infer, models  # noqa: E402
from ngnn.loader import NeighborLoader, synthetic_graph  # noqa: E402


class Plain:
    """The loader as a plain iterable of batches (the loop's input); notes a
    device event at the start of every pass = every layer."""

    def __init__(self, loader):
        self.loader, self.marks = loader, []

    def __iter__(self):
        ev = torch.cuda.Event(enable_timing=True)
        ev.record()
        self.marks.append(ev)
        return iter(self.loader)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return out, a.elapsed_time(b) / 1e3, b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--skip-loop", action="store_true")
    ap.add_argument("--batch-size", type=int, default=4092)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    graph = synthetic_graph("ogbn-products", dev, scale=args.scale)
    torch.manual_seed(0)
    model = ngnn.SAGE(100, 256, 47, 2).to(dev).eval()
    fan = [15, 10]

    def loader():
        return NeighborLoader(graph, None, num_neighbors=fan, batch_size=args.batch_size)

    res = {"workload": "SAGE(100,256,47,2).inference, synthetic ogbn-products", "scale": args.scale,
           "nodes": graph.num_nodes, "edges": graph.num_edges, "batch_size": args.batch_size,
           "fanout": fan, "device": torch.cuda.get_device_name(0)}
    model.inference(graph.x, loader(), dev)  # warm-up (workspaces, code objects)
    infer._record_times = True
    out, res["eval_fused_s"], _ = timed(lambda: model.inference(graph.x, loader(), dev))
    infer._record_times = False
    res["plan"] = list(models.last_inference_plan)
    res["fused_layer_s"] = [round(t, 6) for t in infer.last_inference_times]
    if not args.skip_loop:
        model.inference(graph.x, Plain(loader()), dev)  # warm-up
        plain = Plain(loader())
        ref, res["eval_loop_s"], end = timed(lambda: model.inference(graph.x, plain, dev))
        assert models.last_inference_plan == ["loop", "loop"]
        marks = plain.marks + [end]
        res["loop_layer_s"] = [round(marks[i].elapsed_time(marks[i + 1]) / 1e3, 6) for i in range(2)]
        res["speedup"] = round(res["eval_loop_s"] / res["eval_fused_s"], 3)
        res["max_abs_diff"] = float((out - ref).abs().max())
    for k in ("eval_fused_s", "eval_loop_s"):
        if k in res:
            res[k] = round(res[k], 6)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
