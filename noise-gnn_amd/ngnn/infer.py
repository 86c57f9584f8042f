"""Layer-wise inference without blocks (ABI 22, DESIGN.md "Block-free evaluation").

``SAGE.inference`` / ``SimpleGCN.inference`` (sage.py:42-58,
convolution.py:37-53) keep, per layer and loader batch, only the seed rows of
a conv run over a whole multi-hop block.  Under the sampler's contract a seed
row receives in-edges from hop 0 alone, and hop 0's draws are a pure function
of (block seed, position in the batch, degree) -- so when the loader walks
``arange(N)`` in order, a layer is a pass over loader positions that draws
straight from the graph CSR and reads the previous layer's table by global
node id: no block, no relabelling, no ``x[n_id]`` copy.

Per layer one of three plans (``last_inference_plan``):

``"narrow"``   mean / sum layers with F_out < K: one dense pass
               ``[z | root] = x [W_l ; W_r]^T + [0 | b]`` over the table (the
               row-tile kernel without a neighbour term), then
               ``ngnn_infer_narrow`` gathers F_out-wide z rows, drawing the
               neighbours in the kernel.
``"rowtile"``  every other layer (F_out >= K, or max): ``ngnn_infer_draw``
               writes a chunk's draws as a CSR of global ids, which
               ``ngnn_sage_fwd_raw`` takes through its fused-gather arguments
               (xrow = the chunk's nodes, col_x = the drawn ids).
``"loop"``     the reference loop for that layer (a shape outside the kernels'
               envelope, e.g. K % 4 != 0).
"""
from __future__ import annotations

import torch

from . import _lib, fused

# one entry per layer of the last inference call: "rowtile", "narrow" or
# "loop" (tests read it, so a silent fallback cannot pass)
last_inference_plan: list = []
# device seconds per layer of the last call when _record_times is set (the
# timing tool; costs a device sync per call)
last_inference_times: list = []
_record_times = False
# private knob (tests): at most this many loader batches per chunk
_max_chunk_batches = None


def _u64(v: int) -> int:
    return int(v) & (2**64 - 1)


def seed_rows(graph, fanout: int, batch_size: int, seed0: int, seed_stride: int, r0: int,
              n_rows: int, seeds=None):
    """ngnn_infer_draw: (rowptr int32[n_rows + 1], col int32[n_rows * fanout])
    -- col at its capacity, the first rowptr[-1] entries written; no host
    read-back."""
    lib = _lib.load()
    dev = graph.rowptr.device
    if not graph.rowptr.is_cuda:
        raise RuntimeError("ngnn runs on the GPU only: the graph is on the CPU")
    if seeds is not None:
        seeds = seeds.to(dev, torch.int64).contiguous()
    rowptr = torch.empty(max(n_rows, 0) + 1, dtype=torch.int32, device=dev)
    col = torch.empty(max(n_rows * fanout, 1), dtype=torch.int32, device=dev)
    ws = torch.empty(max(lib.ngnn_infer_draw_workspace_bytes(n_rows), 4), dtype=torch.uint8, device=dev)
    _lib.check(lib.ngnn_infer_draw(
        _lib.ptr(graph.rowptr), _lib.ptr(graph.col), _lib.ptr(seeds), r0, n_rows, batch_size, fanout,
        _u64(seed0), _u64(seed_stride), _lib.ptr(rowptr), _lib.ptr(col), _lib.ptr(ws), ws.numel(),
        _lib.stream_handle(dev)), "ngnn_infer_draw")
    return rowptr, col


def _layer_spec(conv, last: bool):
    """(reduce, W_l, W_r or None, bias, relu) of a SAGEConv / GCNConv."""
    from .nn import GCNConv, SAGEConv
    if isinstance(conv, SAGEConv):
        aggr = "sum" if conv.aggr == "add" else conv.aggr
        return aggr, conv.lin_l.weight, conv.lin_r.weight, conv.lin_l.bias, not last
    if isinstance(conv, GCNConv):
        if conv.normalize:
            # the block-free plan draws the seed rows' in-edges only: it cannot
            # know the sources' degrees on the sampled block -- the loop plan
            return None
        return "sum", conv.lin.weight, None, conv.bias, not last
    return None


def eligible(convs, x_all, loader, device) -> bool:
    """Does this call take the fused plan?  A plain ngnn NeighborLoader over
    arange(N) in order (not sync_free, one rank, no shuffle, whole batches
    kept), fp32 features for all N nodes, an fp32 model of SAGEConv / GCNConv
    layers, hop-0 fanout <= 64."""
    from .loader import NeighborLoader
    if not isinstance(loader, NeighborLoader):
        return False
    if loader.sync_free or loader.world_size != 1 or loader.rank != 0 or loader.shuffle or loader.drop_last:
        return False
    g = loader.graph
    N = g.num_nodes
    dev = torch.device(device)
    if dev.type != "cuda" or not g.rowptr.is_cuda or (dev.index is not None and dev.index != g.rowptr.device.index):
        return False
    if not torch.is_tensor(x_all) or x_all.dim() != 2 or x_all.size(0) != N or x_all.dtype != torch.float32:
        return False
    if N == 0 or N >= 2**31 or loader.batch_size <= 0:
        return False
    if not loader.num_neighbors or not 0 <= int(loader.num_neighbors[0]) <= 64:
        return False
    for conv in convs:
        if _layer_spec(conv, False) is None:
            return False
        if any(p.dtype != torch.float32 or not p.is_cuda for p in conv.parameters()):
            return False
    inp = loader.input_nodes
    if inp.numel() != N:
        return False
    return bool(torch.equal(inp, torch.arange(N, device=inp.device, dtype=inp.dtype)))  # once per call


def _chunks(N: int, bs: int, width: int, fanout: int):
    """Whole-batch chunks [r0, r1) of the positions, each operand of a chunk
    (rows x width floats, rows x fanout draws) under 2 GiB."""
    per_row = 4 * max(width, fanout, 1)
    nb = max(1, ((2**31 - 4096) // per_row) // bs)
    if _max_chunk_batches is not None:
        nb = max(1, min(nb, int(_max_chunk_batches)))
    step = nb * bs
    return [(r0, min(r0 + step, N)) for r0 in range(0, N, step)]


def _rowtile_layer(loader, ep: int, x, spec, out) -> bool:
    """A wide / max layer into `out` [N, Fo]; False (nothing launched): the
    row-tile kernel refuses the shape."""
    reduce, wl, wr, b, relu = spec
    lib = _lib.load()
    g = loader.graph
    N, K = x.shape
    Fo = wl.shape[0]
    bs, f = loader.batch_size, int(loader.num_neighbors[0])
    wl_ = wl.detach()
    wr_ = wr.detach() if wr is not None else None
    if wl_.stride(1) != 1 or (wr_ is not None and (wr_.stride(1) != 1 or wr_.stride(0) != wl_.stride(0))):
        wl_, wr_ = wl_.contiguous(), (wr_.contiguous() if wr_ is not None else None)
    ws = fused._workspace(x.device, "sage_fwd", lib.ngnn_sage_fwd_raw_workspace_bytes(K, Fo, 0), zero=True)
    seed0 = loader.batch_seed(ep, 0)
    stride = loader.batch_seed(ep, 1) - seed0
    for n, (r0, r1) in enumerate(_chunks(N, bs, max(K, Fo), f)):
        rows = r1 - r0
        rowptr, col = seed_rows(g, f, bs, seed0, stride, r0, rows)
        xrow = torch.arange(r0, r1, dtype=torch.int64, device=x.device)
        rc = fused._fwd_raw(x, xrow=xrow, x_rows=N, n_rows=rows, rowptr=rowptr, col=col, col_x=col,
                            reduce=reduce, wl=wl_, wr=wr_, bias=b.detach(), out=out[r0:r1], relu=relu, ws=ws)
        if rc == _lib.E_SHAPE and n == 0:
            return False
        _lib.check(rc, "ngnn_sage_fwd_raw")
    return True


def _narrow_layer(loader, ep: int, x, spec, out) -> bool:
    """A narrowing mean / sum layer into `out` [N, Fo]; False (nothing
    launched): the dense pass is outside the row-tile kernel's envelope."""
    reduce, wl, wr, b, relu = spec
    lib = _lib.load()
    g = loader.graph
    N, K = x.shape
    Fo = wl.shape[0]
    dev = x.device
    bs, f = loader.batch_size, int(loader.num_neighbors[0])
    if K % 4 or x.stride(0) % 4:
        return False  # (as the row-tile plan: 16-B column quads of x)
    Fz = Fo + (-Fo) % 4
    if wr is not None:
        # [z | root] = x [W_l ; 0 ; W_r]^T + [0 | b]: one pass over the table
        w = torch.zeros(Fz + Fo, K, dtype=torch.float32, device=dev)
        w[:Fo].copy_(wl.detach())
        w[Fz:].copy_(wr.detach())
        bias = torch.zeros(Fz + Fo, dtype=torch.float32, device=dev)
        bias[Fz:].copy_(b.detach())
    else:  # GCNConv: z = x W^T, the bias joins in the aggregate's epilogue
        w = wl.detach().contiguous()
        bias = None
    Ft = w.shape[0]
    ld = Ft + (-Ft) % 4
    buf = torch.empty(N, ld, dtype=torch.float32, device=dev)  # (the call's own: released with it)
    ws = fused._workspace(dev, "sage_fwd", lib.ngnn_sage_fwd_raw_workspace_bytes(K, Ft, 0), zero=True)
    st = _lib.stream_handle(dev)
    step = max(1, (2**31 - 4096) // (4 * max(x.stride(0), ld)))
    for n, r0 in enumerate(range(0, N, step)):
        rows = min(step, N - r0)
        rc = fused._fwd_raw(x[r0:r0 + rows], reduce="sum", wr=w, bias=bias, out=buf[r0:r0 + rows], ws=ws)
        if rc == _lib.E_SHAPE and n == 0:
            return False
        _lib.check(rc, "ngnn_sage_fwd_raw")
    seed0 = loader.batch_seed(ep, 0)
    stride = loader.batch_seed(ep, 1) - seed0
    for r0, r1 in _chunks(N, bs, max(ld, Fo), f):
        root = buf[r0:r1, Fz:] if wr is not None else None
        o = out[r0:r1]
        _lib.check(lib.ngnn_infer_narrow(
            _lib.ptr(g.rowptr), _lib.ptr(g.col), None, r0, r1 - r0, bs, f, _u64(seed0), _u64(stride),
            _lib.ptr(buf), ld, _lib.ptr(root), ld, _lib.ptr(b.detach()) if wr is None else None, Fo,
            _lib.REDUCE[reduce], int(relu), _lib.ptr(o), o.stride(0), st), "ngnn_infer_narrow")
    return True


def _loop_layer(conv, x_cur, loader, device, relu: bool):
    """One layer of the reference loop (models._layerwise_inference's body)."""
    xs = []
    for batch in loader:
        n_id = batch.n_id.to(device)
        edge_index = batch.edge_index.to(device)
        x = conv(x_cur.index_select(0, n_id), edge_index)
        x = x[:batch.batch_size]
        if relu:
            x = x.relu()
        xs.append(x)
    return torch.cat(xs, dim=0)


def fused_inference(convs, num_layers: int, x_all, loader, device):
    """The fused plan of an eligible call.  Layer i draws with the loader's
    pass number epoch + i; the loader's epoch ends num_layers further on,
    exactly as iterating it once per layer would leave it."""
    out_device = x_all.device
    x_cur = x_all.to(device)
    if x_cur.stride(1) != 1 or x_cur.stride(0) % 4 != 0:
        x_cur = x_cur.contiguous()
    ep0 = loader.epoch
    N = x_cur.size(0)
    plan, times, events = [], [], []
    for i in range(num_layers):
        conv = convs[i]
        spec = _layer_spec(conv, i == num_layers - 1)
        reduce, wl = spec[0], spec[1]
        Fo, K = wl.shape
        kind = "narrow" if (reduce in ("mean", "sum") and Fo < K) else "rowtile"
        if _record_times:
            events.append(torch.cuda.Event(enable_timing=True))
            events[-1].record()
        ok = False
        if x_cur.dtype == torch.float32 and x_cur.size(1) == K:
            out = torch.empty(N, Fo, dtype=torch.float32, device=x_cur.device)
            ok = (_narrow_layer if kind == "narrow" else _rowtile_layer)(loader, ep0 + i, x_cur, spec, out)
        if ok:
            loader.epoch = ep0 + i + 1
        else:
            kind = "loop"
            loader.epoch = ep0 + i  # (the pass the loop is about to make)
            out = _loop_layer(conv, x_cur, loader, device, spec[4])
        plan.append(kind)
        x_cur = out
    if _record_times:
        events.append(torch.cuda.Event(enable_timing=True))
        events[-1].record()
        events[-1].synchronize()
        times = [events[i].elapsed_time(events[i + 1]) / 1e3 for i in range(num_layers)]
    last_inference_plan[:] = plan
    last_inference_times[:] = times
    return x_cur.to(out_device)
