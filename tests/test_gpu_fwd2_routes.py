"""The two routes of ngnn_sage2_fwd (csrc/ngnn_fwd2.hip) at the C ABI, every
launch form on both:

* one call with NGNN_SAGE2_ALL: the fused launch (k_fwd2x: edge phase + main
  phase), then the narrow aggregate;
* three calls EDGE, MAIN, NARROW on the same buffers: k_edge_nb, then k_fwd2,
  then the narrow aggregate -- the route bench.py's per-launch timer and
  NGNN_FWD2_FUSE=0 take.

Forms: K0 = 100 (the 16-deep tail chunk, T16) and 128; dropout off / byte
mode (p = 0.2) / bit mode (p = 0.5); a root term (mean) and none (wr0 NULL,
sum); plain rows and rows indexed through xrow into a 50-row table.  Blocks:
N = 33 with 17 rows with in-edges (two edge tiles, three row tiles, the last
of each ragged) and N = 16 with 3.  H = 256, F1 = 47.

Both routes meet the fp64 oracle (test_gpu_fwd2.py's, run in double) at the
suite's 1e-5 bar for h, the logits and the saved aggregate.  They also agree
bit for bit: the fused kernel runs the same two bodies on the same tile ->
workgroup map, and on the commit before the host half was rewritten every
case here gave max |fused - staged| = 0 for all three arrays, so equality is
asserted.
"""
import pytest
import torch

from ngnn import _lib

from test_gpu_fused import OUT
from test_gpu_fwd2 import _block, _oracle, _params

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
H, F1, TABLE = 256, 47, 50
STAGED = (_lib.SAGE2_EDGE, _lib.SAGE2_MAIN, _lib.SAGE2_NARROW)


def _agg64(x, ei, N, reduce):
    agg = torch.zeros(N, x.size(1), dtype=torch.float64).index_add_(0, ei[1], x.double()[ei[0]])
    if reduce == "mean":
        deg = torch.zeros(N, dtype=torch.float64).index_add_(0, ei[1], torch.ones(ei.size(1), dtype=torch.float64))
        agg = agg / deg.clamp(min=1.0)[:, None]
    return agg


def _forward(stage_list, x_dev, xrow, col_x, blk, N, K0, reduce, w, root, p, seed):
    """ngnn_sage2_fwd once per entry of stage_list on fresh NaN-filled buffers."""
    lib = _lib.load()
    nan = float("nan")
    h = torch.full((N, H), nan, device=DEV)
    out = torch.full((N, F1), nan, device=DEV)
    agg0 = torch.full((N, K0), nan, device=DEV)
    ws = torch.empty(lib.ngnn_sage2_workspace_bytes(K0, F1, N), dtype=torch.uint8, device=DEV)
    wl0, bl0, wr0, wl1, bl1, wr1 = w
    for stages in stage_list:
        _lib.check(lib.ngnn_sage2_fwd(
            _lib.ptr(x_dev), None, _lib.ptr(xrow), None, TABLE if xrow is not None else 0, x_dev.stride(0), K0, N,
            None, blk.n_active, None, _lib.ptr(blk.rowptr), _lib.ptr(blk.col), _lib.ptr(col_x),
            _lib.REDUCE[reduce], _lib.ptr(wl0), _lib.ptr(bl0), _lib.ptr(wr0) if root else None, wl0.stride(0), H,
            _lib.ptr(wl1), _lib.ptr(bl1), _lib.ptr(wr1), wl1.stride(0), F1, p, seed, None, _lib.ptr(h), h.stride(0),
            N, None, _lib.ptr(agg0), agg0.stride(0), _lib.ptr(out), out.stride(0), None, stages, _lib.ptr(ws),
            ws.numel(), _lib.stream_handle(DEV)), "ngnn_sage2_fwd")
    torch.cuda.synchronize()
    return h.cpu(), out.cpu(), agg0.cpu()


@pytest.mark.parametrize("N,n_act", [(33, 17), (16, 3)])
@pytest.mark.parametrize("K0", [100, 128])
@pytest.mark.parametrize("p", [0.0, 0.2, 0.5])
@pytest.mark.parametrize("form", ["root", "root-indexed", "root-free"])
def test_fwd2_fused_and_staged_routes(N, n_act, K0, p, form):
    root, indexed = form != "root-free", form == "root-indexed"
    reduce = "mean" if root else "sum"
    ei, blk = _block(7 * N + K0, N, n_act, deg_max=6, zero_rows=(1,))
    g = torch.Generator().manual_seed(N + K0)
    ref = _params(K0, H, F1, 5)
    if not root:
        with torch.no_grad():
            ref.convs[0].lin_r.weight.zero_()
    seed = 4242 + K0 + N
    if indexed:
        table = torch.randn(TABLE, K0, generator=g)
        xrow = torch.randint(0, TABLE, (N,), generator=g)
        x = table[xrow]
        x_dev, xrow_dev = table.to(DEV), xrow.to(DEV)
        col_x = xrow_dev[blk.col.long()].to(torch.int32)
    else:
        x = torch.randn(N, K0, generator=g)
        x_dev, xrow_dev, col_x = x.to(DEV), None, None
    w = [q.detach().to(DEV) for c in ref.convs for q in (c.lin_l.weight, c.lin_l.bias, c.lin_r.weight)]
    with torch.no_grad():
        h_r, out_r = _oracle(x.double(), ei, ref.double(), reduce, p, seed, N, H)
    agg_r = _agg64(x, ei, N, reduce)
    rows = min(N, -(-n_act // 16) * 16)  # the saved aggregate: rows of the edge tiles
    got = {}
    for name, stage_list in (("fused", (_lib.SAGE2_ALL,)), ("staged", STAGED)):
        h, out, agg0 = got[name] = _forward(stage_list, x_dev, xrow_dev, col_x, blk, N, K0, reduce, w, root, p, seed)
        err = [float((a.double() - b).abs().max()) for a, b in ((h, h_r), (out, out_r), (agg0[:rows], agg_r[:rows]))]
        print(f"{name}: max |err| vs fp64  h {err[0]:.3g}  out {err[1]:.3g}  agg0 {err[2]:.3g}")
        torch.testing.assert_close(h.double(), h_r, **OUT)
        torch.testing.assert_close(out.double(), out_r, **OUT)
        torch.testing.assert_close(agg0[:rows].double(), agg_r[:rows], **OUT)
    diff = [float((a[:r] - b[:r]).abs().max()) for a, b, r in zip(got["fused"], got["staged"], (N, N, rows))]
    print(f"fused vs staged: max |diff|  h {diff[0]:.3g}  out {diff[1]:.3g}  agg0 {diff[2]:.3g}")
    for a, b, r in zip(got["fused"], got["staged"], (N, N, rows)):
        assert torch.equal(a[:r], b[:r])
