"""GPU parity of the two-layer backward's chunk scheme (csrc/ngnn_bwd2.hip):
a row slice owns every S-th 32-row chunk, and a chunk past the seed rows (no
dy row in it) skips everything dy feeds -- its loads, stage B's dy-only
k-chunk, the dW_r1 products.

Every case calls ngnn_sage2_bwd as tests/test_gpu_bwd2.py does, with its block
builder and its float64 restatement, but hands the scattered gradient in as
g_pre (float64 sums rounded once to fp32), so no atomics run: all six
gradients meet tests/gradbar.py's bar (max|g - g_ref| <= 1e-5 max|g_ref|) AND
two launches agree bit for bit.  K0 = 100, F1 = 47, H = 256 throughout.

Shapes (n_rows, R, R'), in chunks of 32 rows:
  (96, 1, 96)     one seed row; chunk 0 is the only seed chunk; slices 3..63
                  own nothing and write zero slab parts
  (200, 40, 200)  a full seed chunk, a partial one, then chunks without dy
  (64, 64, 64)    every chunk is a seed chunk (R = R')
  (70, 0, 70)     no seed chunk: the gradients of g alone
  (2300, 33, 2215)  the launch uses S = 64 row slices whatever the size
                  (B2_S in ngnn_bwd2.hip, the grid of k_bwd2), so R' = 2215
                  gives C = 70 = S + 6 chunks: slices 0 and 1 own a seed chunk
                  and a chunk without dy (c and c + 64), slices 2..5 two
                  chunks without dy, slices 6..63 one.  (With C > S no slice
                  is empty under the cyclic ownership; the small shapes above
                  cover the empty slices.)
"""
import pytest
import torch

from ngnn import _lib

from gradbar import assert_wgrad
from test_gpu_bwd2 import _case, _reference

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
K0, F1 = 100, 47
KEYS = ("dWl1", "dbl1", "dWr1", "dWl0", "dbl0", "dWr0")
ROOT_FREE_KEYS = ("dWl1", "dbl1", "dWl0", "dbl0")
S_SLICES = 64  # B2_S
WIDE = (32 * S_SLICES + 32 * 6 + 60, 33, 32 * S_SLICES + 32 * 5 + 7)  # C = 70 chunks, the last one partial


def _g_pre(c, R, reduce):
    """g[s] = sum over edges s -> d, d < R, of dy[d] (/ deg(d)): [N][C4] fp32,
    zero past F1 (what the forward's loss head scatters)."""
    src, dst = c["ei"][0].long(), c["ei"][1].long()
    N = c["dy"].size(0)
    w = torch.ones(dst.numel(), dtype=torch.float64)
    if reduce == "mean":
        w = w / torch.bincount(dst, minlength=N).double()[dst].clamp(min=1)
    m = dst < R
    g = torch.zeros(N, (F1 + 3) // 4 * 4, dtype=torch.float64)
    g[:, :F1].index_add_(0, src[m], c["dy"].double()[dst[m]] * w[m][:, None])
    return g.float()


def _launch(c, R, Rn, reduce, yscale, g_pre, root=True, agg0=None):
    lib = _lib.load()
    N = c["dy"].size(0)
    d = {k: (v.to(DEV) if isinstance(v, torch.Tensor) else v) for k, v in c.items()}
    out = dict(dWl1=torch.empty(F1, 256, device=DEV), dbl1=torch.empty(F1, device=DEV),
               dWr1=torch.empty(F1, 256, device=DEV) if root else None,
               dWl0=torch.empty(256, K0, device=DEV), dbl0=torch.empty(256, device=DEV),
               dWr0=torch.empty(256, K0, device=DEV) if root else None)
    bounds = torch.tensor([R, Rn], dtype=torch.int32, device=DEV)
    ws = torch.zeros(lib.ngnn_sage2_bwd_workspace_bytes(N, K0, F1), dtype=torch.uint8, device=DEV)
    xr = d["table"] is not None
    x = (d["table"] if xr else d["x"]) if root else None
    xrow = d["xrow"] if xr else None
    a0 = (c["agg0"] if agg0 is None else agg0).to(DEV)
    gp = g_pre.to(DEV)
    res = []
    for _ in range(2):
        for v in out.values():
            if v is not None:
                v.fill_(float("nan"))
        rc = lib.ngnn_sage2_bwd(
            _lib.ptr(d["dy"]), F1, F1, _lib.ptr(d["wl1"]), _lib.ptr(d["wr1"]), 256, _lib.ptr(d["h"]), 256,
            yscale, _lib.ptr(x), None, _lib.ptr(xrow), None, x.size(0) if xr else 0, K0, K0,
            _lib.ptr(a0), K0, _lib.ptr(d["rowptr"]), _lib.ptr(d["col"]), N,
            bounds.data_ptr(), bounds.data_ptr() + 4, _lib.REDUCE[reduce],
            *(_lib.ptr(out[k]) for k in KEYS), _lib.ptr(gp), None,
            _lib.ptr(ws), ws.numel(), _lib.stream_handle(DEV))
        assert rc == _lib.OK, rc
        torch.cuda.synchronize()
        res.append({k: v.cpu() for k, v in out.items() if v is not None})
    for k in res[0]:
        assert torch.equal(res[0][k], res[1][k]), f"{k}: two launches differ"
    return res[0]


def _check(got, want, keys=KEYS):
    for k in keys:
        assert_wgrad(got[k].double(), want[k], msg=k)


@pytest.mark.parametrize("N,R,Rn", [(96, 1, 96), (200, 40, 200), (64, 64, 64), WIDE])
def test_bwd2_chunks_rooted(N, R, Rn):
    c = _case(N + R, N, R, Rn, K0, F1)
    got = _launch(c, R, Rn, "mean", 1.25, _g_pre(c, R, "mean"))
    _check(got, _reference(c, R, Rn, "mean", 1.25))


def test_bwd2_chunks_no_seed_chunk():
    """R = 0 with a g of its own: dy contributes nothing (dW_r1 = db1 = 0) and
    the other four gradients are those of g alone -- the restatement's for the
    block whose seeds scattered that g, with W_r1 = 0 (so dh = g W_l1)."""
    N, Rn, R_g = 70, 70, 40
    c = _case(5, N, R_g, Rn, K0, F1)
    g = _g_pre(c, R_g, "mean")
    assert float(g[32:].abs().max()) > 0  # (g reaches the chunks past the first)
    want = _reference(dict(c, wr1=torch.zeros_like(c["wr1"])), R_g, Rn, "mean", 2.0)
    want["dWr1"] = torch.zeros(F1, 256, dtype=torch.float64)
    want["dbl1"] = torch.zeros(F1, dtype=torch.float64)
    got = _launch(c, 0, Rn, "mean", 2.0, g)
    _check(got, want)


def test_bwd2_chunks_root_free():
    """dW_r0 = dW_r1 = NULL (a root-free stack: W_r1 is read, zeros; x is not)."""
    N, R, Rn = WIDE
    c = _case(3, N, R, Rn, K0, F1)
    c["wr1"] = torch.zeros_like(c["wr1"])
    got = _launch(c, R, Rn, "sum", 2.0, _g_pre(c, R, "sum"), root=False)
    _check(got, _reference(c, R, Rn, "sum", 2.0), ROOT_FREE_KEYS)


def test_bwd2_chunks_fused_row_gather():
    """x rows through n_id: the index of a slice's next chunk (c + S) is the
    one fetched a chunk ahead."""
    N, R, Rn = WIDE
    c = _case(4, N, R, Rn, K0, F1, xr=True)
    got = _launch(c, R, Rn, "mean", 2.0, _g_pre(c, R, "mean"))
    _check(got, _reference(c, R, Rn, "mean", 2.0))


def test_bwd2_chunks_edgeless_rows_without_dy():
    """Mean aggregation; the rows without in-edges keep an aggregate that was
    never written (NaN here), also in the chunks without dy: it counts as 0."""
    N, R, Rn = 200, 40, 200
    c = _case(6, N, R, Rn, K0, F1)
    deg = c["rowptr"][1:].long() - c["rowptr"][:-1].long()
    edgeless = torch.nonzero(deg[:Rn] == 0).flatten()
    assert int((edgeless >= 64).sum()) > 0  # (some sit in chunks 2.. , all without dy)
    poisoned = c["agg0"].clone()
    assert float(poisoned[edgeless].abs().max()) == 0.0
    poisoned[edgeless] = float("nan")
    got = _launch(c, R, Rn, "mean", 1.25, _g_pre(c, R, "mean"), agg0=poisoned)
    _check(got, _reference(c, R, Rn, "mean", 1.25))
