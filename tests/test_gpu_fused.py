"""GPU parity of the fused SAGE path (ngnn_sage_fwd + bounded backward).

Tolerances (fp32): outputs rtol = atol = 1e-5 (north star); gradients, one
more GEMM deep, rtol = 1e-4 / atol = 1e-5; weight gradients (sums over up to
~1e4 rows) max|g - g_ref| <= 1e-5 max|g_ref| per tensor (tests/gradbar.py).  Dropout in the fused path uses a counter-based hash
RNG; ``dropout_keep`` below replicates it on the host so train-mode results are
checked element for element against the oracle with the same mask.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ngnn
from ngnn.block import Block
from ngnn.fused import sage_layer_fwd
from oracle import c_agg, pyg_ref
from gradbar import assert_wgrad

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
OUT = dict(rtol=1e-5, atol=1e-5)
GRAD = dict(rtol=1e-4, atol=1e-5)

M32 = np.uint64(0xFFFFFFFF)


def _lowbias32(x):
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7FEB352D)) & M32
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846CA68B)) & M32
    return x ^ (x >> np.uint64(16))


def dropout_keep(seed, n_rows, n_cols, p):
    """Host replica of ngnn_device.h::Dropout.  Byte mode (thresh != 128): one
    hash per column quad, keep <=> byte (col % 4) >= ceil(p * 256).  Bit mode
    (p = 0.5): keep <=> bit c & 31 of the hash of word c >> 5."""
    s0, s1 = np.uint64(seed & 0xFFFFFFFF), np.uint64((seed >> 32) & 0xFFFFFFFF)
    thresh = dropout_thresh(p)
    r = np.arange(n_rows, dtype=np.uint64)[:, None]
    c = np.arange(n_cols, dtype=np.uint64)[None, :]
    rk = _lowbias32(r ^ s0) ^ s1
    u = np.uint64
    if thresh == 128:
        word = c >> u(5)
        bit = c & u(31)
        h = _lowbias32((rk + word) & M32)
        return torch.from_numpy(((h >> bit) & u(1)) == u(1))
    h = _lowbias32((rk + (c >> u(2))) & M32)
    byte = (h >> (u(8) * (c & u(3)))) & u(0xFF)
    return torch.from_numpy(byte >= u(thresh))


def dropout_thresh(p):
    import math
    pf = float(np.float32(p))
    if pf <= 0:
        return 0
    return max(1, min(256, math.ceil(pf * 256.0)))


def dropout_scale(p):
    """Survivor scale 1 / (1 - p_eff), p_eff = ceil(p * 256) / 256."""
    t = dropout_thresh(p)
    return 0.0 if t >= 256 else float(np.float32(256.0) / np.float32(256 - t))


def rand_block(seed, N, E, order="dst"):
    g = torch.Generator().manual_seed(seed)
    ei = torch.randint(0, N, (2, E), generator=g)
    if order == "dst":
        ei = ei[:, torch.argsort(ei[1], stable=True)]
    return ei


@pytest.mark.parametrize("K,Fo", [(100, 256), (256, 47), (128, 40), (24, 7), (767, 16),
                                  (256, 256), (300, 512), (8, 3), (129, 20), (64, 600),
                                  (767, 1534)])
@pytest.mark.parametrize("reduce", ["mean", "max", "sum"])
def test_fused_layer_matches_oracle(K, Fo, reduce):
    N, E = 700, 5000
    g = torch.Generator().manual_seed(K * 31 + Fo)
    ei = rand_block(K + Fo, N, E, "dst" if K % 2 == 0 else None)
    # leave the last 200 rows without in-edges (skipped W_l half)
    ei = ei[:, ei[1] < N - 200]
    x = torch.randn(N, K, generator=g)
    conv = pyg_ref.SAGEConv(K, Fo, aggr=reduce)
    with torch.no_grad():
        want = conv(x, ei)
    blk = Block(ei.to(DEV), N)
    for relu in (False, True):
        got = sage_layer_fwd(x.to(DEV), blk, reduce, conv.lin_l.weight.to(DEV),
                             conv.lin_l.bias.to(DEV), conv.lin_r.weight.to(DEV), relu=relu,
                             p_drop=0.0, seed=0).cpu()
        torch.testing.assert_close(got, want.relu() if relu else want, **OUT)


def test_fused_layer_dropout_mask_and_scale():
    N, K, Fo, p, seed = 500, 64, 128, 0.5, 12345
    ei = rand_block(1, N, 3000)
    x = torch.randn(N, K)
    conv = pyg_ref.SAGEConv(K, Fo)
    with torch.no_grad():
        pre = conv(x, ei).relu()
    blk = Block(ei.to(DEV), N)
    got = sage_layer_fwd(x.to(DEV), blk, "mean", conv.lin_l.weight.to(DEV), conv.lin_l.bias.to(DEV),
                         conv.lin_r.weight.to(DEV), relu=True, p_drop=p, seed=seed).cpu()
    keep = dropout_keep(seed, N, Fo, p)
    torch.testing.assert_close(got, pre * keep * dropout_scale(p), **OUT)
    frac = keep.float().mean().item()
    assert abs(frac - (1 - p)) < 0.01
    # deterministic in the seed, different for another seed
    again = sage_layer_fwd(x.to(DEV), blk, "mean", conv.lin_l.weight.to(DEV),
                           conv.lin_l.bias.to(DEV), conv.lin_r.weight.to(DEV), relu=True,
                           p_drop=p, seed=seed).cpu()
    assert torch.equal(got, again)


@pytest.mark.parametrize("K,Fo", [(100, 256), (256, 47), (128, 40), (52, 100), (200, 129),
                                  (24, 7), (44, 33), (300, 512), (768, 16)])
def test_math_modes_against_fp64(K, Fo):
    """The default 3 x bf16 split root term and the exact-fp32 one
    (ngnn.fused.exact_f32) both match the oracle at the fp32 bar, and the
    split's error against an fp64 evaluation of the same layer is of the
    order of the exact-fp32 MFMA's own rounding error."""
    from ngnn.fused import exact_f32
    N = 700
    g = torch.Generator().manual_seed(K * 31 + Fo)
    ei = rand_block(K + Fo, N, 3000)
    x = torch.randn(N, K, generator=g)
    conv = pyg_ref.SAGEConv(K, Fo)
    with torch.no_grad():
        want32 = conv(x, ei)
        c64 = pyg_ref.SAGEConv(K, Fo).double()
        c64.load_state_dict({k: v.double() for k, v in conv.state_dict().items()})
        want64 = c64(x.double(), ei)
    blk = Block(ei.to(DEV), N)
    args = (x.to(DEV), blk, "mean", conv.lin_l.weight.to(DEV), conv.lin_l.bias.to(DEV),
            conv.lin_r.weight.to(DEV))
    got_split = sage_layer_fwd(*args, relu=False, p_drop=0.0, seed=1).cpu()
    with exact_f32():
        got_exact = sage_layer_fwd(*args, relu=False, p_drop=0.0, seed=1).cpu()
    torch.testing.assert_close(got_split, want32, **OUT)
    torch.testing.assert_close(got_exact, want32, **OUT)
    e_split = (got_split.double() - want64).abs().max().item()
    e_exact = (got_exact.double() - want64).abs().max().item()
    e_ref = (want32.double() - want64).abs().max().item()  # the CPU fp32 reference's own error
    assert e_split <= 2.0 * max(e_exact, e_ref) + 1e-7, (e_split, e_exact, e_ref)


@pytest.mark.parametrize("K,Fo", [(256, 47), (128, 40), (64, 10), (100, 16), (256, 48), (33, 20)])
@pytest.mark.parametrize("reduce", ["mean", "sum"])
def test_narrow_output_layer_matches_oracle(K, Fo, reduce):
    """NGNN_FWD_NARROW (the output layer's form): z = x W_l^T for every row
    in the root-term launch, then out[d] += mean/sum of z over d's in-edges
    -- equal to the oracle's lin_l(agg(x)) + lin_r(x) at the fp32 bar, with
    and without the edge-row bound (rows past it have no in-edges)."""
    N = 900
    g = torch.Generator().manual_seed(K + Fo)
    ei = rand_block(K * 3 + Fo, N, 5000)
    ei = ei[:, ei[1] < 600]  # rows >= 600 receive no edges
    x = torch.randn(N, K, generator=g)
    conv = pyg_ref.SAGEConv(K, Fo)
    conv.aggr = reduce
    with torch.no_grad():
        want = conv(x, ei)
    for n_act in (None, 600):
        blk = Block(ei.to(DEV), N)
        blk.n_active = n_act
        got = sage_layer_fwd(x.to(DEV), blk, reduce, conv.lin_l.weight.to(DEV),
                             conv.lin_l.bias.to(DEV), conv.lin_r.weight.to(DEV), relu=False,
                             p_drop=0.0, seed=0, narrow=True).cpu()
        torch.testing.assert_close(got, want, **OUT)


@pytest.mark.parametrize("K,Fo", [(767, 512), (768, 1024), (767, 40), (1030, 300), (250, 513)])
@pytest.mark.parametrize("reduce", ["max", "mean", "sum"])
def test_wide_layer_matches_oracle(K, Fo, reduce):
    """The wide path (ngnn_wide.hip: aggregate launch + 2-D tiled fp32-MFMA
    dual GEMM; Amazon-Computers' 767 -> 512 max layer): output with bias,
    ReLU and hash dropout against the oracle with the host-replicated mask,
    the saved aggregate bit-identical to the C oracle's edge-order sums, rows
    past the edge-row bound (no in-edges) on the root term alone, and the
    device-side row bound honoured (rows past it untouched)."""
    from ngnn import _lib
    from ngnn.fused import agg_buffer
    if not _lib.load().ngnn_sage_wide_preferred(K, Fo, 0):
        pytest.skip("shape stays on the row-tile kernel")
    N, p, seed = 1100, 0.5, 77
    g = torch.Generator().manual_seed(K + Fo)
    ei = rand_block(K * 5 + Fo, N, 6000)
    ei = ei[:, ei[1] < 700]  # rows >= 700 receive no edges
    x = torch.randn(N, K, generator=g)
    conv = pyg_ref.SAGEConv(K, Fo, aggr=reduce)
    with torch.no_grad():
        pre = conv(x, ei).relu()
    keep = dropout_keep(seed, N, Fo, p)
    want = pre * keep * dropout_scale(p)
    blk = Block(ei.to(DEV), N)
    blk.n_active = 700
    agg = agg_buffer(N, K, DEV, Fo)
    agg.fill_(float("nan"))
    got = sage_layer_fwd(x.to(DEV), blk, reduce, conv.lin_l.weight.to(DEV),
                         conv.lin_l.bias.to(DEV), conv.lin_r.weight.to(DEV), relu=True,
                         p_drop=p, seed=seed, agg_out=agg).cpu()
    torch.testing.assert_close(got, want, **OUT)
    want_agg = c_agg.agg_fwd(x.numpy(), ei.numpy(), N, reduce)[:700]
    assert torch.equal(agg[:700].cpu(), torch.from_numpy(want_agg))
    # device row bound (a graph slot's row count: the layer's input has 900
    # rows, every edge source among them), no saved-aggregate buffer
    ei2 = ei[:, ei[0] < 900]
    with torch.no_grad():
        want2 = conv(x[:900], ei2).relu() * keep[:900] * dropout_scale(p)
    nrd = torch.tensor([900], dtype=torch.int32, device=DEV)
    blk2 = Block(ei2.to(DEV), N)
    blk2.n_active = 700
    blk2.n_rows_dev = nrd
    got2 = sage_layer_fwd(x.to(DEV), blk2, reduce, conv.lin_l.weight.to(DEV),
                          conv.lin_l.bias.to(DEV), conv.lin_r.weight.to(DEV), relu=True,
                          p_drop=p, seed=seed).cpu()
    torch.testing.assert_close(got2[:900], want2, **OUT)


KINK_TOL = 1e-5
# the GPU's ReLU decisions the oracle takes are a handful per layer (VERDICT r5:
# a bound, so a kernel bug cannot hide behind the override)
KINK_MAX = 128


class _MaskedSAGE(pyg_ref.SAGE):
    """Oracle SAGE whose dropout uses given keep masks (one per hidden layer;
    None: no dropout).

    gpu_hidden (optional, one [N, H] tensor per hidden layer: the GPU's own
    post-ReLU/dropout activations, fused._debug_acts): ReLU's kink.  Where a
    pre-activation lies within KINK_TOL of its row's largest magnitude, fp32
    summation order alone (GPU vs CPU) decides its sign, and with it whether
    the whole gradient of that element passes -- one flipped element moved a
    hidden unit's weight-gradient row by ~5e-3 of its max (round 5).  There
    the oracle takes the GPU's decision (h > 0), everywhere else its own:
    backward pinned on identical ReLU masks, as the max tests pin ties.
    kink_rows: only rows below it (the rows the GPU wrote: its R')."""

    def __init__(self, *a, masks=None, gpu_hidden=None, kink_rows=None, **k):
        super().__init__(*a, **k)
        self.masks = masks
        self.gpu_hidden = gpu_hidden
        self.kink_rows = kink_rows
        self.kinks = []  # ambiguous elements overridden, per hidden layer

    def forward(self, x, edge_index):
        self.kinks = []
        for i, conv in enumerate(self.convs):
            x = conv(x, edge_index)
            if i != self.num_layers - 1:
                gh = None if self.gpu_hidden is None else self.gpu_hidden[i]
                if gh is None:
                    x = x.relu()
                else:
                    pre = x.detach()
                    amb = pre.abs() <= KINK_TOL * pre.abs().amax(1, keepdim=True)
                    if self.kink_rows is not None:
                        amb[self.kink_rows:] = False
                    gate = torch.where(amb, gh[:pre.size(0)].cpu() > 0, pre > 0)
                    self.kinks.append(int((amb & (gate != (pre > 0))).sum()))
                    assert self.kinks[-1] <= KINK_MAX, f"layer {i}: {self.kinks[-1]} ReLU kinks overridden"
                    x = x * gate
                if self.masks is not None:
                    x = x * self.masks[i] * dropout_scale(self.dropout)
        return x


@pytest.mark.parametrize("layers,aggr", [(2, "mean"), (3, "mean"), (2, "max")])
@pytest.mark.parametrize("train", [False, True])
def test_stack_fwd_bwd_matches_oracle(layers, aggr, train):
    """Whole SAGE stack on a NeighborLoader-shaped block, loss on the seed rows
    only (pipeline.py:155-160): outputs, dx and every parameter gradient."""
    from ngnn.loader import sample_block, synthetic_graph
    graph = synthetic_graph("ogbn-products", DEV, seed=2, scale=0.005)
    fan = [8, 5, 3][:layers]
    b = sample_block(graph, graph.train_idx[:128], fan, seed=4)
    N = b.num_nodes
    torch.manual_seed(layers)
    mine = ngnn.SAGE(100, 64, 47, layers, dropout=0.5, aggr=aggr).to(DEV)
    mine.train(train)
    seed_box = {}
    if train:
        # capture the seed the model draws, to rebuild the masks on the host
        torch.manual_seed(99)
        seed_box["seed"] = int(torch.randint(0, 2**62, (1,)).item())
        torch.manual_seed(99)
    x = b.x.clone().requires_grad_(True)
    out = mine(x, b.edge_index)
    loss = F.cross_entropy(out[:b.batch_size], b.y[:b.batch_size])
    loss.backward()

    if train:
        masks = [dropout_keep(seed_box["seed"] + 7919 * i, N, 64, 0.5).float()
                 for i in range(layers - 1)]
        ref = _MaskedSAGE(100, 64, 47, layers, dropout=0.5, aggr=aggr, masks=masks)
    else:
        ref = pyg_ref.SAGE(100, 64, 47, layers, dropout=0.5, aggr=aggr).eval()
    ref.load_state_dict({k: v.cpu() for k, v in mine.state_dict().items()})
    xr = b.x.cpu().clone().requires_grad_(True)
    out_r = ref(xr, b.edge_index.cpu())
    loss_r = F.cross_entropy(out_r[:b.batch_size], b.y[:b.batch_size].cpu())
    loss_r.backward()
    torch.testing.assert_close(out.detach().cpu(), out_r.detach(), **OUT)
    torch.testing.assert_close(x.grad.cpu(), xr.grad, **GRAD)
    for (k, p), (_, q) in zip(mine.named_parameters(), ref.named_parameters()):
        assert_wgrad(p.grad.cpu(), q.grad, msg=k)


@pytest.mark.parametrize("aggr", ["mean", "max"])
def test_stack_deterministic_mode(aggr):
    """torch.use_deterministic_algorithms(True) switches the input-gradient
    scatter to the source-grouped CSR gather: same values as the oracle, and
    bitwise identical across runs."""
    from ngnn.loader import sample_block, synthetic_graph
    graph = synthetic_graph("ogbn-products", DEV, seed=5, scale=0.005)
    b = sample_block(graph, graph.train_idx[:128], [8, 5, 3], seed=6)
    torch.manual_seed(1)
    mine = ngnn.SAGE(100, 64, 47, 3, dropout=0.5, aggr=aggr).to(DEV).eval()
    ref = pyg_ref.SAGE(100, 64, 47, 3, dropout=0.5, aggr=aggr).eval()
    ref.load_state_dict({k: v.cpu() for k, v in mine.state_dict().items()})
    prev = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True)
    try:
        runs = []
        for _ in range(2):
            mine.zero_grad()
            x = b.x.clone().requires_grad_(True)
            out = mine(x, b.edge_index)
            F.cross_entropy(out[:b.batch_size], b.y[:b.batch_size]).backward()
            runs.append([x.grad.clone()] + [p.grad.clone() for p in mine.parameters()])
    finally:
        torch.use_deterministic_algorithms(prev)
    for a, c in zip(runs[0], runs[1]):
        assert torch.equal(a, c)
    xr = b.x.cpu().clone().requires_grad_(True)
    F.cross_entropy(ref(xr, b.edge_index.cpu())[:b.batch_size], b.y[:b.batch_size].cpu()).backward()
    torch.testing.assert_close(runs[0][0].cpu(), xr.grad, **GRAD)
    for g, (k, q) in zip(runs[0][1:], ref.named_parameters()):
        assert_wgrad(g.cpu(), q.grad, msg=k)


def test_stack_full_output_gradient():
    """Gradient on EVERY output row (no seed slicing): the bound R = N path."""
    N = 400
    ei = rand_block(7, N, 3000, None)
    x = torch.randn(N, 32)
    torch.manual_seed(0)
    mine = ngnn.SAGE(32, 48, 10, 3).to(DEV).eval()
    ref = pyg_ref.SAGE(32, 48, 10, 3).eval()
    ref.load_state_dict({k: v.cpu() for k, v in mine.state_dict().items()})
    G = torch.randn(N, 10)
    xd = x.to(DEV).requires_grad_(True)
    (mine(xd, ei.to(DEV)) * G.to(DEV)).sum().backward()
    xr = x.clone().requires_grad_(True)
    (ref(xr, ei) * G).sum().backward()
    torch.testing.assert_close(xd.grad.cpu(), xr.grad, **GRAD)
    for (k, p), (_, q) in zip(mine.named_parameters(), ref.named_parameters()):
        assert_wgrad(p.grad.cpu(), q.grad, msg=k)


def test_zero_gradient_and_no_grad_paths():
    N = 100
    ei = rand_block(3, N, 500)
    m = ngnn.SAGE(16, 16, 4, 2).to(DEV)
    x = torch.randn(N, 16, device=DEV)
    out = m(x, ei.to(DEV))
    (out * 0).sum().backward()
    for p in m.parameters():
        assert p.grad is not None and not p.grad.any()
    with torch.no_grad():
        o2 = m.eval()(x, ei.to(DEV))
    assert o2.shape == (N, 4)


def _dgrad_dense_ref(dy, y, yscale, wl, wr, ei, N, R, reduce):
    """fp32 torch reference of a layer's input gradient on the rows the
    bounded backward writes: dz = dy (* [y > 0] * yscale) on rows < R,
    dh = dz W_r + A^T (dz / deg) W_l  (edges into rows >= R dropped)."""
    dz = dy.clone()
    if y is not None:
        dz = torch.where(y > 0, dz * yscale, torch.zeros_like(dz))
    dz[R:] = 0
    src, dst = ei[0], ei[1]
    deg = torch.bincount(dst, minlength=N).clamp(min=1).float()
    m = dz[dst] / deg[dst, None] if reduce == "mean" else dz[dst]
    dagg = torch.zeros_like(dz).index_add_(0, src, m)
    return dz @ wr + dagg @ wl


def _lowdim_img_bytes(Fo, K):
    """Offset of g in the lowdim workspace (include/ngnn.h: [W image | g])."""
    c4, half, ntw = (Fo + 3) // 4 * 4, -(-(-(-K // 16)) // 2), 1
    while ntw < half:
        ntw *= 2
    return ((c4 // 2) * 2 * ntw * 64 * 4 + 255) // 256 * 256


@pytest.mark.parametrize("Fo,K,reduce,masked", [
    (47, 256, "mean", False), (47, 256, "sum", True), (10, 48, "mean", True), (5, 30, "sum", False),
    (8, 300, "mean", True), (12, 100, "mean", False), (3, 17, "mean", True)])
def test_dgrad_lowdim_abi(Fo, K, reduce, masked):
    """ngnn_sage_dgrad_lowdim (narrow-space scatter + MFMA pass) against a
    dense fp32 reference: rows < R' written, rows >= R' untouched, the
    workspace left zero; a second call gives the same result."""
    from ngnn import _lib
    lib = _lib.load()
    N, E, R = 700, 5000, 150
    ei = rand_block(Fo * 7 + K, N, E)
    g = torch.Generator().manual_seed(K)
    dy = torch.randn(N, Fo, generator=g)
    y = torch.randn(N, Fo, generator=g) if masked else None
    wl, wr = torch.randn(Fo, K, generator=g) * 0.2, torch.randn(Fo, K, generator=g) * 0.2
    yscale = 2.0 if masked else 1.0
    ref = _dgrad_dense_ref(dy, y, yscale, wl, wr, ei, N, R, reduce)
    src_into = ei[0][ei[1] < R]
    Rn = max(R, int(src_into.max()) + 1 if src_into.numel() else 0)
    blk = Block(ei.to(DEV), N)
    bnd = torch.tensor([Rn, R], dtype=torch.int32, device=DEV)
    ws = torch.zeros(lib.ngnn_sage_dgrad_lowdim_workspace_bytes(N, Fo, K), dtype=torch.uint8,
                     device=DEV)
    dyd, wld, wrd = dy.to(DEV), wl.to(DEV), wr.to(DEV)
    yd = y.to(DEV) if masked else None
    outs = []
    for _ in range(2):
        dh = torch.full((N, K), 7.0, device=DEV)
        rc = lib.ngnn_sage_dgrad_lowdim(
            _lib.ptr(dyd), Fo, _lib.ptr(yd), Fo, yscale, _lib.ptr(wld), _lib.ptr(wrd), K, Fo, K,
            _lib.ptr(blk.rowptr), _lib.ptr(blk.col), N, bnd.data_ptr() + 4, bnd.data_ptr(),
            _lib.REDUCE[reduce], _lib.ptr(dh), K, 0, _lib.ptr(ws), ws.numel(),
            _lib.stream_handle(DEV))
        _lib.check(rc, "ngnn_sage_dgrad_lowdim")
        torch.cuda.synchronize()
        assert not ws[_lowdim_img_bytes(Fo, K):].any(), "g not left zero"
        outs.append(dh.cpu())
    torch.testing.assert_close(outs[0][:Rn], ref[:Rn], **GRAD)
    assert torch.all(outs[0][Rn:] == 7.0)  # rows >= R' untouched
    # (the narrow-space scatter uses float atomics: run-to-run order noise)
    torch.testing.assert_close(outs[1], outs[0], rtol=1e-5, atol=1e-5)


def test_dgrad_lowdim_shape_envelope():
    """Weight images past the LDS budget are refused with NGNN_E_SHAPE (the
    backward asks ngnn_sage_dgrad_route, which sends no such shape here)."""
    from ngnn import _lib
    lib = _lib.load()
    N, Fo, K = 64, 47, 500
    ei = rand_block(1, N, 200)
    blk = Block(ei.to(DEV), N)
    bnd = torch.tensor([N, N], dtype=torch.int32, device=DEV)
    dy = torch.randn(N, Fo, device=DEV)
    w = torch.randn(Fo, K, device=DEV)
    dh = torch.empty(N, K, device=DEV)
    ws = torch.zeros(lib.ngnn_sage_dgrad_lowdim_workspace_bytes(N, Fo, K), dtype=torch.uint8,
                     device=DEV)
    rc = lib.ngnn_sage_dgrad_lowdim(
        _lib.ptr(dy), Fo, None, Fo, 1.0, _lib.ptr(w), _lib.ptr(w), K, Fo, K, _lib.ptr(blk.rowptr),
        _lib.ptr(blk.col), N, bnd.data_ptr(), bnd.data_ptr() + 4, _lib.REDUCE["mean"],
        _lib.ptr(dh), K, 0, _lib.ptr(ws), ws.numel(), _lib.stream_handle(DEV))
    assert rc == _lib.E_SHAPE


class _MaskedGCN(pyg_ref.SimpleGCN):
    """Oracle SimpleGCN whose dropout uses given keep masks (None: no
    dropout); gpu_hidden / kink_rows: ReLU's kink as _MaskedSAGE."""

    def __init__(self, *a, masks=None, gpu_hidden=None, kink_rows=None, **k):
        super().__init__(*a, **k)
        self.masks = masks
        self.gpu_hidden = gpu_hidden
        self.kink_rows = kink_rows

    def forward(self, x, edge_index):
        for i, conv in enumerate(self.convs):
            x = conv(x, edge_index)
            if i != self.num_layers - 1:
                gh = None if self.gpu_hidden is None else self.gpu_hidden[i]
                if gh is None:
                    x = x.relu()
                else:
                    pre = x.detach()
                    amb = pre.abs() <= KINK_TOL * pre.abs().amax(1, keepdim=True)
                    if self.kink_rows is not None:
                        amb[self.kink_rows:] = False
                    x = x * torch.where(amb, gh[:pre.size(0)].cpu() > 0, pre > 0)
                if self.masks is not None:
                    x = x * self.masks[i] * dropout_scale(self.dropout)
        return x


@pytest.mark.parametrize("dims", [(100, 256, 47), (20, 32, 6), (64, 32, 40), (256, 128, 47)])
@pytest.mark.parametrize("layers", [2, 3])
@pytest.mark.parametrize("train", [False, True])
def test_gcn_stack_fwd_bwd_matches_oracle(dims, layers, train):
    """SimpleGCN (convolution.py:7-35) on the fused stack -- aggregate-first
    layers (F_in <= F_out) and PyG's transform-first form (F_in > F_out) --
    against the oracle: outputs, dx and every parameter gradient, with the
    hash dropout replicated on the host."""
    from ngnn.loader import sample_block, synthetic_graph
    K, H, C = dims
    graph = synthetic_graph("ogbn-products", DEV, seed=7, scale=0.005, num_features=K)
    fan = [8, 5, 3][:layers]
    b = sample_block(graph, graph.train_idx[:128], fan, seed=4)
    N = b.num_nodes
    torch.manual_seed(layers + K)
    mine = ngnn.SimpleGCN(K, H, C, layers, dropout=0.5).to(DEV).train(train)
    if train:
        torch.manual_seed(99)
        s = int(torch.randint(0, 2**62, (1,)).item())
        torch.manual_seed(99)
    x = b.x.clone().requires_grad_(True)
    out = mine(x, b.edge_index)
    y = b.y[:b.batch_size] % C  # (the graph has 47 classes; C may be fewer)
    F.cross_entropy(out[:b.batch_size], y).backward()
    if train:
        masks = [dropout_keep(s + 7919 * i, N, H, 0.5).float() for i in range(layers - 1)]
        ref = _MaskedGCN(K, H, C, layers, dropout=0.5, masks=masks)
    else:
        ref = pyg_ref.SimpleGCN(K, H, C, layers, dropout=0.5).eval()
    ref.load_state_dict({k: v.cpu() for k, v in mine.state_dict().items()})
    xr = b.x.cpu().clone().requires_grad_(True)
    out_r = ref(xr, b.edge_index.cpu())
    F.cross_entropy(out_r[:b.batch_size], y.cpu()).backward()
    # sum aggregation, no normalisation: outputs grow with degree x width, so the
    # absolute tolerance is OUT's relative to the output scale (fp32 reordering)
    scale = max(1.0, float(out_r.detach().abs().max()))
    torch.testing.assert_close(out.detach().cpu(), out_r.detach(), rtol=OUT["rtol"],
                               atol=OUT["atol"] * scale)
    torch.testing.assert_close(x.grad.cpu(), xr.grad, **GRAD)
    for (k, p), (_, q) in zip(mine.named_parameters(), ref.named_parameters()):
        assert_wgrad(p.grad.cpu(), q.grad, msg=k)


@pytest.mark.parametrize("hidden", [64, 160])
def test_gcn_graph_step_matches_eager(hidden):
    """SimpleGCN through GraphedTrainStep (captured step) equals eager
    training on the same batches (dropout off).  hidden 160 > F_in 128:
    aggregate-first layer 0, zero-copy slot; hidden 64: transform-first layer
    0, whose backward rebuilds its aggregate from the slot's rows (copied)."""
    from ngnn.graphs import GraphedTrainStep, slot_size
    from ngnn.loader import NeighborLoader, synthetic_graph
    g = synthetic_graph("ogbn-arxiv", DEV, seed=0, scale=0.05)
    loader = NeighborLoader(g, g.train_idx, [10, 5], 256, shuffle=True, seed=3)
    batches = [b for _, b in zip(range(4), loader)]
    torch.manual_seed(11)
    m_e = ngnn.SimpleGCN(g.x.size(1), hidden, g.num_classes, 2, dropout=0.0).to(DEV)
    m_g = ngnn.SimpleGCN(g.x.size(1), hidden, g.num_classes, 2, dropout=0.0).to(DEV)
    m_g.load_state_dict(m_e.state_dict())
    o_e = torch.optim.Adam(m_e.parameters(), lr=1e-2, fused=True, capturable=True)
    le = []
    for b in batches:
        loss = F.cross_entropy(m_e(b.x, b.edge_index)[:b.batch_size], b.y[:b.batch_size])
        o_e.zero_grad(set_to_none=False)
        loss.backward()
        o_e.step()
        le.append(float(loss))
    o_g = torch.optim.Adam(m_g.parameters(), lr=1e-2, fused=True, capturable=True)
    n_cap, e_cap = slot_size(256, [10, 5])
    step = GraphedTrainStep(m_g, o_g, 256, n_cap, e_cap, g.x.size(1), DEV)
    step.capture(batches[0].x, batches[0].edge_index, batches[0].y)
    assert step.zero_copy == (hidden >= g.x.size(1))
    lg = [float(step(b.x, b.edge_index, b.y)) for b in batches]
    torch.cuda.synchronize()
    for a, c in zip(le, lg):
        assert abs(a - c) < 1e-4 * max(1.0, abs(a)), (le, lg)
    for (n, pe), pg in zip(m_e.named_parameters(), m_g.parameters()):
        torch.testing.assert_close(pg, pe, rtol=1e-4, atol=1e-5, msg=n)


@pytest.mark.parametrize("K,Fo", [(100, 256), (128, 40), (256, 256), (36, 7), (300, 512),
                                  (24, 47)])
@pytest.mark.parametrize("reduce", ["mean", "max", "sum"])
def test_bf16_rows_equal_widened_rows(K, Fo, reduce):
    """NGNN_X_BF16: bf16 rows read as bf16 (root term on the single bf16
    part, gather widened exactly) give BITWISE the layer of the same rows
    widened to fp32 (the split of an exact bf16 value is (x, 0, 0): the three
    dropped products are exact zeros), outputs and saved aggregate; and both
    match the fp32 oracle on the widened rows."""
    N, E = 900, 6000
    g = torch.Generator().manual_seed(K + 7 * Fo)
    ei = rand_block(K * Fo, N, E)
    ei = ei[:, ei[1] < N - 150]
    xb = torch.randn(N, K, generator=g).to(torch.bfloat16)
    conv = pyg_ref.SAGEConv(K, Fo, aggr=reduce)
    blk = Block(ei.to(DEV), N)
    args = (blk, reduce, conv.lin_l.weight.to(DEV), conv.lin_l.bias.to(DEV),
            conv.lin_r.weight.to(DEV))
    outs = []
    for x in (xb.to(DEV), xb.float().to(DEV)):
        agg = torch.full((N, K), 7.0, device=DEV)
        o = sage_layer_fwd(x, *args, relu=True, p_drop=0.25, seed=99, agg_out=agg)
        outs.append((o.cpu(), agg.cpu()))
    assert torch.equal(outs[0][0], outs[1][0])
    # the saved aggregate is defined on rows with in-edges (the backward never
    # reads the others; a pre-aggregated max layer writes them as 0)
    has = torch.bincount(ei[1], minlength=N) > 0
    assert torch.equal(outs[0][1][has], outs[1][1][has])
    with torch.no_grad():
        pre = conv(xb.float(), ei).relu()
    keep = dropout_keep(99, N, Fo, 0.25)
    torch.testing.assert_close(outs[0][0], pre * keep * dropout_scale(0.25), **OUT)


@pytest.mark.parametrize("layers", [2, 3])
def test_bf16_features_stack_matches_widened(layers):
    """A SAGE stack on bf16 features (no input gradient) keeps them bf16 for
    layer 0 (forward and weight gradient read bf16 rows): logits and every
    parameter gradient equal the run on the widened features up to the
    input-gradient scatter's atomic ordering."""
    from ngnn.loader import sample_block, synthetic_graph
    graph = synthetic_graph("ogbn-products", DEV, seed=3, scale=0.005)
    b = sample_block(graph, graph.train_idx[:256], [8, 5, 3][:layers], seed=2)
    torch.manual_seed(5)
    m = ngnn.SAGE(100, 64, 47, layers, dropout=0.5).to(DEV).train()
    res = []
    for x in (b.x.to(torch.bfloat16), b.x.to(torch.bfloat16).float()):
        m.zero_grad(set_to_none=True)
        torch.manual_seed(42)
        # both runs end in the same bf16 cast (the bf16-input stack returns
        # bf16 logits), so the loss backward feeds both the same dlogits
        out = m(x, b.edge_index).to(torch.bfloat16).float()
        F.cross_entropy(out[:256], b.y[:256]).backward()
        res.append((out.detach(), {k: p.grad.clone() for k, p in m.named_parameters()}))
    torch.testing.assert_close(res[0][0], res[1][0], rtol=0, atol=0)
    for k in res[0][1]:
        torch.testing.assert_close(res[0][1][k], res[1][1][k], rtol=1e-5, atol=1e-6, msg=k)


@pytest.mark.parametrize("K,Fo,narrow", [(100, 256, False), (256, 256, False), (36, 7, False),
                                         (300, 512, False), (256, 47, True), (24, 47, True)])
@pytest.mark.parametrize("reduce", ["mean", "sum"])
@pytest.mark.parametrize("xdt", [torch.float32, torch.bfloat16])
def test_bf16_weights_one_part_image_bitwise(K, Fo, narrow, reduce, xdt):
    """NGNN_W_BF16 (a bf16 model's weights, widened): the one-part split
    image skips the products with the weights' second and third parts, which
    are exact zeros -- the root term is BITWISE the three-part layer's (narrow
    mode: the whole layer), with fp32 and bf16 rows, across column slices
    (256 -> 256 takes 3 slices with the three-part image and 1 with one
    part).  The neighbour term of a one-part layer streaming W_l runs on bf16
    MFMA (the aggregate split in three bf16 parts against the bf16 W_l image,
    csrc/ngnn_sage_rt_kern.h nb_chunk_b16) instead of exact fp32 steps: the two
    layers then agree within the fp32 bars, and the saved aggregate is the
    same bits."""
    if narrow and xdt == torch.bfloat16:
        pytest.skip("narrow mode reads fp32 rows")
    N, E = 900, 6000
    g = torch.Generator().manual_seed(K + 3 * Fo)
    ei = rand_block(K * Fo + 1, N, E)
    ei = ei[:, ei[1] < N - 150]
    x = torch.randn(N, K, generator=g).to(xdt).to(DEV)
    conv = pyg_ref.SAGEConv(K, Fo, aggr=reduce)
    wl, bl, wr = (t.detach().to(torch.bfloat16).float().to(DEV)
                  for t in (conv.lin_l.weight, conv.lin_l.bias, conv.lin_r.weight))
    blk = Block(ei.to(DEV), N)
    epi = dict(relu=False, p_drop=0.0) if narrow else dict(relu=True, p_drop=0.25)
    outs = []
    for w1 in (False, True):
        agg = None if narrow else torch.full((N, K), 7.0, device=DEV)
        o = sage_layer_fwd(x, blk, reduce, wl, bl, wr, seed=5, agg_out=agg, narrow=narrow,
                           w_bf16=w1, **epi)
        outs.append((o.cpu(), None if agg is None else agg.cpu()))
    if narrow:
        assert torch.equal(outs[0][0], outs[1][0])
    else:
        torch.testing.assert_close(outs[0][0], outs[1][0], **OUT)
        assert torch.equal(outs[0][1], outs[1][1])
    with torch.no_grad():
        c2 = pyg_ref.SAGEConv(K, Fo, aggr=reduce)
        c2.lin_l.weight.copy_(wl.cpu()), c2.lin_l.bias.copy_(bl.cpu()), c2.lin_r.weight.copy_(wr.cpu())
        ref = c2(x.float().cpu(), ei)
    if not narrow:
        ref = ref.relu() * dropout_keep(5, N, Fo, 0.25) * dropout_scale(0.25)
    torch.testing.assert_close(outs[1][0], ref, **OUT)


@pytest.mark.parametrize("n", [0, 1, 7, 4096 + 3, 3_000_001])
def test_cast_f32_bf16_equals_torch(n):
    """ngnn_cast_f32_bf16 (a bf16 model's logits) is torch's .to(bfloat16)
    bit for bit: round to nearest even, inf kept, every NaN (either sign, any
    payload) the canonical 0x7FC0; ragged lengths and a size that takes the
    4-deep unrolled loop."""
    from ngnn import _lib
    g = torch.Generator().manual_seed(n)
    x = (torch.randn(n, generator=g) * 3).to(DEV)
    if n > 8:
        x[:4] = torch.tensor([float("inf"), -float("inf"), 1.0 + 2**-8, -(1.0 + 3 * 2**-8)])
        # NaNs: quiet +/-, a signalling payload, one with low payload bits only
        nan_bits = torch.tensor([0x7FC00000, -0x00400000, 0x7F800001, 0x7FBFFFFF],
                                dtype=torch.int64).to(torch.int32)
        x[4:8] = nan_bits.view(torch.float32).to(DEV)
    y = torch.empty(n, dtype=torch.bfloat16, device=DEV)
    _lib.check(_lib.load().ngnn_cast_f32_bf16(_lib.ptr(x), _lib.ptr(y), n,
                                              _lib.stream_handle(DEV)), "cast")
    torch.cuda.synchronize()
    want = x.to(torch.bfloat16)
    assert torch.equal(y.view(torch.int16), want.view(torch.int16))


@pytest.mark.parametrize("layers,train", [(2, False), (3, False), (3, True)])
def test_bf16_activations_equal_rounded_fp32_rows(layers, train):
    """A bf16 model's hidden activations are stored as bf16 rows
    (NGNN_OUT_BF16 epilogue; the next layer reads them with NGNN_X_BF16, the
    output layer in narrow mode; the backward's weight gradient reads them as
    bf16 h and bf16 mask rows, the seed-row aggregate rebuild as bf16, the
    input-gradient kernels through ngnn_widen_bf16_rows).  Against the same
    stack whose hidden layers write fp32 rows then rounded to the same bf16
    values: logits bitwise, parameter gradients equal up to the input-gradient
    scatter's atomic order (one bf16 rounding)."""
    from ngnn import fused
    from ngnn.loader import sample_block, synthetic_graph
    graph = synthetic_graph("ogbn-products", DEV, seed=3, scale=0.01)
    graph.x = graph.x.to(torch.bfloat16)
    b = sample_block(graph, graph.train_idx[:512], [10, 8, 5][:layers], seed=2)
    torch.manual_seed(5)
    m = ngnn.SAGE(100, 256, 47, layers, dropout=0.5).to(DEV).to(torch.bfloat16)
    m.train(train)
    orig = fused.sage_layer_fwd
    calls = []

    def rounded_fp32_rows(*a, **k):
        want = k.get("out_bf16", False)
        calls.append(want)
        k["out_bf16"] = False
        h = orig(*a, **k)
        return h.bfloat16().float() if want else h

    res = []
    for patch in (False, True):
        fused.sage_layer_fwd = rounded_fp32_rows if patch else orig
        try:
            m.zero_grad(set_to_none=True)
            torch.manual_seed(42)
            out = m(b.x, b.edge_index)
            F.cross_entropy(out[:512].float(), b.y[:512]).backward()
            torch.cuda.synchronize()
        finally:
            fused.sage_layer_fwd = orig
        res.append((out.detach().float().cpu(),
                    {k: p.grad.detach().float().cpu().clone() for k, p in m.named_parameters()}))
    assert calls.count(True) == layers - 1  # every hidden layer asked for bf16 rows
    assert torch.equal(res[0][0], res[1][0])
    for k in res[0][1]:
        # (bf16 gradients: a different atomic order may move one rounding)
        torch.testing.assert_close(res[0][1][k], res[1][1][k], rtol=2.0**-8,
                                   atol=2.0**-8 * float(res[1][1][k].abs().max()), msg=k)
