"""GCNConv(normalize=True) and the weighted aggregate on the GPU against the
float64 dense form of tests/gcn_norm_ref.py.

Bar: ``out``, ``dx``, ``dW`` and ``db`` each pass tests/gradbar.py's
``assert_wgrad`` (max|err| <= 1e-5 max|ref|, the project's fp32 bar) over the
whole case table -- every N with every width pair, every graph kind and every
(add_self_loops, weighted) combination, ``x`` read through a NaN-padded
leading dimension.  With NGNN_GRAD_LOG the measured ratios are appended to
that file, the case table's as one line per shape: each tensor's worst ratio
over the shape's 28 cases (profiles/gcn_norm_errors.jsonl is one such run).
"""
import contextlib
import os
from unittest import mock

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gcn_norm_ref as R
import ngnn
from gradbar import _log_fields, assert_wgrad, grad_ratio
from ngnn import _lib, fused, models, ops

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _conv(W, b, loops=True, normalize=True):
    conv = ngnn.GCNConv(W.size(1), W.size(0), normalize=normalize,
                        add_self_loops=loops if normalize else None).to(DEV)
    with torch.no_grad():
        conv.lin.weight.copy_(W)
        conv.bias.copy_(b)
    return conv


def _padded(x, pad=3):
    """x on the device as a view of a wider NaN-filled buffer."""
    buf = torch.full((x.size(0), x.size(1) + pad), float("nan"), device=DEV)
    buf[:, :x.size(1)] = x.to(DEV)
    return buf[:, :x.size(1)]


def _run(conv, x, ei, ew, dout, padded=True):
    xd = (_padded(x) if padded else x.to(DEV)).detach().requires_grad_(True)
    conv.zero_grad(set_to_none=True)
    args = (xd, ei.to(DEV)) + ((ew.to(DEV),) if ew is not None else ())
    out = conv(*args)
    out.backward(dout.to(DEV))
    torch.cuda.synchronize()
    return out.detach(), xd.grad, conv.lin.weight.grad, conv.bias.grad


@pytest.mark.parametrize("N,widths", R.shapes(), ids=lambda v: str(v).replace(" ", ""))
def test_conv_matches_the_float64_dense_form(N, widths):
    worst = {}  # tensor -> (ratio, case): one log line per shape, not one per comparison
    log = os.environ.pop("NGNN_GRAD_LOG", None)
    try:
        for kind, mode in R.graph_modes():
            loops, _ = mode
            ei, ew, x, W, b, dout = R.make_case(kind, N, widths, mode, seed=N + widths[0])
            want = R.dense_gcn_conv(x, ei, ew, W, b, add_self_loops=loops, dout=dout)
            got = _run(_conv(W, b, loops), x, ei, ew, dout)
            for name, g, w in zip(("out", "dx", "dW", "db"), got, want):
                w = torch.from_numpy(np.ascontiguousarray(w))
                case = f"{kind} loops={mode[0]} weighted={mode[1]}"
                assert_wgrad(g, w, f"{name} N={N} {widths} {case}")
                err, ref = grad_ratio(g, w)
                if ref > 0 and err / ref >= worst.get(name, (0.0, ""))[0]:
                    worst[name] = (err / ref, case)
    finally:
        if log is not None:
            os.environ["NGNN_GRAD_LOG"] = log
    _log_fields(N=N, widths=list(widths), cases=len(R.graph_modes()), bar=1e-5,
                worst_ratio={k: float(f"{v[0]:.3e}") for k, v in worst.items()},
                worst_case={k: v[1] for k, v in worst.items()})


def test_unnormalised_weighted_matches_a_weighted_index_add():
    for kind in ("unsorted", "self_loops", "target_sorted"):
        ei, ew, x, W, b, dout = R.make_case(kind, 300, (100, 47), (False, True), seed=9)
        want = R.dense_gcn_conv(x, ei, ew, W, b, add_self_loops=False, normalize=False, dout=dout)
        # the same numbers from the op the issue names: a weighted index_add_
        z = x.double() @ W.double().T
        ia = torch.zeros(300, 47, dtype=torch.float64).index_add_(
            0, ei[1], z.index_select(0, ei[0]) * ew.double().unsqueeze(1)) + b.double()
        np.testing.assert_allclose(ia.numpy(), want[0], rtol=0, atol=1e-12 * np.abs(want[0]).max())
        got = _run(_conv(W, b, normalize=False), x, ei, ew, dout)
        for name, g, w in zip(("out", "dx", "dW", "db"), got, want):
            assert_wgrad(g, torch.from_numpy(np.ascontiguousarray(w)), f"weighted-sum {name} {kind}")


@pytest.mark.parametrize("sort_by", ["source", "target"])
@pytest.mark.parametrize("loops", [True, False])
def test_column_slice_edge_weight(sort_by, loops):
    """``edge_weight`` as a column of an ``edge_attr`` matrix (stride 3): both
    CSR orders read its dense copy, also where an order is the identity
    (edges already sorted by that end) and nothing is permuted."""
    ei, _, x, W, b, dout = R.make_case("unsorted", 300, (100, 47), (loops, True), seed=6)
    ei = ei[:, torch.argsort(ei[0 if sort_by == "source" else 1], stable=True)]
    g = torch.Generator().manual_seed(8)
    attr = 0.1 + 1.9 * torch.rand(ei.size(1), 3, generator=g)
    ew = attr[:, 1]
    want = R.dense_gcn_conv(x, ei, ew, W, b, add_self_loops=loops, dout=dout)
    ewd = attr.to(DEV)[:, 1]
    assert ewd.stride(0) == 3
    block = ngnn.get_block(ei.to(DEV), 300)
    assert (block.edge_order(transposed=True) is None) == (sort_by == "source")
    assert (block.edge_order() is None) == (sort_by == "target")
    conv = _conv(W, b, loops)
    xd = _padded(x).detach().requires_grad_(True)
    out = conv(xd, block, ewd)
    out.backward(dout.to(DEV))
    for name, got, w in zip(("out", "dx", "dW", "db"), (out, xd.grad, conv.lin.weight.grad, conv.bias.grad), want):
        assert_wgrad(got, torch.from_numpy(np.ascontiguousarray(w)), f"strided-w {name} {sort_by} loops={loops}")
    # the public op's gradient too
    norm = ops.gcn_norm(block, ewd, add_self_loops=loops)
    z = torch.randn(300, 16, generator=g).to(DEV).requires_grad_(True)
    gz = torch.randn(300, 16, generator=g)
    ops.gcn_propagate(z, block, norm).backward(gz.to(DEV))
    A = R.dense_adj(ei, ew, 300, add_self_loops=loops)
    assert_wgrad(z.grad, torch.from_numpy(A.T @ gz.double().numpy()), f"strided-w propagate dz {sort_by}")


def _ulps(got, want64):
    want = want64.astype(np.float32)
    return np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want)).astype(np.float64)


@pytest.mark.parametrize("kind", ["tail_isolated", "self_loops", "hub", "empty"])
@pytest.mark.parametrize("loops,weighted", R.MODES)
def test_norm_entry_through_ctypes(kind, loops, weighted):
    N = 300
    ei = R.make_graph(kind, N, seed=4)
    if weighted:
        ei = R.one_loop_per_node(ei)
    g = torch.Generator().manual_seed(5)
    ew = (0.1 + 1.9 * torch.rand(ei.size(1), generator=g)) if weighted else None
    block = ngnn.Block(ei.to(DEV), N)
    order = block.edge_order()
    w = None
    if weighted:
        w = ew.to(DEV)
        w = w if order is None else w.index_select(0, order)
    dinv = torch.full((N,), -7.0, device=DEV)
    loop_w = torch.full((N,), -7.0, device=DEV)
    rc = _lib.load().ngnn_gcn_norm(_lib.ptr(block.rowptr), _lib.ptr(block.col), _lib.ptr(w), N, int(loops),
                                   _lib.ptr(dinv), _lib.ptr(loop_w) if loops else None,
                                   _lib.stream_handle(DEV))
    assert rc == 0
    torch.cuda.synchronize()
    # float64 degrees straight from the edge list
    deg = np.zeros(N)
    lw = np.ones(N)
    wv = ew.double().tolist() if weighted else [1.0] * ei.size(1)
    for s, t, v in zip(ei[0].tolist(), ei[1].tolist(), wv):
        if loops and s == t:
            if weighted:
                lw[s] = v
        else:
            deg[t] += v
    if loops:
        deg += lw
        assert np.array_equal(loop_w.cpu().numpy().astype(np.float64), lw)  # exact
    else:
        assert bool((loop_w == -7.0).all())  # not written
    got = dinv.cpu().numpy()
    zero = deg == 0
    assert np.all(got[zero] == 0.0)
    if not loops and kind in ("tail_isolated", "empty"):
        assert zero.any()
    if (~zero).any():
        u = _ulps(got[~zero], deg[~zero] ** -0.5)
        assert u.max() <= 2.0, u.max()


def test_two_calls_are_bitwise_equal():
    ei, ew, x, W, b, dout = R.make_case("hub", 1025, (100, 47), (True, True), seed=2)
    conv = _conv(W, b)
    first = [t.clone() for t in _run(conv, x, ei, ew, dout)]
    ngnn.block.block_cache.clear()
    again = _run(conv, x, ei, ew, dout)
    for a, c in zip(first, again):
        assert torch.equal(a, c)


def _no_gemm():
    """As tests/test_gpu_perconv.py: torch's GEMM entry points raise."""
    def boom(*a, **k):
        raise AssertionError("library GEMM called on the normalised GCN path")
    return [mock.patch.object(F, "linear", boom), mock.patch.object(torch, "matmul", boom),
            mock.patch.object(torch, "mm", boom), mock.patch.object(torch, "addmm", boom),
            mock.patch.object(torch, "bmm", boom)]


@pytest.fixture(scope="module")
def sampled():
    from ngnn.loader import sample_block, synthetic_graph
    g = synthetic_graph("ogbn-products", DEV, seed=3, scale=0.01)
    return sample_block(g, g.train_idx[:256], [10, 5], seed=4)


def test_training_step_issues_no_library_gemm(sampled):
    b = sampled
    torch.manual_seed(0)
    m = ngnn.SimpleGCN(b.x.size(1), 64, 47, 2, dropout=0.0, normalize=True).to(DEV).train()
    with contextlib.ExitStack() as st:
        for p in _no_gemm():
            st.enter_context(p)
        x = b.x.clone().requires_grad_(True)
        out = m(x, b.edge_index)
        F.cross_entropy(out[:b.batch_size], b.y[:b.batch_size]).backward()
        torch.cuda.synchronize()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in m.parameters())
    assert x.grad is not None and torch.isfinite(x.grad).all()


class _RefConv(torch.nn.Module):
    def __init__(self, conv):
        super().__init__()
        self.weight = torch.nn.Parameter(conv.lin.weight.detach().double().cpu().clone())
        self.bias = torch.nn.Parameter(conv.bias.detach().double().cpu().clone())

    def forward(self, x, ei):
        return R.pyg_gcn_conv(x, ei, None, self.weight, self.bias)


class _RefGCN(torch.nn.Module):
    """SimpleGCN(normalize=True, dropout=0) on the host restatement, float64."""

    def __init__(self, model):
        super().__init__()
        self.convs = torch.nn.ModuleList(_RefConv(c) for c in model.convs)

    def forward(self, x, ei):
        for i, c in enumerate(self.convs):
            x = c(x, ei)
            if i != len(self.convs) - 1:
                x = x.relu()
        return x


def _tie_sync(mine, ref):
    """As tests/test_gpu_perconv.py: the reference's ReLU sees the kernel's
    sign where a conv output is within fp32 rounding of zero."""
    seen = []
    hooks = [c.register_forward_hook(lambda m, a, o: seen.append(o.detach().double().cpu()))
             for c in mine.convs]
    at = [0]

    def sync(m, a, o):
        k = seen[at[0]]
        at[0] += 1
        tie = (o.abs() < 1e-6) & ((o > 0) != (k > 0))
        return o + torch.where(tie, k - o, torch.zeros_like(o)).detach()
    return hooks, [c.register_forward_hook(sync) for c in ref.convs]


@pytest.mark.parametrize("layers", [2, 3])
def test_simple_gcn_stack_against_the_host_restatement(sampled, layers):
    b = sampled
    torch.manual_seed(layers)
    m = ngnn.SimpleGCN(b.x.size(1), 64, 47, layers, dropout=0.0, normalize=True).to(DEV).train()
    ref = _RefGCN(m)
    mh, rh = _tie_sync(m, ref)
    calls = []
    lib = _lib.load()
    real = lib.ngnn_gcn_norm
    try:
        with mock.patch.object(lib, "ngnn_gcn_norm", lambda *a: (calls.append(1), real(*a))[1]):
            ngnn.block.block_cache.clear()
            x = b.x.clone().requires_grad_(True)
            out = m(x, b.edge_index)
            F.cross_entropy(out[:b.batch_size], b.y[:b.batch_size]).backward()
            torch.cuda.synchronize()
        # one degree pass per block, shared by every layer and the backward
        assert len(calls) == 1
        xr = b.x.double().cpu().requires_grad_(True)
        out_r = ref(xr, b.edge_index.cpu())
        F.cross_entropy(out_r[:b.batch_size], b.y[:b.batch_size].cpu()).backward()
    finally:
        for h in mh + rh:
            h.remove()
    assert_wgrad(out, out_r, f"stack{layers} out")
    assert_wgrad(x.grad, xr.grad, f"stack{layers} dx")
    for (name, p), c in zip(m.named_parameters(), [q for cv in ref.convs for q in (cv.bias, cv.weight)]):
        assert p.shape == c.shape, name
        assert_wgrad(p.grad, c.grad, f"stack{layers} {name}")


def test_inference_takes_the_loop_plan_and_matches_the_host_loop():
    from ngnn.loader import NeighborLoader, synthetic_graph
    g = synthetic_graph("ogbn-products", DEV, seed=3, scale=0.002)
    torch.manual_seed(1)
    m = ngnn.SimpleGCN(g.x.size(1), 32, 16, 2, dropout=0.0, normalize=True).to(DEV).eval()
    ref = _RefGCN(m)
    loader = NeighborLoader(g, None, num_neighbors=[10, 5], batch_size=128, seed=5)
    models.last_inference_plan[:] = []
    out = m.inference(g.x, loader, DEV)
    assert models.last_inference_plan == ["loop"] * 2
    twin = NeighborLoader(g, None, num_neighbors=[10, 5], batch_size=128, seed=5)  # one pass per layer, as m's
    with torch.no_grad():
        x_cur = g.x.double().cpu()
        for i, conv in enumerate(ref.convs):
            xs = []
            for batch in twin:
                h = conv(x_cur.index_select(0, batch.n_id.cpu()), batch.edge_index.cpu())[:batch.batch_size]
                xs.append(h.relu() if i == 0 else h)
            x_cur = torch.cat(xs, dim=0)
    torch.testing.assert_close(out.double().cpu(), x_cur, rtol=1e-5, atol=1e-5)


def test_unnormalised_unweighted_still_takes_the_fused_path(sampled):
    b = sampled
    lib = _lib.load()
    new = []
    real_n, real_w = lib.ngnn_gcn_norm, lib.ngnn_gcn_wagg
    with mock.patch.object(lib, "ngnn_gcn_norm", lambda *a: (new.append("norm"), real_n(*a))[1]), \
            mock.patch.object(lib, "ngnn_gcn_wagg", lambda *a: (new.append("wagg"), real_w(*a))[1]), \
            mock.patch.object(fused, "gcn_conv", wraps=fused.gcn_conv) as one, \
            mock.patch.object(fused, "gcn_stack", wraps=fused.gcn_stack) as stack:
        conv = ngnn.GCNConv(b.x.size(1), 47).to(DEV)
        conv(b.x, b.edge_index).sum().backward()
        assert one.call_count == 1
        m = ngnn.SimpleGCN(b.x.size(1), 64, 47, 2).to(DEV)
        assert fused.gcn_stack_supported(m, b.x)
        m(b.x, b.edge_index).sum().backward()
        assert stack.call_count == 1
        torch.cuda.synchronize()
    assert new == []
    # ... and a normalised model is outside every fused stack and the slot
    mn = ngnn.SimpleGCN(b.x.size(1), 64, 47, 2, normalize=True).to(DEV)
    assert not fused.gcn_stack_supported(mn, b.x)
    assert not fused.conv_supported(mn.convs[0], b.x)
    assert not fused.zero_copy_ok(mn, 4096, 100)


def test_refusals():
    N = 50
    ei = R.make_graph("unsorted", N, seed=1).to(DEV)
    E = ei.size(1)
    x = torch.randn(N, 8, device=DEV)
    conv = ngnn.GCNConv(8, 4, normalize=True).to(DEV)
    with pytest.raises(ValueError):
        conv(x, ei, torch.ones(E + 1, device=DEV))
    with pytest.raises(ValueError):
        conv(x, ei, torch.ones(E, 1, device=DEV))
    with pytest.raises(TypeError):
        conv(x, ei, torch.ones(E, device=DEV, dtype=torch.float64))
    with pytest.raises(RuntimeError):
        conv(x, ei, torch.ones(E))
    with pytest.raises(NotImplementedError):
        conv(x, ei, torch.ones(E, device=DEV, requires_grad=True))
    with pytest.raises(TypeError):
        conv(x.bfloat16(), ei)
    # an out-of-range id: IndexError from the block, before any new kernel runs
    lib = _lib.load()
    ran = []
    real_n, real_w = lib.ngnn_gcn_norm, lib.ngnn_gcn_wagg
    bad = ei.clone()
    bad[0, 3] = N
    with mock.patch.object(lib, "ngnn_gcn_norm", lambda *a: (ran.append(1), real_n(*a))[1]), \
            mock.patch.object(lib, "ngnn_gcn_wagg", lambda *a: (ran.append(1), real_w(*a))[1]):
        with pytest.raises(IndexError):
            conv(x, bad)
        with pytest.raises(IndexError):
            ops.gcn_norm(bad, num_nodes=N)
    assert ran == []
    from ngnn.graphs import GraphedTrainStep
    m = ngnn.SimpleGCN(8, 8, 4, 2, normalize=True).to(DEV)
    opt = torch.optim.Adam(m.parameters(), capturable=True)
    with pytest.raises(ValueError, match="convs.0"):
        GraphedTrainStep(m, opt, 4, 64, 256, 8, DEV)


def test_no_grad_forward_saves_nothing_and_propagate_matches():
    ei, ew, x, W, b, dout = R.make_case("self_loops", 300, (7, 5), (True, True), seed=3)
    conv = _conv(W, b)
    with torch.no_grad():
        out = conv(_padded(x), ei.to(DEV), ew.to(DEV))
    assert out.grad_fn is None and not out.requires_grad
    want = R.dense_gcn_conv(x, ei, ew, W, b)
    assert_wgrad(out, torch.from_numpy(want), "no_grad out")
    # the public op, transform-first by hand: A^ (x W^T) + b, and its gradient
    block = ngnn.get_block(ei.to(DEV), 300)
    ewd = ew.to(DEV)
    norm = ops.gcn_norm(block, ewd)
    assert ops.gcn_norm(block, ewd) is norm  # cached on the block, keyed by the tensor
    assert ops.gcn_norm(block, ewd.clone()) is not norm
    z = (x.double() @ W.double().T).float().to(DEV).requires_grad_(True)
    bias = b.to(DEV).requires_grad_(True)
    o2 = ops.gcn_propagate(z, block, norm, bias)
    o2.backward(dout.to(DEV))
    A = R.dense_adj(ei, ew, 300)
    assert_wgrad(o2, torch.from_numpy(want), "propagate out")
    assert_wgrad(z.grad, torch.from_numpy(A.T @ dout.double().numpy()), "propagate dz")
    assert_wgrad(bias.grad, dout.double().sum(0), "propagate db")
