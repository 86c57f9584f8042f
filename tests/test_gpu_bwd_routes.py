"""Which input-gradient kernel each layer of a SAGE stack takes in backward,
and that every route computes the oracle's gradients.

The per-layer backward picks, per (F_out, K, reduce, deterministic), one of
four routes (ngnn_sage_dgrad_route): the low-dimensional MFMA pass, the
fused per-row kernel, or the dgrad GEMM followed by the atomic scatter or the
source-grouped gather.  Each case below names the routes its layers take
(layer 0 first); the spans recorded under a KernelTimer must be exactly
those, and x.grad and every parameter gradient must match
oracle.pyg_ref.SAGE at the bars tests/test_gpu_fused.py uses.  x requires a
gradient, so layer 0's input gradient runs and the two-layer kernel is not
taken.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

import ngnn
from ngnn import _lib, _timing
from oracle import pyg_ref
from gradbar import assert_wgrad
from test_gpu_fused import GRAD, rand_block

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
N, E, SEEDS = 300, 2000, 64

LOWDIM, FUSED = "sage_dgrad_lowdim", "sage_dgrad_fused"
GEMM, SCATTER, GATHER = "sage_dgrad", "sage_dgrad_scatter", "sage_dgrad_gather"


@functools.lru_cache(maxsize=None)
def _case(dims, aggr):
    """(edges, x, labels, state dict, oracle's dx, oracle's parameter gradients)
    of one stack: built once, shared by the cases with the same dims."""
    K0, H, C, L = dims
    ei = rand_block(K0 + H + C, N, E)
    g = torch.Generator().manual_seed(K0 * 7 + H)
    x = torch.randn(N, K0, generator=g)
    y = torch.randint(0, C, (SEEDS,), generator=g)
    torch.manual_seed(L)
    ref = pyg_ref.SAGE(K0, H, C, L, dropout=0.5, aggr=aggr).eval()
    xr = x.clone().requires_grad_(True)
    F.cross_entropy(ref(xr, ei)[:SEEDS], y).backward()
    state = {k: v.detach().clone() for k, v in ref.state_dict().items()}
    return ei, x, y, state, xr.grad, [(k, q.grad) for k, q in ref.named_parameters()]


# the two stacks with a layer inside lowdim's rule (Fo < K, sum / mean) that
# the entry refuses: dims -> that layer's (Fo, K)
REFUSED = {(16, 300, 33, 2): (33, 300), (16, 500, 47, 2): (47, 500)}


def _run(dims, aggr, deterministic):
    """Forward and backward of the stack on the GPU under a KernelTimer:
    (its sage_dgrad* span names, x with its gradient, the model)."""
    ei, x, y, state = _case(dims, aggr)[:4]
    mine = ngnn.SAGE(*dims, dropout=0.5, aggr=aggr).to(DEV).eval()
    mine.load_state_dict({k: v.to(DEV) for k, v in state.items()})
    xd = x.to(DEV).requires_grad_(True)
    prev = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(deterministic)
    try:
        with _timing.KernelTimer() as timer:
            out = mine(xd, ei.to(DEV))
            F.cross_entropy(out[:SEEDS], y.to(DEV)).backward()
    finally:
        torch.use_deterministic_algorithms(prev)
    torch.cuda.synchronize()
    return {r.name for r in timer.recs if r.name.startswith("sage_dgrad")}, xd, mine


@pytest.mark.parametrize("dims,aggr,deterministic,spans", [
    # layer 0 lowdim (64 < 100), layer 1 fused (64 = 64), layer 2 lowdim (47 < 64)
    ((100, 64, 47, 3), "mean", False, {LOWDIM, FUSED}),
    # max never takes lowdim
    ((100, 64, 47, 3), "max", False, {FUSED}),
    # layer 0: 160 x 128 weights exceed the fused kernel's LDS budget; layer 1 lowdim
    ((128, 160, 10, 2), "mean", False, {GEMM, SCATTER, LOWDIM}),
    # layer 1: lowdim refuses Fo = 33, K = 300; the weights fit the fused kernel
    ((16, 300, 33, 2), "sum", False, {FUSED}),
    # layer 1: lowdim refuses Fo = 47, K = 500, and the weights are too big for fused
    ((16, 500, 47, 2), "mean", False, {FUSED, GEMM, SCATTER}),
    # deterministic mode: the GEMM and the source-grouped gather on every layer
    ((100, 64, 47, 3), "mean", True, {GEMM, GATHER}),
])
def test_backward_routes(dims, aggr, deterministic, spans):
    dx_ref, wgrads_ref = _case(dims, aggr)[4:]
    got, xd, mine = _run(dims, aggr, deterministic)
    if dims in REFUSED:
        # a backward that finds lowdim's envelope by calling the entry records
        # a span around the refused call: no launch is inside it
        got.discard(LOWDIM)
    assert got == spans, (got, spans)
    torch.testing.assert_close(xd.grad.cpu(), dx_ref, **GRAD)
    params = dict(mine.named_parameters())
    assert list(params) == [k for k, _ in wgrads_ref]
    for k, want in wgrads_ref:
        assert_wgrad(params[k].grad.cpu(), want, msg=k)


@pytest.mark.parametrize("dims,aggr", [((16, 300, 33, 2), "sum"), ((16, 500, 47, 2), "mean")])
def test_refused_lowdim_layer_is_not_entered(dims, aggr):
    """A layer lowdim refuses goes straight to its route: no
    sage_dgrad_lowdim span, and none of that entry's zero-filled per-shape
    workspace."""
    from ngnn import fused
    Fo, K = REFUSED[dims]
    assert _lib.load().ngnn_sage_dgrad_route(Fo, K, _lib.REDUCE[aggr], 0) != _lib.DGRAD_LOWDIM
    got, _, _ = _run(dims, aggr, False)
    assert LOWDIM not in got
    assert not any(key[1] == ("dgrad_lowdim", Fo, K) for key in fused._ws)
