"""ngnn.SAGEH and the tapped fused stack (fused.sage_stack_tap) on the device:
the reference's own fixtures (tests/golden/sageh_*.npz), the logits bit for
bit those of ngnn.SAGE, where dropout sits relative to the returned hidden
state, the route taken inside the two-layer envelope, training steps with
gradients through either or both outputs against the fp64 restatement
(tests/sageh_ref.py) fed the host replica of the hash mask, which `training`
rules the dropout, SAGEPL(fused_stack=True) against the per-conv path, and
what the tapped stack refuses."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ngnn
from ngnn import fused
from ngnn.block import Block
from ngnn.loader import sample_block

import sageh_ref
import sagepl_ref
from gradbar import assert_wgrad
from test_gpu_fused import dropout_keep, dropout_scale
from test_sageh_cpu import CASES, load_case
from test_sagepl_cpu import load_case as load_pl_case
from test_sagepl_gpu import small_graph

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
TOL = dict(rtol=1e-5, atol=1e-5)  # the project's forward bar (test_sagepl_gpu.TOL)


def _conv_state(m):
    return {k: v for k, v in m.state_dict().items() if k.startswith("convs.")}


def _host_seed(s):
    """The hash-dropout seed a model draws right after torch.manual_seed(s) (models._dropout_seed)."""
    torch.manual_seed(s)
    return int(torch.randint(0, 2**62, (1,)).item())


def _keeps(seed, n, widths, p):
    return [dropout_keep(seed + 7919 * i, n, w, p) for i, w in enumerate(widths)]


def _ref64(m, sizes, p):
    ref = sageh_ref.SAGEH(*sizes, dropout=p)
    ref.load_state_dict({k: v.detach().cpu() for k, v in m.state_dict().items()}, strict=True)
    return ref.double()


# ------------------------------------------------------------------ fixtures
@pytest.mark.parametrize("name", sorted(CASES))
def test_reference_fixture(golden_dir, name):
    rec, state = load_case(golden_dir, name)
    m = ngnn.SAGEH(*CASES[name]["sizes"], dropout=0.0)
    m.load_state_dict(state, strict=True)
    m.to(DEV)
    out, h = m(torch.as_tensor(rec["x"]).to(DEV), torch.as_tensor(rec["edge_index"]).to(DEV),
               training=bool(rec["meta/training"]))
    torch.testing.assert_close(out.detach().cpu(), torch.as_tensor(rec["out/out"]), **TOL)
    torch.testing.assert_close(h.detach().cpu(), torch.as_tensor(rec["out/h"]), **TOL)
    sageh_ref.fixture_loss(out, h, rec).backward()
    for k, p in m.named_parameters():
        if k.startswith("convs."):
            assert_wgrad(p.grad, torch.as_tensor(rec["grad/" + k]), msg=k)
        else:
            assert p.grad is None, k


# ------------------------------------------------- logits: SAGE's, bit for bit
@pytest.mark.parametrize("sizes", [(24, 16, 5, 2), (24, 32, 5, 3)])
@pytest.mark.parametrize("p", [0.5, 0.3])
def test_logits_are_sages_bitwise(sizes, p):
    g = small_graph(300, 24, 5, seed=11)
    blk = sample_block(g, torch.arange(40, device=DEV), [4, 3], seed=3)
    torch.manual_seed(2)
    sage = ngnn.SAGE(*sizes, dropout=p).to(DEV).train()
    sh = ngnn.SAGEH(*sizes, dropout=p).to(DEV).train()
    sh.load_state_dict(_conv_state(sage), strict=False)
    calls = fused.eager_ext_calls
    for s in (5, 6):
        torch.manual_seed(s)
        want = sage(blk.x, blk.edge_index)
        torch.manual_seed(s)
        got, h = sh(blk.x, blk.edge_index)
        assert torch.equal(got, want), f"seed {s}"
        assert tuple(h.shape) == (blk.x.size(0), sizes[1])
    assert fused.eager_ext_calls == calls  # (outside the two-layer envelope)
    torch.manual_seed(7)
    assert not torch.equal(sh(blk.x, blk.edge_index)[0], got)  # another seed, another mask


# ------------------------------------------------------- h is pre-dropout
def test_hidden_state_is_returned_before_dropout():
    g = small_graph(200, 24, 5, seed=7)
    blk = sample_block(g, torch.arange(32, device=DEV), [4, 3], seed=2)
    torch.manual_seed(5)
    p = 0.5
    m = ngnn.SAGEH(24, 32, 5, 3, dropout=p).to(DEV)
    out_ev, h_ev = m(blk.x, blk.edge_index, training=False)
    fused._debug_acts = []
    try:
        seed = _host_seed(9)
        torch.manual_seed(9)
        out_tr, h_tr = m(blk.x, blk.edge_index, training=True)
        acts = fused._debug_acts[-1]
    finally:
        fused._debug_acts = None
    # layer 0's dropout differs between the two calls, so h itself is compared
    # on a two-layer twin below; here: its sign pattern and what follows it
    assert bool((h_tr >= 0).all()) and bool((h_tr == 0).any()) and bool((h_tr > 0).any())
    xd = acts[-1]  # what the output layer read
    keep = dropout_keep(seed + 7919, h_tr.size(0), 32, p).to(DEV)
    assert torch.equal(xd, torch.where(keep, h_tr * dropout_scale(p), torch.zeros_like(h_tr)))
    assert bool(((xd == 0) & (h_tr > 0)).any())  # at least one element dropped
    assert not torch.allclose(out_tr, out_ev, rtol=1e-3, atol=1e-3)
    m2 = ngnn.SAGEH(24, 32, 5, 2, dropout=p).to(DEV)
    with torch.no_grad():
        _, h_ev = m2(blk.x, blk.edge_index, training=False)
        z_tr, h_tr = m2(blk.x, blk.edge_index, training=True)
    torch.testing.assert_close(h_tr, h_ev, rtol=1e-6, atol=1e-6)  # no element rescaled or dropped
    assert float(h_ev.abs().max()) > 0 and bool((h_ev == 0).any())
    assert not torch.allclose(z_tr, m2(blk.x, blk.edge_index, training=False)[0].detach(), rtol=1e-3, atol=1e-3)


# ------------------------------------------------ inside the two-layer envelope
def test_two_layer_envelope_takes_the_per_layer_route():
    sizes, p = (128, 256, 40, 2), 0.5
    g = small_graph(600, 128, 40, seed=13)
    blk = sample_block(g, torch.arange(64, device=DEV), [5, 3], seed=4)
    n = blk.x.size(0)
    assert 200 <= n <= 600
    torch.manual_seed(3)
    m = ngnn.SAGEH(*sizes, dropout=p).to(DEV)
    sage = ngnn.SAGE(*sizes, dropout=p).to(DEV).train()
    sage.load_state_dict(_conv_state(m), strict=True)
    calls = fused.eager_ext_calls
    sage(blk.x, blk.edge_index)
    in_envelope = fused.eager_ext_calls == calls + 1  # (the C++ node, when it is built)
    calls = fused.eager_ext_calls
    seed = _host_seed(21)
    torch.manual_seed(21)
    out, h = m(blk.x, blk.edge_index)
    assert fused.eager_ext_calls == calls
    print(f"SAGE on this shape used the eager two-layer node: {in_envelope}")
    ref = _ref64(m, sizes, p)
    with torch.no_grad():
        out_r, h_r = ref(blk.x.cpu().double(), blk.edge_index.cpu(), keeps=_keeps(seed, n, [256], p),
                         scale=dropout_scale(p))
    torch.testing.assert_close(out.detach().cpu().double(), out_r, **TOL)
    torch.testing.assert_close(h.detach().cpu().double(), h_r, **TOL)


# ------------------------------------------- training steps through the tap
B, FAN, C = 16, [4, 3], 5
LOSSES = ("both", "past_bound", "h_only", "logits_only")


def _loss(kind, out, h, y, idx):
    ce = F.cross_entropy(out[:B], y)
    if kind == "both":
        return ce + 0.1 * h[idx].pow(2).mean()
    if kind == "past_bound":  # the last block row: a two-hop node no seed row's edge reads
        return ce + h[-1].pow(2).sum() + h[-1].sum()
    if kind == "h_only":
        return h[idx].pow(2).mean()
    return ce


@pytest.mark.parametrize("kind", LOSSES)
@pytest.mark.parametrize("sizes,p", [((24, 16, C, 2), 0.3), ((24, 32, C, 3), 0.5)])
def test_training_step_matches_fp64(sizes, p, kind):
    g = small_graph(300, 24, C, seed=3)
    blk = sample_block(g, torch.randperm(300, generator=torch.Generator().manual_seed(4))[:B].to(DEV), FAN, seed=9)
    n, L = blk.x.size(0), sizes[3]
    ei = blk.edge_index.cpu()
    # the premise of "past_bound": the output layer reads no row that far
    assert int(ei[0][ei[1] < B].max()) + 1 < n and n - 1 >= B
    y = torch.randint(0, C, (B,), generator=torch.Generator().manual_seed(8))
    idx = torch.tensor([0, 3, B - 1])
    torch.manual_seed(12)
    f = ngnn.NGNN(in_size=sizes[0], hidden_size=sizes[1], out_size=C, num_layers=L, dropout=p, module="sageH")
    m = f.network.to(DEV).train()
    seed = _host_seed(31)
    torch.manual_seed(31)
    out, h = m(blk.x, blk.edge_index)
    loss = _loss(kind, out, h, y.to(DEV), idx.to(DEV))
    loss.backward()
    ref = _ref64(m, sizes, p)
    out_r, h_r = ref(blk.x.cpu().double(), ei, keeps=_keeps(seed, n, [sizes[1]] * (L - 1), p),
                     scale=dropout_scale(p))
    loss_r = _loss(kind, out_r, h_r, y, idx)
    loss_r.backward()
    torch.testing.assert_close(out.detach().cpu().double(), out_r.detach(), **TOL)
    torch.testing.assert_close(h.detach().cpu().double(), h_r.detach(), **TOL)
    assert abs(float(loss.detach()) - float(loss_r.detach())) <= 1e-5 * max(1.0, abs(float(loss_r.detach())))
    for (k, q), (_, r) in zip(m.named_parameters(), ref.named_parameters()):
        if r.grad is None:  # act / bnl; the output layer under "h_only"
            assert q.grad is None or not bool(q.grad.any()), k
            assert not k.startswith("convs.") or (kind == "h_only" and k.startswith(f"convs.{L - 1}.")), k
        else:
            assert_wgrad(q.grad, r.grad, msg=f"{kind} {k}")
    before = [q.detach().clone() for q in m.convs.parameters()]
    f.optimizer.step()  # NGNN(module='sageH') trains a step on the device
    moved = [not torch.equal(a, q.detach()) for a, q in zip(before, m.convs.parameters())]
    assert all(moved[:3 * (L - 1)]) and (kind == "h_only" or all(moved))


def test_training_argument_rules_the_dropout():
    g = small_graph(200, 24, C, seed=7)
    blk = sample_block(g, torch.arange(32, device=DEV), FAN, seed=2)
    torch.manual_seed(5)
    m = ngnn.SAGEH(24, 32, C, 2, dropout=0.5).to(DEV)
    m.eval()
    base = m(blk.x, blk.edge_index, training=False)[0]
    m.train()
    assert torch.equal(m(blk.x, blk.edge_index, training=False)[0], base)  # no dropout, no seed drawn
    state = torch.random.get_rng_state()
    m(blk.x, blk.edge_index, training=False)
    assert torch.equal(torch.random.get_rng_state(), state)
    m.eval()
    dropped = m(blk.x, blk.edge_index, training=True)[0]
    assert not torch.allclose(dropped, base, rtol=1e-3, atol=1e-3)
    assert not torch.equal(torch.random.get_rng_state(), state)  # the seed was drawn
    assert not torch.allclose(m(blk.x, blk.edge_index)[0], base, rtol=1e-3, atol=1e-3)  # the default: True


# --------------------------------------------------- SAGEPL(fused_stack=True)
def test_sagepl_fused_stack_matches_per_conv_path():
    g = small_graph(300, 24, C, seed=3)
    blk = sample_block(g, torch.arange(B, device=DEV), FAN, seed=9)
    torch.manual_seed(1)
    a = ngnn.SAGEPL(24, 32, C, 3, nbr_nodes=300, dropout=0.0).to(DEV).train()
    b = ngnn.SAGEPL(24, 32, C, 3, nbr_nodes=300, dropout=0.0, fused_stack=True).to(DEV).train()
    b.load_state_dict(a.state_dict(), strict=True)
    gen = torch.Generator().manual_seed(2)
    outs = []
    for m in (a, b):
        o = m(blk.x, blk.edge_index, noise_rate=0.1, n_id=blk.n_id)
        assert len(o) == 6
        outs.append(o)
    Gs = [torch.randn(o.shape, generator=gen).to(DEV) for o in outs[0]]
    for o in outs:
        sum((t * G).sum() for t, G in zip(o, Gs)).backward()
    for nm, want, got in zip(sagepl_ref.OUT_NAMES, *outs):
        torch.testing.assert_close(got, want, msg=lambda s: f"{nm}: {s}", **TOL)
    rows = blk.n_id
    rest = torch.ones(300, dtype=torch.bool, device=DEV)
    rest[rows] = False
    assert bool((b.noise.grad[rest] == 0).all())
    assert_wgrad(b.noise.grad[rows], a.noise.grad[rows], msg="noise rows")
    for (k, p), (_, q) in zip(b.named_parameters(), a.named_parameters()):
        if k != "noise":
            assert_wgrad(p.grad, q.grad, msg=k)
    # use_bn keeps the per-conv path
    bn = ngnn.SAGEPL(24, 32, C, 2, nbr_nodes=300, dropout=0.0, use_bn=True, fused_stack=True).to(DEV).train()
    assert not fused.sage_tap_supported(bn, blk.x)
    assert len(bn(blk.x, blk.edge_index, n_id=blk.n_id)) == 6


def test_sagepl_block_fixture_through_the_fused_stack(golden_dir):
    """test_sagepl_gpu.test_reference_fixture[sagepl_block] with fused_stack=True, at its bars."""
    rec, state, n_id = load_pl_case(golden_dir, "sagepl_block")
    nbr_nodes = state["noise"].shape[0]
    m = ngnn.SAGEPL(100, 32, 47, 3, nbr_nodes=nbr_nodes, dropout=0.0, fused_stack=True)
    m.load_state_dict(state, strict=True)
    m.to(DEV).eval()
    x = torch.as_tensor(rec["x"]).to(DEV)
    assert fused.sage_tap_supported(m, x)
    outs = m(x, torch.as_tensor(rec["edge_index"]).to(DEV), noise_rate=float(rec["noise_rate"]), n_id=n_id.to(DEV))
    for nm, o in zip(sagepl_ref.OUT_NAMES, outs):
        torch.testing.assert_close(o.detach().cpu(), torch.as_tensor(rec["out/" + nm]), msg=lambda s: f"{nm}: {s}",
                                   **TOL)
    sagepl_ref.fixture_loss(outs, rec).backward()
    gn = m.noise.grad.cpu()
    rest = torch.ones(nbr_nodes, dtype=torch.bool)
    rest[n_id] = False
    assert (gn[rest] == 0).all()
    got, want = gn[n_id], torch.as_tensor(rec["grad/noise_rows"])
    clamped = want.abs().amax(dim=1) > 1e3  # the zero noise row: g * rate / 1e-12
    assert int(clamped.sum()) == 1
    for r in torch.nonzero(clamped).flatten().tolist():
        assert_wgrad(got[r], want[r], msg=f"noise row {r} (clamped)")
    assert_wgrad(got[~clamped], want[~clamped], msg="noise rows")
    for k, p in m.named_parameters():
        if k != "noise":
            assert_wgrad(p.grad, torch.as_tensor(rec["grad/" + k]), msg=k)


class _RowHint(torch.autograd.Function):
    """Identity whose backward marks the gradient as ngnn.losses mark theirs."""

    @staticmethod
    def forward(ctx, h, rows):
        ctx.rows = rows
        return h.view_as(h)

    @staticmethod
    def backward(ctx, g):
        g = g.clone()
        g._ngnn_nonzero_rows = ctx.rows
        return g, None


def test_row_hint_on_the_hidden_gradient_is_honoured():
    """A loss that leaves its _ngnn_nonzero_rows hint on dh (as ngnn.losses do on
    the logits' gradient) gets the gradients of the unhinted run, and no
    ngnn_row_extent launch for dh: a hint that lies (too small) changes them."""
    # a block whose seed rows read sources < 20 only: the output layer's source
    # bound is at most 20, dh reaches row 49
    n, rows, gen = 60, 50, torch.Generator().manual_seed(3)
    dst = torch.sort(torch.randint(0, n, (400,), generator=gen)).values
    src = torch.where(dst < B, torch.randint(0, 20, (400,), generator=gen), torch.randint(0, n, (400,), generator=gen))
    ei = torch.stack([src, dst]).to(DEV)
    x = torch.randn(n, 24, generator=gen).to(DEV)
    torch.manual_seed(4)
    m = ngnn.SAGEH(24, 32, C, 3, dropout=0.0).to(DEV)
    G = torch.randn(rows, 32, generator=gen).to(DEV)

    def grads(hint):
        m.zero_grad(set_to_none=True)
        out, h = m(x, ei)
        if hint is not None:
            h = _RowHint.apply(h, hint)
        (F.cross_entropy(out[:B], torch.zeros(B, dtype=torch.long, device=DEV)) + (h[:rows] * G).sum()).backward()
        return [q.grad.clone() for q in m.convs.parameters()]

    want = grads(None)
    for a, b in zip(grads(rows), want):
        assert_wgrad(a, b, msg="hinted")
    lied = grads(B)  # rows B .. rows - 1 of dh dropped: the hint is what bounds the launches
    assert not torch.allclose(lied[0], want[0], rtol=1e-3, atol=1e-6)


# ---------------------------------------------------------------- refusals
def test_graph_slot_block_raises():
    g = small_graph(200, 24, C, seed=7)
    blk = sample_block(g, torch.arange(16, device=DEV), FAN, seed=2)
    m = ngnn.SAGEH(24, 16, C, 2).to(DEV)
    block = Block(blk.edge_index, blk.x.size(0))
    block.n_rows_dev = torch.tensor([blk.x.size(0)], dtype=torch.int32, device=DEV)
    with pytest.raises(ngnn._lib.NGNNError, match="graph slot"):
        fused.sage_stack_tap(m, blk.x, block, 0)
    with pytest.raises(ngnn._lib.NGNNError):  # outside the envelope: the caller checks sage_tap_supported
        fused.sage_stack_tap(m, blk.x.bfloat16(), Block(blk.edge_index, blk.x.size(0)), 0)
    assert np.isfinite(float(fused.sage_stack_tap(m, blk.x, Block(blk.edge_index, blk.x.size(0)), 0)[0].detach().sum()))
