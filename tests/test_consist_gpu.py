"""ngnn.losses.get_uncertainty_batch and ngnn.losses.fix_cr on the device
against the float64 run of tests/consist_ref.py (pinned to the reference's own
module by tests/test_consist_ref.py) and against the reference-generated
fixtures tests/golden/consist_*.npz.

Bars, the project's (tests/test_noisy_losses_gpu.py): w at rtol = atol = 1e-5;
losses rtol 1e-5, atol 1e-6; gradients by gradbar.assert_wgrad (1e-5 of the
tensor's max); the graph step against the same loop body run eagerly, losses
1e-5, parameters rtol 1e-4, atol 2e-6."""
import copy
import os

import numpy as np
import pytest
import torch

import consist_ref as R
from gradbar import assert_wgrad
from ngnn import _lib
from ngnn.block import get_block
from ngnn.losses import fix_cr, get_uncertainty_batch, seed_cross_entropy

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
NAN = float("nan")
CS = [2, 7, 47, 64, 65, 130]  # below, at and past one 64-lane stride
MODES = {"hard": ("ce", True), "soft": ("ce", False), "l2": ("l2", True)}


def _padded(y, extra_rows=0, pad=0, grad=True):
    """A device leaf [n + extra_rows, C + pad], NaN outside y, and its [:, :C] view."""
    n, C = y.shape
    buf = torch.full((n + extra_rows, C + pad), NAN)
    buf[:n, :C] = y
    leaf = buf.to(DEV).requires_grad_(grad)
    return leaf, leaf[:, :C]


def _close_w(got, want):
    torch.testing.assert_close(got.cpu().double(), want.double(), rtol=1e-5, atol=1e-5)


def _close_loss(got, want):
    torch.testing.assert_close(got.detach().cpu().double().reshape(()), want.detach().double().reshape(()),
                               rtol=1e-5, atol=1e-6, equal_nan=True)


def _ref64(yp, yn, B, mode, cutoff, w, scale=1.0):
    """(loss, d y_pure[:B], d y_noisy[:B]) of the float64 restatement (a
    gradient autograd leaves None: zeros)."""
    nm, hard = MODES[mode]
    a, b = yp.double().requires_grad_(True), yn.double().requires_grad_(True)
    loss = R.fix_cr(a, b, B, nm, cutoff, hard, None if w is None else w.double())
    (loss * scale).backward()
    zero = torch.zeros_like(a)
    ga, gb = (zero if a.grad is None else a.grad), (zero if b.grad is None else b.grad)
    nb = min(B, yp.size(0))
    assert torch.count_nonzero(ga[nb:]) == 0 and torch.count_nonzero(gb[nb:]) == 0
    return loss.detach(), ga[:nb], gb[:nb]


def _fix_cr_check(yp, yn, B, mode, cutoff, w, extra_rows=0, pad=0, scale=None, batch_size=None):
    """fix_cr on NaN-padded leaves against the float64 run; returns the loss."""
    nm, hard = MODES[mode]
    n, C = yp.shape
    lp, vp = _padded(yp, extra_rows, pad)
    ln, vn = _padded(yn, extra_rows, pad)
    wd = None if w is None else torch.cat([w, torch.full((extra_rows,), NAN)]).to(DEV)
    loss = fix_cr(vp, vn, None, batch_size=B if batch_size is None else batch_size, name=nm, p_cutoff=cutoff,
                  use_hard_labels=hard, w=wd)
    want, gp, gn = _ref64(yp, yn, B, mode, cutoff, w, 1.0 if scale is None else scale)
    _close_loss(loss, want)
    (loss if scale is None else loss * scale).backward()
    nb = min(B, n)
    tag = f"fix_cr {mode} B={B} C={C} cutoff={cutoff} w={w is not None}"
    g = ln.grad.cpu()
    assert torch.count_nonzero(g[nb:]) == 0 and torch.count_nonzero(g[:, C:]) == 0
    assert_wgrad(g[:nb, :C], gn, msg=tag + " d y_noisy")
    if mode == "hard":  # nothing flows into y_pure
        assert lp.grad is None or torch.count_nonzero(lp.grad) == 0
    else:
        g = lp.grad.cpu()
        assert torch.count_nonzero(g[nb:]) == 0 and torch.count_nonzero(g[:, C:]) == 0
        assert_wgrad(g[:nb, :C], gp, msg=tag + " d y_pure")
    return loss


# ------------------------------------------------------------------ fixtures

@pytest.mark.parametrize("name", ["consist_b300", "consist_b65"])
def test_vs_reference_fixture(golden_dir, name):
    g = np.load(os.path.join(golden_dir, name + ".npz"))
    t = {k: torch.from_numpy(np.asarray(g[k])) for k in g.files}
    B, C, cutoff = int(t["B"]), int(t["C"]), float(t["p_cutoff"])
    ei, yp, yn = t["edge_index"], t["y_pure"], t["y_noisy"]
    w = get_uncertainty_batch(ei.to(DEV), yp.to(DEV), C, DEV)
    assert w.shape == (yp.size(0),) and w.dtype == torch.float32 and not w.requires_grad
    _close_w(w, t["w"])
    w64 = R.uncertainty(ei, yp.double(), C)
    _close_w(w, w64)
    assert float(w[1]) == 1.0  # the source without out-edges
    for mode, (nm, hard) in MODES.items():
        loss = _fix_cr_check(yp, yn, B, mode, cutoff, w.cpu())
        _close_loss(loss, t[f"{mode}/loss"])
        a, b = yp.to(DEV).requires_grad_(True), yn.to(DEV).requires_grad_(True)
        fix_cr(a, b, None, batch_size=B, name=nm, p_cutoff=cutoff, use_hard_labels=hard, w=w).backward()
        assert torch.count_nonzero(b.grad[B:]) == 0
        assert_wgrad(b.grad.cpu()[:B], t[f"{mode}/grad_noisy"], msg=f"{name} {mode} d y_noisy")
        if mode == "hard":
            assert a.grad is None or torch.count_nonzero(a.grad) == 0
        else:
            assert torch.count_nonzero(a.grad[B:]) == 0
            assert_wgrad(a.grad.cpu()[:B], t[f"{mode}/grad_pure"], msg=f"{name} {mode} d y_pure")
        if mode != "l2":
            kw = dict(batch_size=B, name=nm, use_hard_labels=hard)
            _close_loss(fix_cr(yp.to(DEV), yn.to(DEV), None, p_cutoff=cutoff, **kw), t[f"{mode}/loss_w_none"])
            _close_loss(fix_cr(yp.to(DEV), yn.to(DEV), None, p_cutoff=0.0, w=w, **kw), t[f"{mode}/loss_cutoff0"])


# -------------------------------------------------------- uncertainty shapes

DEGS = [0, 1, 63, 64, 65, 200]  # around the 64-entry list load


def _degree_graph(n, seed):
    """Edges by source: node 0 with 3,000 out-edges, the others cycling through
    DEGS (node 1: none), plus one duplicate edge and one self-loop; the
    endpoints random.  Returns the src-sorted [2, E]."""
    g = torch.Generator().manual_seed(seed)
    deg = torch.tensor([3000] + [DEGS[(i - 1) % len(DEGS)] for i in range(1, n)])
    src = torch.repeat_interleave(torch.arange(n), deg)
    dst = torch.randint(0, n, (src.numel(),), generator=g)
    last = n - 1
    if n > 2:  # a self-loop and an exact duplicate on the last node (node 1 stays empty)
        src = torch.cat([src, torch.tensor([last, last, last])])
        dst = torch.cat([dst, torch.tensor([last, 0, 0])])
    return torch.stack([src, dst])


def _raw_uncertainty(y, csr, n, C, R, k, guard=8, sentinel=-7.0):
    """ngnn_nbr_uncertainty at the C ABI into w[0..R) of a sentinel-filled buffer."""
    buf = torch.full((R + guard,), sentinel, device=DEV)
    _lib.check(_lib.load().ngnn_nbr_uncertainty(
        y.data_ptr(), y.stride(0) if n > 1 else C, n, C, csr.rowptr.data_ptr(), csr.col.data_ptr(), R, k, 1e-16,
        buf.data_ptr(), _lib.stream_handle(DEV)), "ngnn_nbr_uncertainty")
    torch.cuda.synchronize()
    return buf.cpu()


@pytest.mark.parametrize("C", CS)
@pytest.mark.parametrize("N", [1, 5, 65, 300])
def test_uncertainty_shapes_orders_rows_and_guard(N, C):
    y = R.log_probs(N, C, 2.0, 100 * C + N)
    ei = _degree_graph(N, 7 * N + C)
    want = R.uncertainty(ei, y.double(), C)
    assert float(want[min(1, N - 1)]) == 1.0 or N == 1
    _, yd = _padded(y, 0, 3, grad=False)  # ld = C + 3, NaN in the padding
    E = ei.size(1)
    perm = torch.randperm(E, generator=torch.Generator().manual_seed(N + C))
    orders = {"src-sorted": ei, "dst-sorted": ei[:, torch.argsort(ei[1], stable=True)], "unsorted": ei[:, perm]}
    for tag, e in orders.items():
        ed = e.to(DEV)
        w = get_uncertainty_batch(ed, yd, C)
        assert w.shape == (N,) and torch.isfinite(w).all(), tag
        _close_w(w, want)
        blk = get_block(ed, N)
        assert torch.equal(get_uncertainty_batch(blk, yd, C), w), tag  # a Block; and bitwise repeatable
        assert torch.equal(get_uncertainty_batch(ed, yd, C), w), tag
        for rows in sorted({1, N - 1, N}):
            part = get_uncertainty_batch(ed, yd, C, rows=rows)
            assert part.shape == (rows,) and torch.equal(part, w[:rows]), (tag, rows)
            raw = _raw_uncertainty(yd, blk.transposed(), N, C, rows, C)
            assert torch.equal(raw[:rows], w[:rows].cpu()) and bool((raw[rows:] == -7.0).all()), (tag, rows)
    # nbr_classes is the entropy's base only: another value, the same neighbourhoods
    w3 = get_uncertainty_batch(orders["unsorted"].to(DEV), yd, C + 1)
    _close_w(w3, R.uncertainty(ei, y.double(), C + 1))
    with pytest.raises(ValueError):
        get_uncertainty_batch(orders["unsorted"].to(DEV), yd, 1)


# ------------------------------------------------------------ fix_cr shapes

def _cutoff_inputs(B, C, seed):
    """(y_pure, y_noisy, cutoff): N = B rows; the cutoff near the median row
    maximum, the seed walked until the generator's three conditions hold
    (B = 1 cannot have a row on each side)."""
    first = R.log_probs(B, C, 2.0, seed)
    cutoff = round(float(torch.exp(first).max(1).values.median()), 3)
    yp, yn, _, kept = R.admissible_pair(B, C, B, 2.0, cutoff, seed, need_both=B > 1)
    assert B == 1 or 0 < kept < B
    return yp, yn, cutoff


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("C", CS)
@pytest.mark.parametrize("B", [1, 3, 5, 65, 1025])
def test_fix_cr_shapes_leading_dimension_and_row_bound(B, C, mode):
    """N = B + 3 with NaN rows past B, ld = C + 3 with NaN padding; with and
    without w; p_cutoff 0 and one that masks some rows."""
    yp, yn, cutoff = _cutoff_inputs(B, C, 1000 * C + B)
    w = torch.rand(B, generator=torch.Generator().manual_seed(B + C)) + 0.1
    for cut in (0.0, cutoff):
        for ww in (None, w):
            _fix_cr_check(yp, yn, B, mode, cut, ww, extra_rows=3, pad=3)


@pytest.mark.parametrize("mode", list(MODES))
def test_fix_cr_non_unit_incoming_gradient(mode):
    yp, yn, cutoff = _cutoff_inputs(65, 7, 11)
    w = torch.rand(65, generator=torch.Generator().manual_seed(12)) + 0.1
    _fix_cr_check(yp, yn, 65, mode, cutoff, w, extra_rows=5, scale=-2.5)
    _fix_cr_check(yp, yn, 65, mode, cutoff, None, scale=0.125)


@pytest.mark.parametrize("mode", list(MODES))
def test_fix_cr_batch_size_past_the_rows(mode):
    yp, yn, cutoff = _cutoff_inputs(37, 7, 21)
    _fix_cr_check(yp, yn, 37, mode, cutoff, None, pad=3, batch_size=512)


@pytest.mark.parametrize("mode", list(MODES))
def test_fix_cr_two_forwards_before_either_backward(mode):
    nm, hard = MODES[mode]
    cases = [_cutoff_inputs(33, 7, s) for s in (31, 32)]
    leaves, losses = [], []
    for yp, yn, cutoff in cases:
        lp, vp = _padded(yp, 4, 0)
        ln, vn = _padded(yn, 4, 0)
        leaves.append((lp, ln))
        losses.append(fix_cr(vp, vn, None, batch_size=33, name=nm, p_cutoff=cutoff, use_hard_labels=hard))
    for loss in losses:
        loss.backward()
    for (lp, ln), (yp, yn, cutoff) in zip(leaves, cases):
        _, gp, gn = _ref64(yp, yn, 33, mode, cutoff, None)
        assert_wgrad(ln.grad.cpu()[:33], gn, msg="two forwards d y_noisy")
        assert torch.count_nonzero(ln.grad[33:]) == 0
        if mode != "hard":
            assert_wgrad(lp.grad.cpu()[:33], gp, msg="two forwards d y_pure")


# ------------------------------------------------- semantics easy to lose

def test_fix_cr_bitwise_tie_takes_the_first_index():
    C = 70  # the tie spans two 64-lane chunks: columns 3 and 66
    z = torch.zeros(4, C)
    z[:, 3] = 2.0
    z[:, 66] = 2.0
    z[1, 10] = 2.0  # row 1: a three-way tie, the first at 3 still
    yp = torch.log_softmax(z, dim=1)
    assert torch.equal(yp[:, 3], yp[:, 66])
    yn = R.log_probs(4, C, 1.0, 5)
    a, b = yp.to(DEV).requires_grad_(True), yn.to(DEV).requires_grad_(True)
    loss = fix_cr(a, b, None, batch_size=4)
    lsm = torch.log_softmax(torch.exp(yn.double()), dim=1)
    _close_loss(loss, -lsm[:, 3].mean())
    loss.backward()
    g = b.grad.cpu()
    assert bool((g[:, 3] < 0).all()) and bool((g[:, 66] > 0).all()) and float(g[1, 10]) > 0


def test_fix_cr_masked_nan_row_still_poisons_the_loss():
    yp, yn, cutoff = _cutoff_inputs(65, 7, 41)
    masked = int(torch.nonzero(~R.keep_mask(yp, 65, cutoff))[0])
    yn = yn.clone()
    yn[masked, 2] = NAN
    for hard in (True, False):
        loss = fix_cr(yp.to(DEV), yn.to(DEV), None, batch_size=65, p_cutoff=cutoff, use_hard_labels=hard)
        assert torch.isnan(loss).item()  # the mask multiplies
        assert torch.isnan(R.fix_cr(yp.double(), yn.double(), 65, "ce", cutoff, hard)).item()
        # past B the same NaN is never read
        ok = fix_cr(yp.to(DEV), yn.to(DEV), None, batch_size=masked, p_cutoff=cutoff, use_hard_labels=hard) \
            if masked else None
        assert ok is None or torch.isfinite(ok).item()


def test_fix_cr_w_receives_no_gradient_and_inputs_stay_on_the_device():
    yp, yn, cutoff = _cutoff_inputs(65, 7, 51)
    w = (torch.rand(65, generator=torch.Generator().manual_seed(52)) + 0.1).to(DEV).requires_grad_(True)
    a, b = yp.to(DEV).requires_grad_(True), yn.to(DEV).requires_grad_(True)
    # ind_noisy and T are accepted and never read (a device tensor: no copy to the host)
    loss = fix_cr(a, b, torch.arange(5, device=DEV), batch_size=65, T=0.5, p_cutoff=cutoff, use_hard_labels=False, w=w)
    loss.backward()
    assert w.grad is None and a.grad is not None and b.grad is not None
    _close_loss(loss, _ref64(yp, yn, 65, "soft", cutoff, w.detach().cpu())[0])
    # l2 ignores w and p_cutoff
    l2 = fix_cr(a, b, None, batch_size=65, name="l2", p_cutoff=0.99, w=w)
    assert torch.equal(l2, fix_cr(a, b, None, batch_size=65, name="l2"))
    with pytest.raises(ValueError):
        fix_cr(a, b, None, name="kl")
    # get_uncertainty_batch: detached whatever it is given
    ei = R.graph_edges(65, 300, 1).to(DEV)
    assert not get_uncertainty_batch(ei, a, 7).requires_grad


# ---------------------------------------------------------- a captured step

def _pl_step(model, opt, blk, x, y, n_id, B, C):
    """One train_ct-style step on a SAGEPL model: seed cross entropy plus the
    uncertainty-weighted consistency term, backward, Adam."""
    opt.zero_grad(set_to_none=True)
    _, y_pure, logits, _, y_noisy, _ = model(x, blk, 0.1, n_id)
    w = get_uncertainty_batch(blk, y_pure.detach(), C, rows=B)
    loss = seed_cross_entropy(logits, y, B) + 1.0 * fix_cr(y_pure, y_noisy, None, batch_size=B, w=w)
    loss.backward()
    opt.step()
    return loss.detach()


def test_captured_step_with_uncertainty_weighted_consistency():
    """SAGEPL (its six outputs feed the term directly), N = 200, F = 16,
    hidden 32, C = 7, B = 32: one step captured as a HIP graph and replayed
    three times, against the same body run eagerly on a twin."""
    import ngnn
    from ngnn.optim import Adam
    N, F, H, C, B, TABLE = 200, 16, 32, 7, 32, 500
    torch.manual_seed(7)
    m_g = ngnn.SAGEPL(F, H, C, 2, TABLE, dropout=0.0).to(DEV).train()
    m_e = copy.deepcopy(m_g)
    o_g, o_e = Adam(m_g.parameters(), lr=1e-2), Adam(m_e.parameters(), lr=1e-2)
    gen = torch.Generator().manual_seed(8)
    ei = R.graph_edges(N, 1200, 9, hub_deg=100).to(DEV)
    blk = get_block(ei, N)  # validated (its one host read-back) and grouped both ways before the capture
    blk.transposed()
    batches = [(torch.randn(N, F, generator=gen).to(DEV), torch.randint(0, C, (N,), generator=gen).to(DEV),
                torch.randperm(TABLE, generator=gen)[:N].to(DEV)) for _ in range(4)]
    x, y, n_id = (t.clone() for t in batches[0])
    snap = [p.detach().clone() for p in m_g.parameters()]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):  # warm-up: gradients, workspaces, the optimizer's state
            _pl_step(m_g, o_g, blk, x, y, n_id, B, C)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss_g = _pl_step(m_g, o_g, blk, x, y, n_id, B, C)
    torch.cuda.synchronize()
    with torch.no_grad():  # back to the twin's start: parameters, and a fresh optimizer's zeros
        for p, v in zip(m_g.parameters(), snap):
            p.copy_(v)
        for st in o_g.state.values():
            for t in st.values():
                if torch.is_tensor(t):
                    t.zero_()
    for bx, by, bid in batches[1:]:
        x.copy_(bx)
        y.copy_(by)
        n_id.copy_(bid)
        graph.replay()
        le = float(_pl_step(m_e, o_e, blk, bx, by, bid, B, C))
        lg = float(loss_g)
        assert abs(lg - le) <= 1e-5 * max(1.0, abs(le)), (lg, le)
    torch.cuda.synchronize()
    for (n, pg), pe in zip(m_g.named_parameters(), m_e.parameters()):
        torch.testing.assert_close(pg, pe, rtol=1e-4, atol=2e-6, msg=f"captured step: {n}")
