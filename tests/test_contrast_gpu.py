"""shuffle_pos and the contrastive discriminator loss on the device:
ngnn_shuffle_rows bitwise against the numpy restatement of its draw
(tests/contrast_ref.py) over both kernels' size classes, paddings and
alignments; ngnn.ops.shuffle_pos; ngnn_contrast_fwd / _bwd against the
float64 run of the reference's op sequence and against the reference's own
fixtures; duplicates, large logits, bad indices, the batch_size buffers; and
one train_ct step with the contrastive term against the same step on the
torch composition."""
import os

import numpy as np
import pytest
import torch

import ngnn
from ngnn import _lib, losses
from ngnn.loader import Graph, sample_block
from ngnn.losses import CTLoss, contrastive_loss

import contrast_ref as R
from gradbar import WGRAD_REL, assert_wgrad, grad_ratio

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
LOSS_TOL = dict(rtol=1e-5, atol=1e-6)
NAN = float("nan")


# ------------------------------------------------------------------ shuffle
def _padded(rows, cols, pad, offset, values=None):
    """A [rows, cols] view with row stride cols + pad into a NaN-filled flat
    buffer, its base `offset` floats past the (256-B aligned) allocation."""
    ld = cols + pad
    flat = torch.full((offset + max(rows, 1) * ld,), NAN, dtype=torch.float32, device=DEV)
    full = flat[offset:offset + rows * ld].view(rows, ld)
    if values is not None:
        full[:, :cols] = values
    return flat, full, ld


def _shuffle_raw(xfull, ldx, n, F, m, seed, ofull, ldo):
    _lib.check(_lib.load().ngnn_shuffle_rows(_lib.ptr(xfull), ldx, n, F, m, seed, _lib.ptr(ofull), ldo,
                                             _lib.stream_handle(DEV)), "ngnn_shuffle_rows")


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


SHUFFLE_F = [1, 7, 64, 65, 100, 128, 131, 256, 257, 767, 8710]


@pytest.mark.parametrize("F", SHUFFLE_F)
def test_shuffle_rows_bitwise(F):
    rows = (1, 3) if F == 8710 else (1, 3, 65, 1025)
    n_max = rows[-1]
    ms = sorted({0, min(1, F), min(2, F), int(0.7 * F), max(F - 1, 0), F})
    x = np.random.default_rng(F).standard_normal((n_max, F)).astype(np.float32)
    seed = 0x1234_5678_9ABC_DEF0 + F
    wants = {m: R.shuffle_rows_ref(x, m, seed) for m in ms}  # once per (F, m): fewer rows are its prefix
    for case, (pad, offset) in enumerate(((3, 0), (0, 0), (5, 1))):
        # (3, 0): NaN-padded rows; (0, 0): dense, 16-B aligned where F allows; (5, 1): base off by one float
        _, xfull, ldx = _padded(n_max, F, pad, offset, torch.from_numpy(x).to(DEV))
        for m in ms:
            want = wants[m]
            for n in rows if case == 0 else rows[-1:]:
                oflat, ofull, ldo = _padded(n_max, F, pad + 2, offset)
                _shuffle_raw(xfull, ldx, n, F, m, seed, ofull, ldo)
                got = ofull.cpu().numpy()
                assert np.array_equal(_bits(got[:n, :F]), _bits(want[:n])), (F, m, n, pad, offset)
                # the padding and the rows past n were never written, and no NaN came in from x's padding
                assert np.isnan(got[:n, F:]).all() and np.isnan(got[n:]).all()
                assert np.isnan(oflat[:offset].cpu().numpy()).all()
                assert not np.isnan(got[:n, :F]).any()


# (seed, F, m, row): the row's keys tie in their upper 32 bits where it matters (selection threshold; ranks in
# S_r) -- found by search, checked by tests/test_contrast_ref.py: the one-wave kernel's exact path
UPPER_HALF_TIES = [(61, 256, 197, 372), (35, 256, 256, 683)]


@pytest.mark.parametrize("seed,F,m,row", UPPER_HALF_TIES)
def test_shuffle_rows_upper_half_ties_take_the_exact_path(seed, F, m, row):
    assert any(R.upper_half_shortcut_fails(row, F, m, seed))
    n = 1025
    x = np.random.default_rng(seed).standard_normal((n, F)).astype(np.float32)
    want = R.shuffle_rows_ref(x, m, seed)
    xd = torch.from_numpy(x).to(DEV)
    out = torch.empty(n, F, device=DEV)
    _shuffle_raw(xd, F, n, F, m, seed, out, F)
    got = out.cpu().numpy()
    assert np.array_equal(_bits(got[row]), _bits(want[row]))
    assert np.array_equal(_bits(got), _bits(want))


def test_shuffle_rows_seeds_and_repeats():
    N, F, m = 65, 100, 70
    x = torch.randn(N, F, device=DEV)
    outs = []
    for seed in (5, 5, 6):
        o = torch.empty(N, F, device=DEV)
        _shuffle_raw(x, F, N, F, m, seed, o, F)
        outs.append(o)
    assert torch.equal(outs[0], outs[1])
    assert not torch.equal(outs[0], outs[2])
    # empty work: success, nothing touched
    o = torch.full((4, 8), NAN, device=DEV)
    _shuffle_raw(x, F, 0, 8, 4, 1, o, 8)
    _shuffle_raw(x, F, 4, 0, 0, 1, o, 8)
    assert torch.isnan(o).all()


def test_shuffle_pos_op():
    x = torch.randn(65, 100, device=DEV, requires_grad=True)
    # prob -> m as the reference computes it (augmentation.py:94)
    for F, prob in ((100, 0.7), (128, 0.9)):
        xs = torch.randn(33, F, device=DEV)
        out = ngnn.shuffle_pos(xs, device=DEV, prob=prob, seed=21)
        want = R.shuffle_rows_ref(xs.cpu().numpy(), int(F * prob), 21)
        assert np.array_equal(_bits(out.cpu().numpy()), _bits(want))
    out = ngnn.ops.shuffle_pos(x, prob=0.7, seed=3)
    assert not out.requires_grad and out.grad_fn is None and out.data_ptr() != x.data_ptr()
    assert out.shape == x.shape and out.is_contiguous()
    # a row-strided view is read in place
    wide = torch.randn(40, 140, device=DEV)
    view = wide[:, 20:120]
    assert torch.equal(ngnn.shuffle_pos(view, prob=0.7, seed=4), ngnn.shuffle_pos(view.contiguous(), prob=0.7, seed=4))
    # seed=None draws from torch's CPU generator: manual_seed repeats the run
    torch.manual_seed(77)
    a = ngnn.shuffle_pos(x, prob=0.7)
    b = ngnn.shuffle_pos(x, prob=0.7)
    torch.manual_seed(77)
    c = ngnn.shuffle_pos(x, prob=0.7)
    assert torch.equal(a, c) and not torch.equal(a, b)
    assert torch.equal(ngnn.shuffle_pos(x, prob=0.0, seed=1), x.detach())
    with pytest.raises(ValueError):
        ngnn.shuffle_pos(x, prob=1.5, seed=1)


# ----------------------------------------------------------------- contrast
def _dev_inputs(N, H, seed, scale=0.25, pad=0):
    """relu(scale * randn) triples on the device as leaf tensors; pad > 0: each a
    [:, :H] view of a NaN-padded [N, H + pad] buffer (row stride H + pad)."""
    cpu = R.relu_inputs(N, H, seed, scale)
    dev = []
    for t in cpu:
        if pad:
            buf = torch.full((N, H + pad), NAN, device=DEV)
            buf[:, :H] = t.to(DEV)
            dev.append(buf[:, :H].detach().requires_grad_(True))
        else:
            dev.append(t.to(DEV).requires_grad_(True))
    return cpu, dev


def _check_against_f64(cpu, dev, idx, scale=1.0, batch_size=None, tag=""):
    loss = contrastive_loss(*dev, idx.to(DEV), batch_size=batch_size)
    (loss * scale).backward()
    want_loss, *want = R.contrast_ref_f64(*cpu, idx, scale)
    torch.testing.assert_close(loss.detach().cpu().double(), want_loss, **LOSS_TOL)
    rest = torch.ones(cpu[0].size(0), dtype=torch.bool)
    rest[idx] = False
    for t, w, nm in zip(dev, want, ("dh", "dhp", "dhn")):
        g = t.grad.cpu()
        assert g.shape == w.shape
        assert_wgrad(g, w, f"{tag} {nm}")
        assert (g[rest] == 0).all(), f"{tag} {nm}: a row outside idx was written"
    return loss


@pytest.mark.parametrize("H", [1, 7, 64, 65, 130, 256, 512])
def test_contrast_loss_and_gradients_vs_float64(H):
    for M in (1, 3, 64, 65, 300, 1025):
        N = M + 37
        idx = torch.randperm(N, generator=torch.Generator().manual_seed(M))[:M]
        pad = 3 if M in (3, 65, 1025) else 0
        cpu, dev = _dev_inputs(N, H, seed=1000 * H + M, pad=pad)
        _check_against_f64(cpu, dev, idx, scale=3.5 if M in (64, 65) else 1.0, tag=f"H{H} M{M}")


def test_contrast_duplicate_indices_accumulate():
    M, N, H = 65, 102, 130
    g = torch.Generator().manual_seed(9)
    idx = torch.randperm(N, generator=g)[:45]
    idx = torch.cat([idx, idx[torch.randint(0, 45, (20,), generator=g)]])[torch.randperm(M, generator=g)]
    assert idx.numel() == M and idx.unique().numel() == 45
    cpu, dev = _dev_inputs(N, H, seed=10)
    _check_against_f64(cpu, dev, idx, tag="duplicates")


def test_contrast_large_logits_keep_the_positive_gradient():
    """Unit-scale ReLU'd activations at H = 256: the logits reach about 60,
    where torch's float32 BCEWithLogits backward has lost sigma(-a) entirely."""
    N, H, M = 300, 256, 205
    idx = torch.randperm(N, generator=torch.Generator().manual_seed(3))[:M]
    cpu, dev = _dev_inputs(N, H, seed=11, scale=1.0)
    a = (cpu[0][idx].double() * cpu[1][idx].double()).sum(1)
    assert float(a.max()) > 50 and float(a.min()) > 17
    loss = _check_against_f64(cpu, dev, idx, tag="large logits")
    assert float(dev[1].grad.abs().max()) > 0
    # the float32 torch composition does not meet that bar (what the fused path is for)
    comp = [t.detach().clone().requires_grad_(True) for t in dev]
    R.contrast_ref(*comp, idx.to(DEV)).backward()
    err, ref = grad_ratio(comp[1].grad, R.contrast_ref_f64(*cpu, idx)[2])
    assert err > WGRAD_REL * ref
    # deterministic forward: bitwise equal twice
    again = contrastive_loss(*dev, idx.to(DEV))
    assert torch.equal(loss.detach(), again.detach())


@pytest.mark.parametrize("name", ["contrast_n128_h130", "contrast_n64_h512"])
def test_contrast_reference_fixture(golden_dir, name):
    g = np.load(os.path.join(golden_dir, name + ".npz"))
    dev = [torch.from_numpy(g[k]).to(DEV).requires_grad_(True) for k in ("h", "hp", "hn")]
    idx = torch.from_numpy(g["idx"]).to(DEV)
    loss = contrastive_loss(*dev, idx)
    loss.backward()
    torch.testing.assert_close(loss.detach().cpu(), torch.from_numpy(g["loss"]), **LOSS_TOL)
    for t, k in zip(dev, ("grad_h", "grad_hp", "grad_hn")):
        assert_wgrad(t.grad.cpu(), torch.from_numpy(g[k]), f"{name} {k}")
    # the two-step drop-ins give the same loss
    lp, ln = losses.Discriminator_innerprod()(dev[0][idx], dev[1][idx], dev[2][idx])
    assert lp.shape == (idx.numel(), 1) and ln.shape == (idx.numel(), 1)
    two = losses.BCEExeprtLoss(dev[0].size(0))(lp, ln)
    torch.testing.assert_close(two.detach().cpu(), torch.from_numpy(g["loss"]), **LOSS_TOL)


def test_contrast_bad_index_is_nan_counted_and_unwritten():
    N, H, M = 50, 65, 9
    cpu, dev = _dev_inputs(N, H, seed=12)
    idx = torch.randperm(N, generator=torch.Generator().manual_seed(4))[:M]
    bad_at = 4
    idx[bad_at] = N
    losses.contrast_bad_indices(DEV, reset=True)
    loss = contrastive_loss(*dev, idx.to(DEV))
    loss.backward()
    assert torch.isnan(loss).item()
    assert contrastive_loss.bad_index.is_cuda and contrastive_loss.bad_index.dtype == torch.int32
    assert int(contrastive_loss.bad_index.item()) == 1
    assert losses.contrast_bad_indices(DEV, reset=True) == 1 and losses.contrast_bad_indices(DEV) == 0
    # the good rows got their gradients, nothing else was written (no row N exists to write)
    good = torch.cat([idx[:bad_at], idx[bad_at + 1:]])
    _, *want = R.contrast_ref_f64(*cpu, good, scale=(M - 1) / M)  # (the kernel's mean is over M)
    rest = torch.ones(N, dtype=torch.bool)
    rest[good] = False
    for t, w in zip(dev, want):
        assert_wgrad(t.grad.cpu(), w, "bad index: good rows")
        assert (t.grad.cpu()[rest] == 0).all()


def test_contrast_batch_size_buffers():
    N, H, B = 200, 64, 48
    cpu, dev = _dev_inputs(N, H, seed=13)
    g = torch.Generator().manual_seed(5)
    idx1 = torch.randperm(B, generator=g)[:20]
    loss = _check_against_f64(cpu, dev, idx1, batch_size=B, tag="batch_size first")
    grads = [t.grad for t in dev]
    for gr in grads:
        assert gr.shape == (N, H) and (gr[B:] == 0).all()
    # the hint rides on the tensor the backward hands to autograd
    seen = []

    class Spy(torch.autograd.Function):  # stands where the SAGE stack's backward reads the hint
        @staticmethod
        def forward(ctx, t):
            return t.view_as(t)

        @staticmethod
        def backward(ctx, gr):
            seen.append((getattr(gr, "_ngnn_nonzero_rows", None), tuple(gr.shape)))
            return gr

    h2 = dev[0].detach().clone().requires_grad_(True)
    contrastive_loss(Spy.apply(h2), dev[1].detach(), dev[2].detach(), idx1.to(DEV), batch_size=B).backward()
    assert seen == [(B, (N, H))]
    # a second call with other indices: no stale rows below B
    idx2 = torch.arange(B - 7, B)
    for t in dev:
        t.grad = None
    _check_against_f64(cpu, dev, idx2, batch_size=B, tag="batch_size second")
    # an index >= B is bad under the promise
    losses.contrast_bad_indices(DEV, reset=True)
    bad = contrastive_loss(*[t.detach() for t in dev], torch.tensor([1, B], device=DEV), batch_size=B)
    assert torch.isnan(bad).item() and losses.contrast_bad_indices(DEV, reset=True) == 1
    # no rows: NaN, the reference's mean over nothing, without a launch of the entries
    empty = contrastive_loss(*dev, torch.empty(0, dtype=torch.int64, device=DEV), batch_size=B)
    assert torch.isnan(empty).item() and empty.is_cuda
    assert torch.isfinite(loss).item()


# --------------------------------------------------- one train_ct step
B, FAN, N_TAB, F_IN, HID, C = 64, [4, 3], 400, 32, 64, 7


def _graph(n, f, c, seed):
    g = torch.Generator().manual_seed(seed)
    degs = torch.randint(1, 9, (n,), generator=g)
    rowptr = torch.zeros(n + 1, dtype=torch.int64)
    rowptr[1:] = torch.cumsum(degs, 0)
    col = torch.randint(0, n, (int(rowptr[-1]),), generator=g).to(torch.int32)
    x = torch.randn(n, f, generator=g)
    y = torch.randint(0, c, (n,), generator=g)
    return Graph(rowptr.to(DEV), col.to(DEV), x.to(DEV), y.to(DEV), torch.arange(n, device=DEV), c)


def test_train_ct_step_with_the_contrastive_term():
    """pipeline_test.py:113-144 on two SAGEPL models: CTLoss -> topk_rewire ->
    shuffle_pos -> the four extra passes -> contrastive_loss(batch_size=B),
    against the same step whose contrastive term is the reference's op
    sequence in float32 on the device (fed the device's shuffled new_x)."""
    g = _graph(N_TAB, F_IN, C, seed=3)
    blk = sample_block(g, torch.randperm(N_TAB, generator=torch.Generator().manual_seed(4))[:B].to(DEV), FAN,
                       seed=9)
    gen = torch.Generator().manual_seed(6)
    y_noise = torch.randint(0, C, (N_TAB,), generator=gen).to(DEV)
    clean = (torch.rand(N_TAB, generator=gen) < 0.7).to(DEV)
    models = []
    for s in (1, 2):
        torch.manual_seed(s)
        models.append(ngnn.SAGEPL(F_IN, HID, C, 2, nbr_nodes=N_TAB, dropout=0.0).to(DEV).train())
    beta, forget = 0.5, 0.2
    new_x = ngnn.shuffle_pos(blk.x, device=DEV, prob=0.7, seed=31)
    assert new_x.shape == blk.x.shape and not torch.equal(new_x, blk.x)

    def step(fused: bool):
        for m in models:
            m.zero_grad(set_to_none=True)
        outs = [m(blk.x, blk.edge_index, noise_rate=0.1, n_id=blk.n_id) for m in models]
        res = CTLoss(DEV)(outs[0][2][:B], outs[1][2][:B], y_noise[blk.n_id[:B]], forget, blk.n_id[:B], clean)
        ind_noisy = (res[6], res[7])
        pos_edge, neg_edge = ngnn.topk_rewire(outs[0][0], blk.edge_index, DEV, k_percent=0.1)
        hedge = [m(blk.x, pos_edge, noise_rate=0.1, n_id=blk.n_id)[0] for m in models]
        hneg = [m(new_x, neg_edge, noise_rate=0.7, n_id=blk.n_id)[3] for m in models]
        if fused:
            cont = [contrastive_loss(outs[i][0], hedge[i], hneg[i], ind_noisy[i], batch_size=B) for i in range(2)]
        else:
            cont = [R.contrast_ref(outs[i][0], hedge[i], hneg[i], ind_noisy[i]) for i in range(2)]
        loss = res[0] + res[1] + beta * cont[0] + beta * cont[1]
        loss.backward()
        grads = [{k: p.grad.detach().clone() for k, p in m.named_parameters()} for m in models]
        return loss.detach(), [c.detach() for c in cont], ind_noisy, grads

    want_loss, want_cont, want_ind, want_grads = step(fused=False)
    got_loss, got_cont, got_ind, got_grads = step(fused=True)
    assert want_ind[0].numel() == B - int((1 - forget) * B) and want_ind[0].numel() > 0
    for i in range(2):
        assert torch.equal(got_ind[i], want_ind[i])
        assert abs(float(got_cont[i]) - float(want_cont[i])) <= 1e-5
    assert abs(float(got_loss) - float(want_loss)) <= 1e-5
    assert losses.contrast_bad_indices(DEV) == 0
    for i in range(2):
        assert set(got_grads[i]) == set(want_grads[i]) and "noise" in got_grads[i]
        for k, w in want_grads[i].items():
            assert float(w.abs().max()) > 0, k
            assert_wgrad(got_grads[i][k], w, f"model {i + 1} {k}")
