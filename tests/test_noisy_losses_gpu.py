"""ngnn.losses.backward_correction and ngnn.losses.CoDiLoss on the device
against the float64 run of tests/losses_noisy_ref.py (pinned to the
reference's own module by tests/test_noisy_losses_ref.py) and against the
reference-generated fixtures tests/golden/bc_*.npz / codi_*.npz.

Bars, the project's (tests/test_losses_gpu.py): losses rtol 1e-5, atol 1e-6;
pure ratios and kept sets exact (rows whose keys lie within 1e-5 of the
selection boundary may swap, test_coteaching_gpu._selection's rule -- the
yardstick then takes the device's selection); gradients by
gradbar.assert_wgrad (1e-5 of the tensor's max: these gradients are
O(1 / (B C)), an absolute bar would hide everything); js at rtol = atol =
1e-5; graph steps against the same loop body run eagerly, losses 1e-5,
parameters rtol 1e-4, atol 2e-6."""
import os

import numpy as np
import pytest
import torch

import losses_noisy_ref as R
from gradbar import assert_wgrad
from ngnn import _lib
from ngnn.losses import CoDiLoss, CTLoss, backward_correction
from test_coteaching_gpu import _selection

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
NAN = float("nan")
CS = [1, 7, 47, 64, 65, 130]          # below, at and past one 64-lane stride
BS = [1, 3, 5, 65, 1024, 1025, 2049]  # four rows per workgroup; the select's 1024 threads, padded sorts


def _padded(y, extra_rows=0, pad=0):
    """A device leaf [B + extra_rows, C + pad], NaN outside y, and its [:, :C] view."""
    B, C = y.shape
    buf = torch.full((B + extra_rows, C + pad), NAN)
    buf[:B, :C] = y
    leaf = buf.to(DEV).requires_grad_(True)
    return leaf, leaf[:, :C]


def _matrix(C, kind="pair"):
    if C == 1:
        return np.ones((1, 1))
    return R.pair_flip_matrix(C, 0.3) if kind == "pair" else R.uniform_flip_matrix(C, 0.3)


# ------------------------------------------------------- backward correction

def _bc_ref64(x, y, mat, scale=1.0):
    xd = x.double().requires_grad_(True)
    loss = R.backward_correction(xd, y, mat, x.size(1))
    (loss * scale).backward()
    return loss.detach(), xd.grad


def _bc_check(x, y, mat, extra_rows=0, pad=0, scale=None):
    B, C = x.shape
    leaf, view = _padded(x, extra_rows, pad)
    yd = torch.cat([y, torch.zeros(extra_rows, dtype=torch.long)]).to(DEV)
    loss = backward_correction(view, yd, mat, C, DEV, batch_size=B if extra_rows else None)
    want, gwant = _bc_ref64(x, y, mat, 1.0 if scale is None else scale)
    torch.testing.assert_close(loss.detach().cpu().double(), want, rtol=1e-5, atol=1e-6)
    (loss if scale is None else loss * scale).backward()
    g = leaf.grad.cpu()
    assert torch.count_nonzero(g[B:]) == 0 and torch.count_nonzero(g[:, C:]) == 0
    assert_wgrad(g[:B, :C], gwant, msg=f"bc B={B} C={C}")
    return loss


@pytest.mark.parametrize("name", ["bc_b300", "bc_b65"])
def test_bc_vs_reference_fixture(golden_dir, name):
    g = np.load(os.path.join(golden_dir, name + ".npz"))
    x, y = torch.from_numpy(g["output"]), torch.from_numpy(g["labels"])
    loss = _bc_check(x, y, g["C"])
    torch.testing.assert_close(loss.detach().cpu(), torch.from_numpy(g["loss"]), rtol=1e-5, atol=1e-6)
    a = x.to(DEV).requires_grad_(True)
    backward_correction(a, y.to(DEV), g["C"], x.size(1), DEV).backward()
    assert_wgrad(a.grad.cpu(), torch.from_numpy(g["grad_output"]), msg=name)


@pytest.mark.parametrize("C", CS)
@pytest.mark.parametrize("B", BS)
def test_bc_shapes_leading_dimension_and_row_bound(B, C):
    """ld = C + 3 with NaN in the padding, N = B + 3 with NaN rows the loss
    never reads, gradient rows >= B exactly zero; a non-symmetric matrix."""
    x = R.bc_logits(B, C, 3.0, 100 * C + B)
    y = torch.randint(0, C, (B,), generator=torch.Generator().manual_seed(B + C))
    _bc_check(x, y, _matrix(C), extra_rows=3, pad=3)


def test_bc_b8192_whole_rows():
    x = R.bc_logits(8192, 47, 3.0, 7)
    y = torch.randint(0, 47, (8192,), generator=torch.Generator().manual_seed(8))
    _bc_check(x, y, _matrix(47, "uniform"))


def test_bc_non_unit_incoming_gradient():
    x = R.bc_logits(65, 7, 8.0, 11)
    y = torch.randint(0, 7, (65,), generator=torch.Generator().manual_seed(12))
    _bc_check(x, y, _matrix(7), extra_rows=5, scale=-2.5)
    _bc_check(x, y, _matrix(7), scale=0.125)


def test_bc_two_forwards_before_either_backward():
    mat = _matrix(7)
    xs = [R.bc_logits(33, 7, 3.0, s) for s in (21, 22)]
    ys = [torch.randint(0, 7, (33,), generator=torch.Generator().manual_seed(s)) for s in (23, 24)]
    leaves, losses = [], []
    for x, y in zip(xs, ys):
        leaves.append(torch.cat([x, torch.full((4, 7), NAN)]).to(DEV).requires_grad_(True))
        losses.append(backward_correction(leaves[-1], torch.cat([y, y[:4]]).to(DEV), mat, 7, batch_size=33))
    from ngnn.losses import unit_grad
    one = unit_grad(losses[0])  # (the training step's path: the rows the forward wrote are handed over)
    g0 = torch.autograd.grad(losses[0], leaves[0], one)[0]
    g1 = torch.autograd.grad(losses[1], leaves[1], one)[0]
    assert g0.data_ptr() != g1.data_ptr()  # one pooled buffer per pending node
    for g, x, y in zip((g0, g1), xs, ys):
        assert_wgrad(g.cpu()[:33], _bc_ref64(x, y, mat)[1], msg="two forwards")
        assert torch.count_nonzero(g[33:]) == 0


def test_bc_replaced_matrix_is_inverted_again():
    x = R.bc_logits(40, 5, 2.0, 31)
    y = torch.randint(0, 5, (40,), generator=torch.Generator().manual_seed(32))
    a, yd = x.to(DEV), y.to(DEV)
    mat = R.uniform_flip_matrix(5, 0.3)
    l0 = backward_correction(a, yd, mat, 5)
    assert torch.equal(l0, backward_correction(a, yd, mat, 5))  # (cached inverse, bitwise repeatable)
    mat[:] = R.pair_flip_matrix(5, 0.2)  # the same object, new contents
    l1 = backward_correction(a, yd, mat, 5)
    torch.testing.assert_close(l1.cpu().double(), _bc_ref64(x, y, mat)[0], rtol=1e-5, atol=1e-6)
    t = torch.from_numpy(R.uniform_flip_matrix(5, 0.1))  # a tensor, then modified in place
    l2 = backward_correction(a, yd, t, 5)
    torch.testing.assert_close(l2.cpu().double(), _bc_ref64(x, y, t)[0], rtol=1e-5, atol=1e-6)
    t.copy_(torch.from_numpy(R.pair_flip_matrix(5, 0.4)))
    l3 = backward_correction(a, yd, t, 5)
    torch.testing.assert_close(l3.cpu().double(), _bc_ref64(x, y, t)[0], rtol=1e-5, atol=1e-6)
    assert len({float(l0), float(l1), float(l2), float(l3)}) == 4
    for _ in range(3):  # a new matrix per run (flip_label): never a stale entry, even at a reused address
        m = R.pair_flip_matrix(5, 0.05 + 0.1 * _)
        got = backward_correction(a, yd, m, 5)
        torch.testing.assert_close(got.cpu().double(), _bc_ref64(x, y, m)[0], rtol=1e-5, atol=1e-6)
        del m


def test_bc_label_out_of_range_is_nan_and_deterministic():
    x = R.bc_logits(130, 47, 2.0, 41)
    y = torch.randint(0, 47, (130,), generator=torch.Generator().manual_seed(42))
    mat = _matrix(47)
    a = x.to(DEV).requires_grad_(True)
    l0 = backward_correction(a, y.to(DEV), mat, 47)
    l0.backward()
    g0 = a.grad.clone()
    a.grad = None
    l1 = backward_correction(a, y.to(DEV), mat, 47)
    l1.backward()
    assert torch.equal(l0, l1) and torch.equal(g0, a.grad)  # fixed-order sums: bitwise
    for bad in (47, 1 << 40, -1):
        yb = y.clone()
        yb[17] = bad
        a.grad = None
        lb = backward_correction(a, yb.to(DEV), mat, 47)
        lb.backward()
        torch.cuda.synchronize()
        assert torch.isnan(lb).item()
        assert torch.isnan(a.grad[17]).all() and torch.isfinite(a.grad[:17]).all() and torch.isfinite(a.grad[18:]).all()


def test_bc_bf16_logits():
    N, C, B = 700, 47, 256
    # (rounded to bf16: the admissibility of the rounded values is what counts)
    x = R.bc_logits(N, C, 3.0, 51, torch.bfloat16)
    y = torch.randint(0, C, (N,), generator=torch.Generator().manual_seed(52))
    mat = _matrix(C)
    a = x.to(DEV).requires_grad_(True)
    loss = backward_correction(a, y.to(DEV), mat, C, batch_size=B)
    want, gwant = _bc_ref64(x[:B].float(), y[:B], mat)
    torch.testing.assert_close(loss.detach().cpu().double(), want, rtol=1e-5, atol=1e-6)
    loss.backward()
    assert a.grad.dtype == torch.bfloat16
    assert torch.equal(a.grad[B:], torch.zeros_like(a.grad[B:]))
    torch.testing.assert_close(a.grad[:B].float().cpu(), gwant.float().to(torch.bfloat16).float(),
                               rtol=8e-3, atol=1e-5 * float(gwant.abs().max()))  # (atol: the fp32 bar)


# ---------------------------------------------------------------------- CoDi

def _codi_inputs(B, C, seed, scale=2.0):
    g = torch.Generator().manual_seed(seed)
    y1, y2 = scale * torch.randn(B, C, generator=g), scale * torch.randn(B, C, generator=g)
    yn = torch.randint(0, C, (B,), generator=g)
    ind = torch.randperm(3 * B, generator=g)[:B]
    clean = torch.rand(3 * B, generator=g) < 0.6
    return y1, y2, yn, ind, clean


def _codi_check(y1, y2, yn, forget, ind, clean, lam=0.1, extra_rows=0, pad=0, ignore=-100, exact_order=False):
    B, C = y1.shape
    la, a = _padded(y1, extra_rows, pad)
    lb, b = _padded(y2, extra_rows, pad)
    fill = torch.zeros(extra_rows, dtype=torch.long)
    crit = CoDiLoss(DEV, lam, ignore_index=ignore, return_indices=True)
    out = crit(a, b, torch.cat([yn, fill]).to(DEV), forget, None if ind is None else torch.cat([ind, fill]).to(DEV),
               None if clean is None else clean.to(DEV), batch_size=B if extra_rows else None)
    out[0].backward()
    out[1].backward()
    torch.cuda.synchronize()
    nr = int((1 - forget) * B) or B  # an empty selection keeps every row
    assert out[4].numel() == nr and out[5].numel() == nr and out[6].numel() == B - nr and out[7].numel() == B - nr
    for k, n in ((out[4], out[6]), (out[5], out[7])):
        assert torch.equal(torch.cat([k, n]).sort().values.cpu(), torch.arange(B))
    y1d, y2d = y1.double().requires_grad_(True), y2.double().requires_grad_(True)
    k1, k2, _ = R.codi_keys(y1d.detach(), y2d.detach(), yn, lam, ignore)
    if exact_order:
        for got_k, got_n, key in ((out[4], out[6], k1), (out[5], out[7], k2)):
            assert torch.equal(torch.cat([got_k, got_n]).cpu(), torch.sort(key, stable=True).indices)
    sel1 = _selection(k1, nr, out[4].cpu()).sort().values
    sel2 = _selection(k2, nr, out[5].cpu()).sort().values
    assert torch.equal(out[4].sort().values.cpu(), sel1) and torch.equal(out[5].sort().values.cpu(), sel2)
    ref = R.codi_loss(y1d, y2d, yn, forget, ind, clean, lam, ignore, sel=(sel1, sel2))
    for k in (0, 1):
        torch.testing.assert_close(out[k].detach().cpu().double(), ref[k].detach(), rtol=1e-5, atol=1e-6,
                                   equal_nan=True)
    if clean is not None:
        assert float(out[2]) == pytest.approx(float(ref[2]), abs=1e-7)
        assert float(out[3]) == pytest.approx(float(ref[3]), abs=1e-7)
        assert int(crit.index_error.item()) == 0
    ref[0].backward()
    ref[1].backward()
    for leaf, want, tag in ((la, y1d.grad, "y1"), (lb, y2d.grad, "y2")):
        g = leaf.grad.cpu()
        assert torch.count_nonzero(g[B:]) == 0 and torch.count_nonzero(g[:, C:]) == 0
        assert_wgrad(g[:B, :C], want, msg=f"codi {tag} B={B} C={C}")
    return out


@pytest.mark.parametrize("name", ["codi_b300", "codi_b1024"])
def test_codi_vs_reference_fixture(golden_dir, name):
    g = np.load(os.path.join(golden_dir, name + ".npz"))
    y1, y2 = torch.from_numpy(g["y1"]), torch.from_numpy(g["y2"])
    out = _codi_check(y1, y2, torch.from_numpy(g["y_noise"]), float(g["forget_rate"]), torch.from_numpy(g["ind"]),
                      torch.from_numpy(g["noise_or_not"]), lam=float(g["co_lambda"]))
    # (boundary key gaps >= 1e-3, asserted by the generator: the sets are decided)
    assert torch.equal(out[4].sort().values.cpu(), torch.from_numpy(g["ind_1_update"]))
    assert torch.equal(out[5].sort().values.cpu(), torch.from_numpy(g["ind_2_update"]))
    torch.testing.assert_close(out[0].detach().cpu(), torch.from_numpy(g["loss_1"]), rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(out[1].detach().cpu(), torch.from_numpy(g["loss_2"]), rtol=1e-5, atol=1e-6)
    assert float(out[2]) == pytest.approx(float(g["pure_ratio_1"]), abs=1e-7)
    assert float(out[3]) == pytest.approx(float(g["pure_ratio_2"]), abs=1e-7)
    a, b = y1.to(DEV).requires_grad_(True), y2.to(DEV).requires_grad_(True)
    o = CoDiLoss(DEV, float(g["co_lambda"]))(a, b, torch.from_numpy(g["y_noise"]).to(DEV), float(g["forget_rate"]),
                                              torch.from_numpy(g["ind"]).to(DEV),
                                              torch.from_numpy(g["noise_or_not"]).to(DEV))
    assert o[4:] == (0, 0, 0, 0)  # the reference's default return
    o[0].backward()
    o[1].backward()
    assert_wgrad(a.grad.cpu(), torch.from_numpy(g["grad_y1"]), msg=name + " y1")
    assert_wgrad(b.grad.cpu(), torch.from_numpy(g["grad_y2"]), msg=name + " y2")


@pytest.mark.parametrize("C", CS)
@pytest.mark.parametrize("B", BS)
def test_codi_shapes_leading_dimension_and_row_bound(B, C):
    y1, y2, yn, ind, clean = _codi_inputs(B, C, 1000 * C + B)
    _codi_check(y1, y2, yn, 0.3, ind, clean, extra_rows=3, pad=3)


def test_codi_b8192():
    y1, y2, yn, ind, clean = _codi_inputs(8192, 47, 61)
    _codi_check(y1, y2, yn, 0.45, ind, clean)


@pytest.mark.parametrize("forget,kept", [(1.0, 65), (0.98, 1), (0.0, 65)])
def test_codi_num_remember_edges(forget, kept):
    """num_remember 0 (every row kept, ratios over B), 1 and B."""
    y1, y2, yn, ind, clean = _codi_inputs(65, 7, 71)
    assert (int((1 - forget) * 65) or 65) == kept and int((1 - forget) * 65) in (0, 1, 65)
    out = _codi_check(y1, y2, yn, forget, ind, clean, extra_rows=2)
    assert out[4].numel() == kept


@pytest.mark.parametrize("lam", [0.0, 0.1, 1.0])
def test_codi_co_lambda(lam):
    y1, y2, yn, ind, clean = _codi_inputs(300, 47, 81)
    out = _codi_check(y1, y2, yn, 0.2, ind, clean, lam=lam)
    if lam:
        return
    # co_lambda = 0: CTLoss's device results, bitwise
    a, b = y1.to(DEV).requires_grad_(True), y2.to(DEV).requires_grad_(True)
    ct = CTLoss(DEV)(a, b, yn.to(DEV), 0.2, ind.to(DEV), clean.to(DEV))
    for k in range(8):
        assert torch.equal(out[k].detach(), ct[k].detach()), k
    a2, b2 = y1.to(DEV).requires_grad_(True), y2.to(DEV).requires_grad_(True)
    o = CoDiLoss(DEV, 0.0)(a2, b2, yn.to(DEV), 0.2, ind.to(DEV), clean.to(DEV))
    for l_ in (ct[0], ct[1], o[0], o[1]):
        l_.backward()
    assert torch.equal(a.grad, a2.grad) and torch.equal(b.grad, b2.grad)


def test_codi_duplicated_rows_tie_by_row_index_and_ignored_rows():
    y1, y2, yn, ind, clean = _codi_inputs(64, 5, 91)
    for src, dst in ((3, 40), (3, 41), (10, 11), (20, 63)):  # duplicated rows: equal keys in both models
        y1[dst], y2[dst], yn[dst] = y1[src], y2[src], yn[src]
    _codi_check(y1, y2, yn, 0.5, ind, clean, exact_order=False)
    # every row the same: every key ties, the order is the row index
    z1, z2 = y1[:1].repeat(64, 1), y2[:1].repeat(64, 1)
    zn = yn[:1].repeat(64)
    out = _codi_check(z1, z2, zn, 0.25, ind, clean, exact_order=True)
    assert torch.equal(out[4].cpu(), torch.arange(48)) and torch.equal(out[7].cpu(), torch.arange(48, 64))
    # ignored rows: cross entropy 0 in the key, left out of the means, zero gradient
    yn[::7] = -100
    _codi_check(y1, y2, yn, 0.25, ind, clean)
    yn[::7] = 9  # another ignore_index
    _codi_check(y1, y2, yn, 0.25, ind, clean, ignore=9)


def test_codi_backwards_are_independent():
    w1 = torch.randn(8, 4, device=DEV, requires_grad=True)
    w2 = torch.randn(8, 4, device=DEV, requires_grad=True)
    x = torch.randn(32, 8, device=DEV)
    out = CoDiLoss(DEV)(x @ w1, x @ w2, torch.randint(0, 4, (32,), device=DEV), 0.3, None, None)
    out[0].backward()
    assert w1.grad is not None and w2.grad is None
    out[1].backward()
    assert w2.grad is not None


def test_codi_out_of_range_ind_sets_index_error():
    y1, y2, yn, ind, clean = _codi_inputs(40, 5, 95)
    crit = CoDiLoss(DEV)
    crit(y1.to(DEV), y2.to(DEV), yn.to(DEV), 0.0, ind.to(DEV), clean.to(DEV))
    assert int(crit.index_error.item()) == 0
    ind[7] = 3 * 40  # one past noise_or_not
    out = crit(y1.to(DEV), y2.to(DEV), yn.to(DEV), 0.0, ind.to(DEV), clean.to(DEV))
    assert int(crit.index_error.item()) != 0 and torch.isfinite(out[0]).item()


def _codi_raw(y1, y2, yn, nr, lam, pad=0):
    """ngnn_codi_loss_fwd at the C ABI with js_out; returns (js, out[4])."""
    B, C = y1.shape
    _, a = _padded(y1, 0, pad)
    _, b = _padded(y2, 0, pad)
    a, b = a.detach(), b.detach()
    lib = _lib.load()
    ws = torch.empty(lib.ngnn_codi_loss_workspace_bytes(B), dtype=torch.uint8, device=DEV)
    out = torch.empty(4, device=DEV)
    i1, i2 = torch.empty(B, dtype=torch.int64, device=DEV), torch.empty(B, dtype=torch.int64, device=DEV)
    js = torch.empty(B, device=DEV)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    ynd = yn.to(DEV)
    _lib.check(lib.ngnn_codi_loss_fwd(a.data_ptr(), a.stride(0), b.data_ptr(), b.stride(0), B, C, ynd.data_ptr(), -100,
                                      nr, lam, None, None, 0, out.data_ptr(), i1.data_ptr(), i2.data_ptr(),
                                      js.data_ptr(), ws.data_ptr(), ws.numel(), err.data_ptr(),
                                      _lib.stream_handle(DEV)), "ngnn_codi_loss_fwd")
    torch.cuda.synchronize()
    return js.cpu(), out.cpu()


@pytest.mark.parametrize("B,C,pad", [(300, 47, 0), (65, 130, 3), (5, 1, 0), (1025, 7, 3)])
def test_codi_js_out_vs_float64(B, C, pad):
    y1, y2, yn, _, _ = _codi_inputs(B, C, 7 * B + C)
    js, _ = _codi_raw(y1, y2, yn, B // 2, 0.1, pad)
    torch.testing.assert_close(js.double(), R.js_rows(y1.double(), y2.double()), rtol=1e-5, atol=1e-5)
    # near-identical models: js ~ 1e-7, float32 may return small negatives (as the reference's does)
    y3 = y1 + 1e-3 * torch.randn(B, C, generator=torch.Generator().manual_seed(B))
    js, _ = _codi_raw(y1, y3, yn, B // 2, 0.1, pad)
    torch.testing.assert_close(js.double(), R.js_rows(y1.double(), y3.double()), rtol=1e-5, atol=1e-5)
    # a column whose probability underflows in both models: 0, not NaN (xlogy's rule)
    y1[:, 0], y3[:, 0] = -300.0, -300.0
    if C > 1:
        js, _ = _codi_raw(y1, y3, yn, B // 2, 0.1, pad)
        assert torch.isfinite(js).all()
        torch.testing.assert_close(js.double(), R.js_rows(y1.double(), y3.double()), rtol=1e-5, atol=1e-5)


# --------------------------------------------------------------- graph steps

def _sage():
    import ngnn
    return ngnn.SAGE(100, 64, 47, 2, dropout=0.0).to(DEV).train()


def _small_block_setup(n_models):
    """models, their eager twins, three full blocks and noisy labels."""
    from ngnn.loader import sample_block, synthetic_graph
    g = synthetic_graph("ogbn-products", DEV, seed=1, scale=0.01)
    torch.manual_seed(3)
    models = [_sage() for _ in range(n_models)]
    twins = [_sage() for _ in range(n_models)]
    for m, t in zip(models, twins):
        t.load_state_dict(m.state_dict())
    blocks = [sample_block(g, g.train_idx[256 * i:256 * (i + 1)], [5, 4], seed=10 + i) for i in range(3)]
    gen = torch.Generator(device=DEV).manual_seed(5)
    flip = torch.rand(g.num_nodes, device=DEV, generator=gen) < 0.3
    yhn = torch.where(flip, torch.randint(0, 47, (g.num_nodes,), device=DEV, generator=gen), g.y)
    return g, models, twins, blocks, yhn


def _assert_params(m_graph, m_eager, tag):
    for (n, pg), pe in zip(m_graph.named_parameters(), m_eager.parameters()):
        torch.testing.assert_close(pg, pe, rtol=1e-4, atol=2e-6, msg=f"{tag}:{n}")


def _close(a, b):
    return abs(a - b) <= 1e-5 * max(1.0, abs(b))


def test_graphed_train_step_with_backward_correction():
    from ngnn.graphs import GraphedTrainStep, slot_size
    from ngnn.optim import Adam
    g, (m_g,), (m_e,), blocks, yhn = _small_block_setup(1)
    mat = R.pair_flip_matrix(47, 0.3)

    def loss_fn(out, y, B):
        return backward_correction(out, y, mat, 47, batch_size=B)

    o_g, o_e = Adam(m_g.parameters(), lr=1e-2), Adam(m_e.parameters(), lr=1e-2)
    n_cap, e_cap = slot_size(256, [5, 4])
    step = GraphedTrainStep(m_g, o_g, 256, n_cap, e_cap, 100, DEV, loss_fn=loss_fn)
    step.capture(blocks[0].x, blocks[0].edge_index, yhn[blocks[0].n_id])
    for b in blocks[1:]:  # two replays, and the same loop body eagerly
        lg = float(step(b.x, b.edge_index, yhn[b.n_id]))
        le = loss_fn(m_e(b.x, b.edge_index), yhn[b.n_id], 256)
        o_e.zero_grad(set_to_none=False)
        le.backward()
        o_e.step()
        assert _close(lg, float(le.detach())), (lg, float(le.detach()))
    torch.cuda.synchronize()
    _assert_params(m_g, m_e, "bc")


@pytest.mark.parametrize("forget", [0.25, 1.0])
def test_graphed_coteaching_step_with_codi(forget):
    """forget 1.0: num_remember 0 keys its own graph and keeps every row."""
    from ngnn.graphs import GraphedCoTeachingStep, slot_size
    from ngnn.optim import Adam
    g, (m1, m2), (e1, e2), blocks, yhn = _small_block_setup(2)
    clean = yhn == g.y
    n_cap, e_cap = slot_size(256, [5, 4])
    step = GraphedCoTeachingStep(m1, Adam(m1.parameters(), lr=1e-2), m2, Adam(m2.parameters(), lr=1e-2),
                                 CoDiLoss(DEV, 0.1), 256, n_cap, e_cap, 100, DEV, noise_or_not=clean)
    crit, oe1, oe2 = CoDiLoss(DEV, 0.1), Adam(e1.parameters(), lr=1e-2), Adam(e2.parameters(), lr=1e-2)
    step.capture(blocks[0].x, blocks[0].edge_index, yhn[blocks[0].n_id], blocks[0].n_id, forget)
    assert list(step._graphs) == [int((1 - forget) * 256)]
    for b in blocks[1:]:  # two replays, and the same loop body eagerly
        got = step(b.x, b.edge_index, yhn[b.n_id], b.n_id, forget)
        assert tuple(got[4:]) == (0, 0, 0, 0)
        got = [float(t) for t in got[:4]]
        want = crit(e1(b.x, b.edge_index), e2(b.x, b.edge_index), yhn[b.n_id], forget, b.n_id, clean,
                    batch_size=256)
        for o in (oe1, oe2):
            o.zero_grad(set_to_none=False)
        want[0].backward()
        oe1.step()
        want[1].backward()
        oe2.step()
        want = [float(t.detach()) for t in want[:2]]
        assert _close(got[0], want[0]) and _close(got[1], want[1]), (got, want)
        assert 0.0 <= got[2] <= 1.0 and 0.0 <= got[3] <= 1.0
    torch.cuda.synchronize()
    assert len(step._graphs) == 1
    _assert_params(m1, e1, "codi model1")
    _assert_params(m2, e2, "codi model2")


def test_codi_short_block_runs_eagerly():
    from ngnn.graphs import GraphedCoTeachingStep, slot_size
    from ngnn.loader import sample_block
    from ngnn.optim import Adam
    g, (m1, m2), _, blocks, yhn = _small_block_setup(2)
    n_cap, e_cap = slot_size(256, [5, 4])
    step = GraphedCoTeachingStep(m1, Adam(m1.parameters()), m2, Adam(m2.parameters()),
                                 CoDiLoss(DEV, 0.1, return_indices=True), 256, n_cap, e_cap, 100, DEV,
                                 noise_or_not=torch.ones(g.num_nodes, dtype=torch.bool, device=DEV))
    short = sample_block(g, g.train_idx[256:356], [5, 4], seed=2)
    out = step(short.x, short.edge_index, yhn[short.n_id], short.n_id, 0.25, batch_size=100)
    torch.cuda.synchronize()
    assert out[4].numel() == 75 and out[6].numel() == 25 and not step._graphs
    assert torch.isfinite(out[0]) and torch.isfinite(out[1]) and float(out[2]) == 1.0
