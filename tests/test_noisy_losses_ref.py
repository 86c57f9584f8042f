"""tests/losses_noisy_ref.py (the float64 yardstick of the GPU tests) against
the reference's own backward_correction and CoDiLoss: the fixtures
tests/golden/bc_*.npz and codi_*.npz (made by make_golden_noisy_losses.py
from the reference's module) -- kept sets and pure ratios exactly, losses
and gradients at rtol 1e-6 -- and hand-computed known answers."""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import losses_noisy_ref as R
from oracle.losses_ref import ct_loss


@pytest.mark.parametrize("name", ["codi_b300", "codi_b1024"])
def test_codi_restatement_vs_reference_fixture(golden_dir, name):
    g = np.load(os.path.join(golden_dir, name + ".npz"))
    y1 = torch.from_numpy(g["y1"]).requires_grad_(True)
    y2 = torch.from_numpy(g["y2"]).requires_grad_(True)
    out = R.codi_loss(y1, y2, torch.from_numpy(g["y_noise"]), float(g["forget_rate"]),
                      torch.from_numpy(g["ind"]), torch.from_numpy(g["noise_or_not"]),
                      co_lambda=float(g["co_lambda"]))
    assert torch.equal(out[4].sort().values, torch.from_numpy(g["ind_1_update"]))
    assert torch.equal(out[5].sort().values, torch.from_numpy(g["ind_2_update"]))
    assert float(out[2]) == float(g["pure_ratio_1"]) and float(out[3]) == float(g["pure_ratio_2"])
    torch.testing.assert_close(out[0].detach(), torch.from_numpy(g["loss_1"]), rtol=1e-6, atol=0)
    torch.testing.assert_close(out[1].detach(), torch.from_numpy(g["loss_2"]), rtol=1e-6, atol=0)
    out[0].backward()
    out[1].backward()
    for got, want in ((y1.grad, g["grad_y1"]), (y2.grad, g["grad_y2"])):
        want = torch.from_numpy(want)
        torch.testing.assert_close(got, want, rtol=1e-6, atol=0)
    # the float64 run, the GPU tests' yardstick, selects the same rows
    d = R.codi_loss(y1.detach().double(), y2.detach().double(), torch.from_numpy(g["y_noise"]),
                    float(g["forget_rate"]), torch.from_numpy(g["ind"]), torch.from_numpy(g["noise_or_not"]),
                    co_lambda=float(g["co_lambda"]))
    assert torch.equal(d[4].sort().values, torch.from_numpy(g["ind_1_update"]))
    assert torch.equal(d[5].sort().values, torch.from_numpy(g["ind_2_update"]))


@pytest.mark.parametrize("name", ["bc_b300", "bc_b65"])
def test_bc_restatement_vs_reference_fixture(golden_dir, name):
    g = np.load(os.path.join(golden_dir, name + ".npz"))
    x = torch.from_numpy(g["output"]).requires_grad_(True)
    y = torch.from_numpy(g["labels"])
    loss = R.backward_correction(x, y, g["C"], x.size(1))
    torch.testing.assert_close(loss.detach(), torch.from_numpy(g["loss"]), rtol=1e-6, atol=0)
    loss.backward()
    want = torch.from_numpy(g["grad_output"])
    torch.testing.assert_close(x.grad, want, rtol=1e-6, atol=0)
    low, high, near = R.clamp_stats(x.detach())
    assert low >= 1 and near >= 1e-3  # (what the generator asserted: the clamp is exercised, nothing on its edge)
    # the closed-form gradient the device kernel evaluates, in float64, against autograd
    xd = x.detach().double().requires_grad_(True)
    R.backward_correction(xd, y, g["C"], x.size(1)).backward()
    B, C = xd.shape
    w = R.correction_inverse(g["C"]).double()[y]
    p = torch.softmax(xd.detach(), dim=1)
    m = ((p >= R.CLAMP_LO) & (p <= R.CLAMP_HI)).double()
    closed = -(w * m - p * (w * m).sum(1, keepdim=True)) / (B * C)
    assert float((closed - xd.grad).abs().max()) <= 1e-12 * float(xd.grad.abs().max())


def test_bc_identity_matrix_is_clamped_nll_over_c():
    # C = 2, B = 2, identity correction: -mean(onehot * log q) = sum_r -log q[r, y_r] / (B C)
    x = torch.tensor([[0.0, math.log(3.0)], [20.0, 0.0]], dtype=torch.float64)
    y = torch.tensor([1, 1])
    loss = R.backward_correction(x, y, np.eye(2), 2)
    # row 0: p = (1/4, 3/4); row 1: p_1 = 1 / (1 + e^20) ~ 2.06e-9, clamped to 1e-5
    want = (-math.log(0.75) - math.log(1e-5)) / 4
    assert float(loss) == pytest.approx(want, rel=1e-12)
    # the clamped entry passes no gradient: row 1's gradient is zero
    x.requires_grad_(True)
    R.backward_correction(x, y, np.eye(2), 2).backward()
    assert torch.equal(x.grad[1], torch.zeros(2, dtype=torch.float64))
    torch.testing.assert_close(x.grad[0], torch.tensor([0.25, -0.25], dtype=torch.float64) / 4)


def test_codi_equal_models_has_zero_js_and_reduces_to_ctloss():
    y = R.logits(64, 5, 2.0, 1, torch.float64)
    yn = torch.randint(0, 5, (64,), generator=torch.Generator().manual_seed(2))
    ind, clean = torch.arange(64), torch.rand(64, generator=torch.Generator().manual_seed(3)) < 0.5
    js = R.js_rows(y, y)
    assert float(js.abs().max()) <= 1e-15
    got = R.codi_loss(y, y.clone(), yn, 0.25, ind, clean, co_lambda=1.0)
    want = ct_loss(y, y.clone(), yn, 0.25, ind, clean)
    for k in range(4):
        assert float(got[k]) == pytest.approx(float(want[k]), rel=1e-14), k
    for k in range(4, 8):
        assert torch.equal(got[k], want[k]), k


def test_codi_js_known_answer_and_xlogy_rule():
    # p = (1, 0), q = (1/2, 1/2) up to e^-200: mean = (3/4, 1/4)
    y1 = torch.tensor([[0.0, -200.0]], dtype=torch.float64)
    y2 = torch.zeros(1, 2, dtype=torch.float64)
    # sum_k mean_k (log mean_k - (lp_k + lq_k) / 2), lp = (0, -200), lq = (log 1/2, log 1/2)
    want = 0.75 * (math.log(0.75) - math.log(0.5) / 2) + 0.25 * (math.log(0.25) - (-200 + math.log(0.5)) / 2)
    assert float(R.js_rows(y1, y2)[0]) == pytest.approx(want, rel=1e-12)
    # both probabilities underflow to 0 in one column: that term is 0 (xlogy), not NaN
    y1 = torch.tensor([[0.0, -2000.0]], dtype=torch.float64)
    assert float(R.js_rows(y1, y1)[0]) == 0.0


def test_codi_forget_everything_keeps_every_row():
    B = 10
    y1, y2 = R.logits(B, 4, 2.0, 5), R.logits(B, 4, 2.0, 6)
    yn = torch.arange(B) % 4
    clean = torch.arange(B) < 3
    out = R.codi_loss(y1, y2, yn, 1.0, None, clean)
    assert out[4].numel() == B and out[5].numel() == B and out[6].numel() == 0
    torch.testing.assert_close(out[0], F.cross_entropy(y1, yn))
    torch.testing.assert_close(out[1], F.cross_entropy(y2, yn))
    assert float(out[2]) == pytest.approx(0.3) and float(out[3]) == pytest.approx(0.3)


def test_flip_matrices():
    u, p = R.uniform_flip_matrix(5, 0.3), R.pair_flip_matrix(5, 0.3)
    np.testing.assert_allclose(u.sum(1), 1.0)
    np.testing.assert_allclose(p.sum(1), 1.0)
    assert np.array_equal(u, u.T) and not np.array_equal(p, p.T)
    inv = np.linalg.inv(p)
    assert np.abs(inv - inv.T).max() > 0.1  # a transposed read of the inverse cannot pass
