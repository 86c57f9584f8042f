"""tests/contrast_ref.py (the yardsticks of the GPU tests) on the CPU:
contrast_ref against the reference's own Discriminator_innerprod +
BCEExeprtLoss (the fixtures tests/golden/contrast_*.npz, made by
make_golden_contrast.py from the reference's module), and the draw of
shuffle_rows_ref: its invariants -- shared with the reference's shuffle_pos,
run from a checkout when NGNN_REFERENCE names one -- and its statistics."""
import importlib
import os
import sys

import numpy as np
import pytest
import torch

import contrast_ref as R
from gradbar import assert_wgrad

FIXTURES = ["contrast_n128_h130", "contrast_n64_h512"]


@pytest.mark.parametrize("name", FIXTURES)
def test_contrast_restatement_vs_reference_fixture(golden_dir, name):
    g = np.load(os.path.join(golden_dir, name + ".npz"))
    h, hp, hn = (torch.from_numpy(g[k]).requires_grad_(True) for k in ("h", "hp", "hn"))
    idx = torch.from_numpy(g["idx"])
    assert idx.unique().numel() == idx.numel()
    loss = R.contrast_ref(h, hp, hn, idx)
    torch.testing.assert_close(loss.detach(), torch.from_numpy(g["loss"]), rtol=1e-5, atol=1e-6)
    loss.backward()
    for t, k in ((h, "grad_h"), (hp, "grad_hp"), (hn, "grad_hn")):
        assert_wgrad(t.grad, torch.from_numpy(g[k]), f"{name} {k}")
    # the float64 run, the GPU tests' yardstick, against the same fixture
    l64, *g64 = R.contrast_ref_f64(h, hp, hn, idx)
    torch.testing.assert_close(l64.float(), torch.from_numpy(g["loss"]), rtol=1e-5, atol=1e-6)
    for got, k in zip(g64, ("grad_h", "grad_hp", "grad_hn")):
        assert_wgrad(torch.from_numpy(g[k]), got, f"{name} {k} vs float64")


def test_contrast_known_answer():
    # one row: a = 3, b = -1 -> softplus(-3) + softplus(-1)
    h = torch.tensor([[1.0, 2.0]], dtype=torch.float64)
    hp = torch.tensor([[1.0, 1.0]], dtype=torch.float64)
    hn = torch.tensor([[1.0, -1.0]], dtype=torch.float64)
    want = np.log1p(np.exp(-3.0)) + np.log1p(np.exp(-1.0))
    assert float(R.contrast_ref(h, hp, hn, torch.tensor([0]))) == pytest.approx(want, rel=1e-14)


def _check_invariants(x, out, m):
    assert out.shape == x.shape
    assert np.array_equal(np.sort(out, axis=1), np.sort(x, axis=1))  # every row a permutation of its input row
    assert int((out != x).sum(axis=1).max(initial=0)) <= m           # at most m positions differ
    if m <= 1:
        assert np.array_equal(out, x)


@pytest.mark.parametrize("F,m", [(1, 0), (1, 1), (7, 0), (7, 1), (7, 2), (7, 7), (100, 70), (100, 99),
                                 (100, 100), (257, 179), (767, 536)])
def test_shuffle_rows_ref_invariants(F, m):
    N = 37
    x = np.random.default_rng(F * 1000 + m).standard_normal((N, F)).astype(np.float32)
    out = R.shuffle_rows_ref(x, m, seed=99)
    _check_invariants(x, out, m)
    assert np.array_equal(out, R.shuffle_rows_ref(x, m, seed=99))
    if m >= 7:
        assert not np.array_equal(out, R.shuffle_rows_ref(x, m, seed=100))
        assert not np.array_equal(out, x)
    # a pure function of the row: a prefix of the rows shuffles the same way
    assert np.array_equal(out[:5], R.shuffle_rows_ref(x[:5], m, seed=99))


def test_shuffle_selection_is_sorted_and_rho_a_permutation():
    S, rho = R.shuffle_selection(50, 100, 70, seed=5)
    assert S.shape == rho.shape == (50, 70)
    assert (np.diff(S, axis=1) > 0).all() and S.min() >= 0 and S.max() < 100
    assert np.array_equal(np.sort(rho, axis=1), np.broadcast_to(np.arange(70), (50, 70)))


def test_upper_half_tie_cases_are_what_they_claim():
    """The seeds of test_contrast_gpu.UPPER_HALF_TIES (found by search over
    seeds at F = 256, 1025 rows): in the named row two keys agree in their
    upper 32 bits and differ below, in the order opposite to their columns."""
    assert R.upper_half_shortcut_fails(372, 256, 197, seed=61) == (True, False)
    assert R.upper_half_shortcut_fails(683, 256, 256, seed=35) == (False, True)
    assert R.upper_half_shortcut_fails(5, 100, 70, seed=1234) == (False, False)
    S, _ = R.shuffle_selection(373, 256, 197, seed=61)
    assert 49 in S[372] and 6 not in S[372]        # the lower halves decide, not the column
    S, rho = R.shuffle_selection(684, 256, 256, seed=35)
    assert rho[683, 212] + 1 == rho[683, 162]


def test_mix64_known_values():
    # splitmix64's first outputs from state 0 are mix64(0), mix64(golden), ... (Vigna's reference vectors)
    assert int(R.mix64(np.uint64(0))) == 0xE220A8397B1DCDAF
    assert int(R.mix64(np.uint64(0x9E3779B97F4A7C15))) == 0x6E789E6AA1B965F4


def test_reference_shuffle_pos_shares_the_invariants():
    ref = os.environ.get("NGNN_REFERENCE")
    if not ref or not os.path.isdir(ref):
        pytest.skip("NGNN_REFERENCE does not name a reference checkout")
    if ref not in sys.path:
        sys.path.insert(0, ref)
    aug = importlib.import_module("src.utils.augmentation")
    torch.manual_seed(7)
    for F, prob in ((100, 0.7), (128, 0.9), (7, 0.1), (7, 0.2)):
        x = torch.randn(33, F)
        out = aug.shuffle_pos(x, "cpu", prob)
        assert not out.requires_grad
        _check_invariants(x.numpy(), out.numpy(), int(F * prob))


def test_shuffle_statistics():
    """N = 4096 rows of arange(F), F = 100, m = 70: every column is selected
    with probability p = m / F (its count within 6 binomial standard
    deviations of N p), and a uniform permutation of m values has one fixed
    point on average, standard deviation 1 per row, so the mean over N rows
    lies within 6 / sqrt(N) = 6 / 64 of 1."""
    N, F, m = 4096, 100, 70
    S, rho = R.shuffle_selection(N, F, m, seed=1234)
    p = m / F
    counts = np.bincount(S.ravel(), minlength=F)
    assert np.abs(counts - N * p).max() <= 6 * np.sqrt(N * p * (1 - p))
    fixed = (rho == np.arange(m)[None, :]).sum(axis=1)
    assert abs(fixed.mean() - 1.0) <= 6 / 64
    # the same through the values: rows equal to arange(F)
    x = np.broadcast_to(np.arange(F, dtype=np.float32), (N, F))
    out = R.shuffle_rows_ref(x, m, seed=1234)
    moved = (out != x).sum(axis=1)
    assert np.array_equal(moved, m - fixed)
