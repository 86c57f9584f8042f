"""tests/consist_ref.py (the yardstick of tests/test_consist_gpu.py) against
the reference-generated fixtures tests/golden/consist_*.npz, its closed-form
gradients against float64 autograd, and known answers by hand.  CPU only."""
import math
import os

import numpy as np
import pytest
import torch

import consist_ref as R

CASES = ["consist_b300", "consist_b65"]
MODES = {"hard": ("ce", True), "soft": ("ce", False), "l2": ("l2", True)}


def _load(golden_dir, name):
    g = np.load(os.path.join(golden_dir, name + ".npz"))
    t = {k: torch.from_numpy(np.asarray(g[k])) for k in g.files}
    return t, int(t["B"]), int(t["C"]), float(t["p_cutoff"])


@pytest.mark.parametrize("name", CASES)
def test_fixture_holds_what_the_tests_rely_on(golden_dir, name):
    t, B, C, cutoff = _load(golden_dir, name)
    ei = t["edge_index"]
    deg = torch.bincount(ei[0], minlength=t["y_pure"].size(0))
    assert int(deg[:B].max()) >= 200 and int(deg[:B].min()) == 0
    assert bool((ei[0] == ei[1]).any()) and torch.unique(ei, dim=1).size(1) < ei.size(1)
    assert bool((ei[0][1:] < ei[0][:-1]).any()) and bool((ei[1][1:] < ei[1][:-1]).any())
    ok, kept = R.admissible(t["y_pure"], B, cutoff)
    assert ok and 0 < kept < B
    assert os.path.getsize(os.path.join(golden_dir, name + ".npz")) < 517713  # the largest fixture before these


@pytest.mark.parametrize("name", CASES)
def test_restatement_matches_the_reference_fixture(golden_dir, name):
    t, B, C, cutoff = _load(golden_dir, name)
    ei, yp, yn = t["edge_index"], t["y_pure"].double(), t["y_noisy"].double()
    w = R.uncertainty(ei, yp, C)
    torch.testing.assert_close(w, t["w"].double(), rtol=1e-6, atol=0)
    assert torch.equal(R.keep_mask(yp, B, cutoff), t["mask"])
    assert torch.equal(R.keep_mask(t["y_pure"], B, cutoff), t["mask"])  # and in float32
    for mode, (nm, hard) in MODES.items():
        a, b = yp.clone().requires_grad_(True), yn.clone().requires_grad_(True)
        loss = R.fix_cr(a, b, B, nm, cutoff, hard, w)
        torch.testing.assert_close(loss.detach(), t[f"{mode}/loss"].double(), rtol=1e-6, atol=0)
        loss.backward()
        for got, key in ((a.grad, "grad_pure"), (b.grad, "grad_noisy")):
            want = t[f"{mode}/{key}"].double()
            got = torch.zeros_like(want) if got is None else got[:B]
            # the fixture is the reference's float32: an entry is a difference of
            # terms up to the tensor's largest, each rounded to 2^-24 of itself,
            # so next to rtol it carries a few 2^-24 of that maximum absolutely
            # (measured: 1e-9 of it, on an entry 1e-4 of it)
            torch.testing.assert_close(got, want, rtol=1e-6, atol=4 * 2.0 ** -24 * float(want.abs().max()))
        if mode != "l2":
            torch.testing.assert_close(R.fix_cr(yp, yn, B, nm, cutoff, hard, None),
                                       t[f"{mode}/loss_w_none"].double(), rtol=1e-6, atol=0)
            torch.testing.assert_close(R.fix_cr(yp, yn, B, nm, 0.0, hard, w),
                                       t[f"{mode}/loss_cutoff0"].double(), rtol=1e-6, atol=0)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("with_w", [False, True])
def test_closed_form_gradients_match_float64_autograd(mode, with_w):
    nm, hard = MODES[mode]
    N, C, B, cutoff = 40, 11, 33, 0.4
    yp, yn, _, _ = R.admissible_pair(N, C, B, 2.0, cutoff, 7)
    yp, yn = yp.double(), yn.double()
    w = torch.rand(N, dtype=torch.float64, generator=torch.Generator().manual_seed(1)) if with_w else None
    for g in (1.0, -2.5):
        a, b = yp.clone().requires_grad_(True), yn.clone().requires_grad_(True)
        (R.fix_cr(a, b, B, nm, cutoff, hard, w) * g).backward()
        dp, dn = R.fix_cr_grads(yp, yn, B, nm, cutoff, hard, w, g)
        for got, auto in ((dp, a.grad), (dn, b.grad)):
            auto = torch.zeros(N, C, dtype=torch.float64) if auto is None else auto
            assert torch.count_nonzero(auto[B:]) == 0
            assert float((got - auto[:B]).abs().max()) <= 1e-12 * max(float(auto.abs().max()), 1e-300)
    if mode != "l2":
        assert float(b.grad.abs().max()) > 0


def _onehot_logp(c, k):
    p = torch.full((c,), 1e-30, dtype=torch.float64)
    p[k] = 1.0
    return torch.log(p)


def test_uncertainty_known_answers():
    C = 5
    uni = torch.full((C,), math.log(1.0 / C), dtype=torch.float64)
    y = torch.stack([uni, _onehot_logp(C, 2), _onehot_logp(C, 0), _onehot_logp(C, 1), _onehot_logp(C, 2),
                     _onehot_logp(C, 3), _onehot_logp(C, 4), uni])
    # 0 -> 1 (one-hot neighbour); 7 -> 2, 3, 4, 5, 6 (they average to uniform);
    # 3 -> 3 twice (a self-loop, duplicated); 1, 2, 4, 5, 6 have no out-edges
    ei = torch.tensor([[7, 0, 7, 3, 7, 7, 3, 7], [2, 1, 3, 3, 4, 5, 3, 6]])
    w = R.uncertainty(ei, y, C)
    for i in (1, 2, 4, 5, 6):
        assert float(w[i]) == 1.0
    assert float(w[0]) == pytest.approx(math.exp(-(-math.log2(1 + 1e-5)) / math.log2(C)), rel=1e-12)
    assert float(w[3]) == pytest.approx(float(w[0]), rel=1e-12)
    want = math.exp(-(-math.log2(1.0 / C + 1e-5)) / math.log2(C))
    assert float(w[7]) == pytest.approx(want, rel=1e-9)
    assert float(w[7]) == pytest.approx(math.exp(-1.0), rel=1e-4)  # exp(-log2 C / log2 C) up to the 1e-5 term
    # grouped by edge_index[0]: the flipped graph answers differently
    assert float(R.uncertainty(ei.flip(0), y, C)[1]) != 1.0


def test_fix_cr_known_answers():
    C, B = 4, 3
    yp = torch.log_softmax(torch.tensor([[1.0, 3.0, 3.0, 0.0], [2.0, 0.0, 1.0, 0.5], [0.0, 0.0, 0.0, 0.0]],
                                        dtype=torch.float64), dim=1)
    yn = torch.log_softmax(torch.tensor([[0.3, 0.1, 2.0, 0.0], [0.0, 1.0, 0.0, 0.2], [1.0, 0.0, 0.5, 0.0]],
                                        dtype=torch.float64), dim=1)
    assert float(yp[0, 1]) == float(yp[0, 2]) and float(yp[2, 0]) == float(yp[2, 3])  # bitwise ties
    # a tie picks the first index: rows 0 and 2 take columns 1 and 0
    lsm = torch.log_softmax(torch.exp(yn), dim=1)
    want = -(lsm[0, 1] + lsm[1, 0] + lsm[2, 0]) / 3
    assert float(R.fix_cr(yp, yn, B)) == pytest.approx(float(want), rel=1e-14)
    _, dn = R.fix_cr_grads(yp, yn, B)
    assert float(dn[0, 1]) < 0 < float(dn[0, 2])
    # p_cutoff above every maximum: loss 0, zero gradients
    for hard in (True, False):
        a, b = yp.clone().requires_grad_(True), yn.clone().requires_grad_(True)
        loss = R.fix_cr(a, b, B, "ce", 0.99, hard)
        loss.backward()
        assert float(loss.detach()) == 0.0
        assert a.grad is None or torch.count_nonzero(a.grad) == 0
        assert torch.count_nonzero(b.grad) == 0
        dp, dn = R.fix_cr_grads(yp, yn, B, "ce", 0.99, hard)
        assert torch.count_nonzero(dp) == 0 and torch.count_nonzero(dn) == 0
    # l2 ignores w (and p_cutoff), and batch_size past the rows takes them all
    w = torch.tensor([0.1, 0.2, 0.3], dtype=torch.float64)
    assert float(R.fix_cr(yp, yn, B, "l2", 0.99, True, w)) == float(((yn - yp) ** 2).mean())
    assert float(R.fix_cr(yp, yn, 512)) == float(R.fix_cr(yp, yn, B))
    # the mean runs over all B rows, masked ones included
    top = torch.exp(yp).max(1).values
    cut = float(top.sort().values[1]) - 1e-6  # keeps two of three rows
    kept = top >= cut
    assert int(kept.sum()) == 2
    want = -(lsm[torch.arange(3), torch.max(torch.exp(yp), dim=-1).indices] * kept).sum() / 3
    assert float(R.fix_cr(yp, yn, B, "ce", cut)) == pytest.approx(float(want), rel=1e-14)
