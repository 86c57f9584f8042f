"""Restatements for the shuffle_pos / contrastive-loss tests (a helper, not a
test): the exact draw of ngnn_shuffle_rows (include/ngnn.h) in numpy uint64,
and the reference's Discriminator_innerprod + BCEExeprtLoss op sequence
(src/utils/data_utils.py:34-64) in torch, dtype-generic so that it runs in
float64."""
import numpy as np
import torch

_U = np.uint64
ROW_SALT = _U(0x632BE59BD9B4E019)
PERM_SALT = _U(0xD1B54A32D192ED03)


def mix64(z):
    """The sampler's mixer (ngnn_sample_dev.h), on uint64 arrays, modulo 2^64."""
    with np.errstate(over="ignore"):
        z = np.asarray(z, dtype=_U) + _U(0x9E3779B97F4A7C15)
        z = (z ^ (z >> _U(30))) * _U(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> _U(27))) * _U(0x94D049BB133111EB)
        return z ^ (z >> _U(31))


def shuffle_selection(n_rows: int, F: int, m: int, seed: int):
    """(S, rho): S [n_rows, m] the selected columns of every row in ascending
    order (p_0 < ... < p_{m-1}); rho [n_rows, m] with out[r, S[r, j]] =
    x[r, S[r, rho[r, j]]]."""
    with np.errstate(over="ignore"):
        r = np.arange(n_rows, dtype=_U)
        c = np.arange(F, dtype=_U)
        b1 = mix64(_U(seed) ^ mix64(r + ROW_SALT))
        key1 = mix64(b1[:, None] + c[None, :])
        order = np.argsort(key1, axis=1, kind="stable")  # ties by column
        S = np.sort(order[:, :m], axis=1)
        b2 = mix64(b1 ^ PERM_SALT)
        key2 = mix64(b2[:, None] + S.astype(_U))
    by_rank = np.argsort(key2, axis=1, kind="stable")  # by_rank[r, t] = the j of rank t (ties by p_j)
    rho = np.empty_like(by_rank)
    np.put_along_axis(rho, by_rank, np.broadcast_to(np.arange(m), by_rank.shape), axis=1)
    return S, rho


def upper_half_shortcut_fails(row: int, F: int, m: int, seed: int):
    """(stage 1, stage 2) for one row: would ranks counted on the keys' upper
    32 bits alone (the narrow kernel's fast path) differ from the exact ones
    where it matters -- more than m columns below the threshold, or ranks
    within S_r that are not a permutation?  True: that row must take the
    kernel's exact path."""
    with np.errstate(over="ignore"):
        b1 = mix64(_U(seed) ^ mix64(_U(row) + ROW_SALT))
        hi1 = mix64(b1 + np.arange(F, dtype=_U)) >> _U(32)
        S, _ = shuffle_selection(row + 1, F, m, seed)
        hi2 = mix64(mix64(b1 ^ PERM_SALT) + S[row].astype(_U)) >> _U(32)
    a1 = (hi1[None, :] < hi1[:, None]).sum(axis=1)
    a2 = (hi2[None, :] < hi2[:, None]).sum(axis=1)
    return int((a1 < m).sum()) != m, int(a2.sum()) != m * (m - 1) // 2


def shuffle_rows_ref(x, m: int, seed: int):
    """ngnn_shuffle_rows(x, m, seed) on a numpy [N, F] array: a new array."""
    x = np.asarray(x)
    out = x.copy()
    N, F = x.shape
    if m <= 0 or N == 0:
        return out
    S, rho = shuffle_selection(N, F, m, seed)
    src = np.take_along_axis(S, rho, axis=1)
    np.put_along_axis(out, S, np.take_along_axis(x, src, axis=1), axis=1)
    return out


def contrast_ref(h, hp, hn, idx):
    """The reference's op sequence: three row gathers, Discriminator_innerprod
    (two mul + sum with keepdim), BCEExeprtLoss (two squeezes, two
    BCEWithLogitsLoss against ones / zeros, added).  Differentiable in h, hp,
    hn; any float dtype."""
    H, Hp, Hn = h[idx], hp[idx], hn[idx]
    logits_pa = torch.sum(torch.mul(H, Hp), dim=1, keepdim=True)
    logits_n = torch.sum(torch.mul(H, Hn), dim=1, keepdim=True)
    lp, ln = torch.squeeze(logits_pa), torch.squeeze(logits_n)
    crit = torch.nn.BCEWithLogitsLoss()
    return crit(lp, torch.ones_like(lp)) + crit(ln, torch.zeros_like(ln))


def contrast_ref_f64(h, hp, hn, idx, scale: float = 1.0):
    """(loss, dh, dhp, dhn) of ``scale * contrast_ref`` run in float64 on the
    CPU from any tensors: the GPU tests' yardstick."""
    a, p, n = (t.detach().double().cpu().clone().requires_grad_(True) for t in (h, hp, hn))
    loss = contrast_ref(a, p, n, idx.detach().cpu())
    (loss * scale).backward()
    return loss.detach(), a.grad, p.grad, n.grad


def relu_inputs(N: int, H: int, seed: int, scale: float = 0.25, dtype=torch.float32):
    """h, hp, hn = relu(scale * randn): hidden activations after SAGE's ReLU."""
    g = torch.Generator().manual_seed(seed)
    return tuple(torch.relu(scale * torch.randn(N, H, generator=g, dtype=torch.float32)).to(dtype)
                 for _ in range(3))
