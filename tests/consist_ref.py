"""Restatement of the reference's uncertainty-weighted consistency term
(src/utils/losses.py:185-246: get_uncertainty_batch, fix_cr), written from
its op sequence in plain torch so that it runs in float64: the yardstick of
tests/test_consist_gpu.py, pinned to the reference's own module by
tests/test_consist_ref.py through the fixtures of
tests/golden/make_golden_consist.py.

Also the closed-form gradients the HIP kernels implement (fix_cr_grads) and
the input builders the tests and the fixture generator share.
"""
import math

import torch

ENT_EPS = 1e-5


def uncertainty(edge_index, y_pure, nbr_classes, epsilon=1e-16):
    """w[i] = exp(-H(ptc_i) / log2(nbr_classes)), ptc_i the mean of exp(y_pure)
    over the edges whose edge_index[0] is i, taken at edge_index[1] (the
    reference's coo(row=edge_index[0], col=edge_index[1]) @ p)."""
    p = torch.exp(y_pure)
    n = p.size(0)
    s = torch.zeros_like(p).index_add_(0, edge_index[0], p[edge_index[1]])
    deg = torch.zeros(n, dtype=p.dtype).index_add_(0, edge_index[0], torch.ones(edge_index.size(1), dtype=p.dtype))
    ptc = s / (deg.view(-1, 1) + epsilon)
    h = -(ptc * torch.log2(ptc + ENT_EPS)).sum(1)
    return torch.exp(-h / math.log2(nbr_classes))


def keep_mask(y_pure, batch_size, p_cutoff):
    pp = torch.exp(y_pure[:batch_size])
    return pp.max(dim=-1).values >= p_cutoff


def fix_cr(y_pure, y_noisy, batch_size=512, name="ce", p_cutoff=0.0, use_hard_labels=True, w=None):
    """The loss, differentiable in y_pure and y_noisy (any float dtype)."""
    assert name in ("ce", "l2")
    yp, yn = y_pure[:batch_size], y_noisy[:batch_size]
    if name == "l2":
        return ((yn - yp) ** 2).mean()
    pp, pn = torch.exp(yp), torch.exp(yn)
    top, idx = torch.max(pp, dim=-1)
    mask = (top >= p_cutoff).to(pp.dtype)
    lsm = torch.log_softmax(pn, dim=-1)  # the probabilities as logits, as the reference
    if use_hard_labels:
        rows = -lsm.gather(1, idx.view(-1, 1)).squeeze(1)
    else:
        rows = -(pp * lsm).sum(1)
    rows = rows * mask
    if w is not None:
        rows = w[:batch_size] * rows
    return rows.mean()


def fix_cr_grads(y_pure, y_noisy, batch_size=512, name="ce", p_cutoff=0.0, use_hard_labels=True, w=None, g=1.0):
    """The closed forms of include/ngnn.h (ngnn_fix_cr_*): (d y_pure, d y_noisy)
    on the rows < B, for the incoming gradient g."""
    yp, yn = y_pure[:batch_size].detach(), y_noisy[:batch_size].detach()
    B, C = yp.shape
    if name == "l2":
        d = 2.0 * g * (yn - yp) / (B * C)
        return -d, d
    pp, pn = torch.exp(yp), torch.exp(yn)
    top, idx = torch.max(pp, dim=-1)
    m = (top >= p_cutoff).to(pp.dtype)
    wr = torch.ones(B, dtype=pp.dtype) if w is None else w[:B].to(pp.dtype)
    c = (g * m * wr / B).view(-1, 1)
    lsm = torch.log_softmax(pn, dim=-1)
    s = torch.exp(lsm)
    if use_hard_labels:
        onehot = torch.zeros_like(pp).scatter_(1, idx.view(-1, 1), 1.0)
        return torch.zeros_like(pp), c * (s - onehot) * pn
    return -c * pp * lsm, c * (s * pp.sum(1, keepdim=True) - pp) * pn


# ------------------------------------------------------------------ inputs

def log_probs(n, c, scale, seed):
    """float32 log-softmax rows of scale * N(0, 1) logits."""
    g = torch.Generator().manual_seed(seed)
    return torch.log_softmax(scale * torch.randn(n, c, generator=g), dim=1)


def admissible(y_pure, batch_size, p_cutoff, need_both=True):
    """The three conditions under which no comparison hinges on rounding: on
    rows < B the top two of exp(y_pure) differ by >= 1e-3 relative, no row's
    maximum lies within 1e-3 relative of p_cutoff, and (need_both) at least
    one row is masked out and one kept.  Returns (ok, kept rows)."""
    pp = torch.exp(y_pure[:batch_size].double())
    if pp.size(1) > 1:
        top2 = pp.topk(2, dim=1).values
        if bool(((top2[:, 0] - top2[:, 1]) < 1e-3 * top2[:, 0]).any()):
            return False, 0
    top = pp.max(1).values
    if p_cutoff > 0 and bool(((top - p_cutoff).abs() < 1e-3 * p_cutoff).any()):
        return False, 0
    kept = int((top >= p_cutoff).sum())
    if need_both and not 0 < kept < batch_size:
        return False, kept
    return True, kept


def admissible_pair(n, c, batch_size, scale, p_cutoff, seed, need_both=True):
    """(y_pure, y_noisy, seed used, kept): the seed walked upward until
    `admissible` holds."""
    for s in range(seed, seed + 1000):
        yp = log_probs(n, c, scale, s)
        ok, kept = admissible(yp, batch_size, p_cutoff, need_both)
        if ok:
            return yp, log_probs(n, c, scale, s + 100003), s, kept
    raise AssertionError(f"no admissible seed from {seed} on (n={n}, c={c}, B={batch_size}, cutoff={p_cutoff})")


def graph_edges(n, e, seed, hub=0, hub_deg=200, lone=1):
    """[2, ~e] int64 edges in random order, neither row sorted: a source `hub`
    with >= hub_deg out-edges, one exact duplicate edge, one self-loop, and a
    source `lone` without out-edges."""
    g = torch.Generator().manual_seed(seed)
    src = torch.randint(0, n, (e,), generator=g)
    dst = torch.randint(0, n, (e,), generator=g)
    keep = src != lone
    src, dst = src[keep], dst[keep]
    if n > 2:
        hs = torch.full((hub_deg,), hub, dtype=torch.long)
        hd = torch.randint(0, n, (hub_deg,), generator=g)
        loop = 2 if n > 2 else 0
        src = torch.cat([src, hs, src[:1], torch.tensor([loop])])
        dst = torch.cat([dst, hd, dst[:1], torch.tensor([loop])])
    perm = torch.randperm(src.numel(), generator=g)
    return torch.stack([src[perm], dst[perm]])
