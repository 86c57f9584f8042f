"""The float64 restatements of tests/layer_bwd_ref.py checked without a GPU:
against torch autograd of the oracle's SAGEConv in float64, against the
oracle's plain-C edge-order backward (bitwise), and -- the input self-check --
that the case inputs of tests/test_layer_bwd_gpu.py are benign: a plain fp32
torch evaluation of every case sits ten times inside the weight-gradient bar
(rel = 1e-6), so the GPU tests never meet or miss the 1e-5 bar because of
their inputs.
"""
import numpy as np
import pytest
import torch

import layer_bwd_ref as lr
from gradbar import assert_wgrad
from oracle import c_agg, pyg_ref

N = lr.N_NODES
EI = lr.make_block()
F64 = dict(rtol=1e-10, atol=1e-12)


def test_block_has_the_edge_cases():
    src, dst = EI[0], EI[1]
    E = EI.size(1)
    assert 3800 <= E <= 4200 and int(EI.min()) >= 0 and int(EI.max()) < N
    indeg, outdeg = torch.bincount(dst, minlength=N), torch.bincount(src, minlength=N)
    assert int(indeg[lr.HUB_DST]) == lr.HUB_DEG and int(outdeg[lr.HUB_SRC]) == lr.HUB_DEG
    assert int((indeg[:63] == 0).sum()) >= 40           # edgeless targets below every R >= 63
    assert int((outdeg == 0).sum()) >= 30                # sources without out-edges
    assert int((src == dst).sum()) >= 30                 # self-loops
    assert E - torch.unique(EI, dim=1).size(1) >= 40     # duplicate edges
    for R in (63, 64, 65, 130):
        assert int((indeg[R:] > 0).sum()) > 0            # targets at or past R with in-edges
        assert R < lr.rnext_of(EI, R) < N                # sources at or past R feed rows below R
    assert lr.rnext_of(EI, 0) == 0 and lr.rnext_of(EI, N) == N
    assert not bool((dst[1:] >= dst[:-1]).all())         # edge order is not target-sorted


@pytest.mark.parametrize("reduce", ["mean", "sum", "max"])
@pytest.mark.parametrize("R", [0, 1, 65, 130, N])
def test_refs_match_float64_autograd(reduce, R):
    """wgrad_ref and the fused dgrad_ref against autograd of SAGEConv in
    float64: out = conv(h, ei); (relu(out) * keep * scale).backward(G), G zero
    on rows >= R.  NaNs sit wherever the contract says nothing is read."""
    K, Fo, scale = 24, 20, 2.0
    gen = torch.Generator().manual_seed(17 + R)
    h32 = lr.int_features(N, K, gen) if reduce == "max" else torch.randn(N, K, generator=gen)
    conv = pyg_ref.SAGEConv(K, Fo, aggr=reduce).double()
    h = h32.double().requires_grad_(True)
    out = conv(h, EI)
    keep = (torch.rand(N, Fo, generator=gen) < 0.6).double()
    act = out.relu() * keep
    G = torch.randn(N, Fo, generator=gen).double()
    G[R:] = 0
    (act * scale).backward(G)

    agg32 = lr.agg_of(h32, EI, N, reduce)
    rowptr = lr.rowptr_of(EI, N)
    edgeless = (rowptr[1:] == rowptr[:-1]).nonzero().flatten()
    if reduce != "max":  # (float64 aggregate for the float64 comparison)
        aggd = pyg_ref.propagate(h32.double(), EI, reduce)
    else:
        aggd = agg32
    dy = lr.poison_rows(torch.randn(N, Fo, generator=gen).double(), R)
    dy[:R] = G[:R]
    y = lr.poison_rows(act.detach(), R)
    dwl, dwr, db = lr.wgrad_ref(dy, y, scale, lr.poison_rows(h32.double(), R),
                                lr.poison_rows(aggd, R, edgeless), rowptr, R)
    torch.testing.assert_close(dwl, conv.lin_l.weight.grad, **F64)
    torch.testing.assert_close(dwr, conv.lin_r.weight.grad, **F64)
    torch.testing.assert_close(db, conv.lin_l.bias.grad, **F64)
    Rn = lr.rnext_of(EI, R)
    hp = lr.poison_rows(h32, Rn) if reduce == "max" else None
    ap = lr.poison_rows(agg32, R, edgeless) if reduce == "max" else None
    dh = lr.dgrad_fused_ref(dy, y, scale, conv.lin_l.weight.detach(), conv.lin_r.weight.detach(),
                            EI, N, R, reduce, hp, ap)
    assert torch.isfinite(dh).all()
    torch.testing.assert_close(dh, h.grad, **F64)
    assert not dh[Rn:].any()


def test_max_inputs_have_ties_and_zero_maxima():
    d = lr.gather_inputs(64, EI, N, "max")
    s, t = EI[0], EI[1]
    eq = (d["h"][s] == d["agg"][t]).float()
    ties = torch.zeros(N, 64).index_add_(0, t, eq)
    assert int((ties > 1).sum()) > 1000 and int(ties[lr.HUB_DST].max()) >= 10
    has = torch.bincount(t, minlength=N) > 0
    assert int((d["agg"][has] == 0).sum()) > 100


@pytest.mark.parametrize("reduce", ["mean", "sum", "max"])
@pytest.mark.parametrize("R", [0, 3, 65, N])
def test_gather_order_is_the_oracles_edge_order(reduce, R):
    """dgrad_gather_f32 == droot + oracle agg_bwd on the edges into rows < R,
    bitwise, and within fp32 rounding of dgrad_ref."""
    K = 36
    d = lr.gather_inputs(K, EI, N, reduce)
    rowptr = lr.rowptr_of(EI, N)
    edgeless = (rowptr[1:] == rowptr[:-1]).nonzero().flatten()
    dagg, droot = lr.poison_rows(d["dagg"], R), lr.poison_rows(d["droot"], R)
    agg = lr.poison_rows(d["agg"], R, edgeless) if reduce == "max" else None
    got = lr.dgrad_gather_f32(dagg, droot, EI, N, R, reduce, d["h"], agg)
    eir = lr.restrict(EI, R).numpy()
    want = c_agg.agg_bwd(d["dagg"][:R].numpy(), eir, N, reduce,
                         x=None if d["h"] is None else d["h"].numpy(),
                         agg=None if d["agg"] is None else d["agg"][:R].numpy())
    want[:R] = d["droot"][:R].numpy().astype(np.float32) + want[:R]
    assert got.dtype == np.float32 and np.array_equal(got, want)
    ref = lr.dgrad_ref(dagg, droot, EI, N, R, reduce, d["h"], agg)
    assert_wgrad(torch.from_numpy(got), ref, f"gather_f32 {reduce} R={R}", rel=1e-6)


def test_bound_refs():
    g = np.zeros((9, 3), np.float32)
    assert lr.row_extent_ref(g) == 0 and lr.row_extent_ref(g, 4) == 4
    g[2, 2] = -0.0
    assert lr.row_extent_ref(g) == 0
    g[5, 0] = np.nan
    assert lr.row_extent_ref(g) == 6 and lr.row_extent_ref(g, 8) == 8
    rowptr, col = lr.target_grouped(EI, N)
    for R in lr.R_ALL:
        rn, nnz = lr.prefix_stats_ref(rowptr.numpy(), col.numpy(), R)
        assert rn == lr.rnext_of(EI, R) and nnz == int((EI[1] < R).sum())
        assert lr.prefix_stats_ref(rowptr.numpy(), col.numpy(), R, N + 5)[0] == N + 5


# ---- the input self-check: plain fp32 torch at rel = 1e-6 on every GPU case
@pytest.mark.parametrize("Fo,K", lr.WGRAD_CASES + lr.WGRAD_BF16H_CASES)
@pytest.mark.parametrize("R", lr.R_FEW)
def test_wgrad_inputs_are_benign(Fo, K, R):
    d = lr.wgrad_inputs(Fo, K, EI, N)
    rowptr = lr.rowptr_of(EI, N)
    for y in (None, d["y"]):
        want = lr.wgrad_ref(d["dy"], y, 2.0, d["h"], d["agg"], rowptr, R)
        dz = d["dy"][:R] if y is None else torch.where(y[:R] > 0, d["dy"][:R] * 2.0, torch.zeros(()))
        a = d["agg"][:R] * (rowptr[1:R + 1] > rowptr[:R]).float()[:, None]
        got = (dz.t() @ a, dz.t() @ d["h"][:R], dz.sum(0))
        for name, g, w in zip(("dwl", "dwr", "db"), got, want):
            assert_wgrad(g, w, f"fp32 torch {name} Fo={Fo} K={K} R={R}", rel=1e-6)


def _dgrad_f32(dagg, droot, ei, R, reduce, h, agg):
    """Plain fp32 torch: index_add_ over the edges into rows < R."""
    keep = ei[1] < R
    s, t = ei[0][keep], ei[1][keep]
    g = dagg[t]
    if reduce == "mean":
        g = g / torch.bincount(ei[1], minlength=N).clamp(min=1).float()[t, None]
    elif reduce == "max":
        eq = (h[s] == agg[t]).float()
        ties = (agg == 0).float().index_add_(0, t, eq)
        g = eq * g / ties[t].clamp(min=1)
    dh = torch.zeros_like(dagg)
    dh[:R] = droot[:R]
    return dh.index_add_(0, s, g)


@pytest.mark.parametrize("reduce", ["mean", "sum", "max"])
@pytest.mark.parametrize("Fo,K", lr.DGRAD_FUSED_CASES)
def test_dgrad_fused_inputs_are_benign(Fo, K, reduce):
    d = lr.dgrad_inputs(Fo, K, EI, N, reduce)
    for R in lr.R_FEW:
        for y in (None, d["y"]):
            want = lr.dgrad_fused_ref(d["dy"], y, 2.0, d["wl"], d["wr"], EI, N, R, reduce,
                                      d["h"], d["agg"])
            dz = torch.zeros(N, Fo)
            dz[:R] = d["dy"][:R] if y is None else torch.where(y[:R] > 0, d["dy"][:R] * 2.0,
                                                              torch.zeros(()))
            got = _dgrad_f32(dz @ d["wl"], dz @ d["wr"], EI, R, reduce, d["h"], d["agg"])
            assert_wgrad(got, want, f"fp32 torch dgrad {reduce} Fo={Fo} K={K} R={R}", rel=1e-6)


@pytest.mark.parametrize("reduce", ["mean", "sum", "max"])
@pytest.mark.parametrize("K", lr.GATHER_K)
def test_gather_inputs_are_benign(K, reduce):
    d = lr.gather_inputs(K, EI, N, reduce)
    for R in lr.R_FEW:
        want = lr.dgrad_ref(d["dagg"], d["droot"], EI, N, R, reduce, d["h"], d["agg"])
        got = _dgrad_f32(d["dagg"], d["droot"], EI, R, reduce, d["h"], d["agg"])
        assert_wgrad(got, want, f"fp32 torch gather {reduce} K={K} R={R}", rel=1e-6)
