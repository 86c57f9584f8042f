"""The per-layer backward restated in float64 -- the reference the kernels of
csrc/ngnn_sage_bwd.hip (and the two bound kernels of csrc/ngnn_sage.hip) are
measured against -- plus the hand-built block and the case inputs that
tests/test_layer_bwd_cpu.py and tests/test_layer_bwd_gpu.py share.  Plain
torch / numpy on the CPU; nothing of the library is imported.

Contract (include/ngnn.h): R bounds the rows of the output gradient, so
nothing at or past row R of dy / y / h / agg / dagg / droot is read, and the
saved aggregate of a row without in-edges is never read (it was never
written).  Every function below slices or selects BEFORE it converts or
multiplies, so NaNs parked in those places cannot enter a result.
"""
import numpy as np
import torch

N_NODES = 600
HUB_DST, HUB_SRC, HUB_DEG = 5, 7, 150
R_ALL = (0, 1, 3, 63, 64, 65, 130, N_NODES)
R_FEW = (65, N_NODES)


# ----------------------------------------------------------------- the block
def make_block(shuffle=True):
    """edge_index [2, E] int64 (row 0 sources, row 1 targets), N = 600,
    E ~ 4000, with everything the bounded backward can trip over:

    * target rows 20..62 (43 rows, below every R >= 63), 300 and 599 have no
      in-edges;
    * hub target 5: in-degree 150 (sources 300..449); hub source 7:
      out-degree 150 (targets 0..19 without 5, and 63..193);
    * sources 450..469 and 590..599 have no out-edges;
    * edges into targets < 200 come from sources < 500, so for R <= 130 the
      input-gradient bound R' lies in (R, N): rows past it exist and sources
      at or past R feed rows below R; targets at or past R keep in-edges;
    * 40 duplicated edges, 30 self-loops; the edge order is shuffled.
    """
    N = N_NODES
    g = torch.Generator().manual_seed(20241019)
    edgeless = set(range(20, 63)) | {300, 599}
    no_out = set(range(450, 470)) | set(range(590, 600))
    dst_ok = torch.tensor([d for d in range(N) if d not in edgeless and d != HUB_DST])
    lo_src = torch.tensor([s for s in range(500) if s not in no_out and s != HUB_SRC])
    all_src = torch.tensor([s for s in range(N) if s not in no_out and s != HUB_SRC])
    n_rand = 3600
    dst = dst_ok[torch.randint(0, dst_ok.numel(), (n_rand,), generator=g)]
    pick_lo = lo_src[torch.randint(0, lo_src.numel(), (n_rand,), generator=g)]
    pick_all = all_src[torch.randint(0, all_src.numel(), (n_rand,), generator=g)]
    src = torch.where(dst < 200, pick_lo, pick_all)
    rand = torch.stack([src, dst])
    dup = rand[:, torch.randperm(n_rand, generator=g)[:40]]
    loops = dst_ok[(dst_ok != HUB_SRC) & ~torch.isin(dst_ok, torch.tensor(sorted(no_out)))]
    loops = loops[torch.randperm(loops.numel(), generator=g)[:30]]
    hub_in = torch.stack([torch.arange(300, 300 + HUB_DEG), torch.full((HUB_DEG,), HUB_DST)])
    hub_targets = torch.tensor([d for d in range(20) if d != HUB_DST] + list(range(63, 194)))
    assert hub_targets.numel() == HUB_DEG
    hub_out = torch.stack([torch.full((HUB_DEG,), HUB_SRC), hub_targets])
    ei = torch.cat([rand, dup, torch.stack([loops, loops]), hub_in, hub_out], dim=1).long()
    if shuffle:
        ei = ei[:, torch.randperm(ei.size(1), generator=g)]
    return ei.contiguous()


def rowptr_of(ei, N):
    """int64 [N + 1] target-grouped row pointer of edge_index."""
    deg = torch.bincount(ei[1], minlength=N)
    return torch.cat([torch.zeros(1, dtype=torch.long), deg.cumsum(0)])


def restrict(ei, R):
    """The edges into rows < R, in their original order."""
    return ei[:, ei[1] < R]


def rnext_of(ei, R):
    """R' = max(R, 1 + max source of the edges into rows < R)."""
    s = ei[0][ei[1] < R]
    return max(R, int(s.max()) + 1 if s.numel() else 0)


# ------------------------------------------------------------ float64 rules
def masked_dz(dy, y, yscale, R):
    """dz = dy[:R] (* [y[:R] > 0] * yscale with a mask), float64."""
    dz = dy[:R].double()
    if y is not None:
        dz = torch.where(y[:R].double() > 0, dz * float(yscale), torch.zeros_like(dz))
    return dz


def wgrad_ref(dy, y, yscale, h, agg, rowptr, R, h_idx=None):
    """(dW_l, dW_r, db) in float64: dW_r = dz^T h[:R], dW_l = dz^T (agg[:R]
    where the row has in-edges, else 0), db = sum dz.  h_idx: row r of the
    layer input is row h_idx[r] of the table h."""
    dz = masked_dz(dy, y, yscale, R)
    hh = (h[h_idx[:R]] if h_idx is not None else h[:R]).double()
    deg = (rowptr[1:R + 1] - rowptr[:R]).reshape(-1, 1)
    a = agg[:R]
    a = torch.where(deg > 0, a, torch.zeros_like(a)).double()
    return dz.t() @ a, dz.t() @ hh, dz.sum(0)


def dgrad_ref(dagg, droot, ei, N, R, reduce, h=None, agg=None):
    """dh [N, K] float64: dh[j] = [j < R] droot[j] + sum over edges j -> d,
    d < R, of f(dagg[d]); f = identity (sum), / max(deg(d), 1) (mean), or the
    amax rule [h[j] == agg[d]] dagg[d] / ([agg[d] == 0] + ties(d)) with the
    equalities taken on the given (fp32) values."""
    K = dagg.shape[1]
    keep = ei[1] < R
    s, d = ei[0][keep], ei[1][keep]
    g = dagg[:R].double()[d]
    if reduce == "mean":
        deg = torch.bincount(ei[1], minlength=N).clamp(min=1).double()
        g = g / deg[d, None]
    elif reduce == "max":
        eq = (h[s] == agg[:R][d]).double()
        ties = (agg[:R] == 0).double().index_add_(0, d, eq)
        g = eq * g / ties[d].clamp(min=1)  # (a clamped count belongs to eq == 0 only)
    elif reduce not in ("sum", "add"):
        raise ValueError(reduce)
    dh = torch.zeros(N, K, dtype=torch.float64)
    dh[:R] = droot[:R].double()
    return dh.index_add_(0, s, g)


def dgrad_fused_ref(dy, y, yscale, wl, wr, ei, N, R, reduce, h=None, agg=None):
    """The fused form: droot = dz W_r and dagg = dz W_l in float64 first."""
    dz = masked_dz(dy, y, yscale, R)
    K = wl.shape[1]
    droot = torch.zeros(N, K, dtype=torch.float64)
    dagg = torch.zeros(N, K, dtype=torch.float64)
    droot[:R], dagg[:R] = dz @ wr.double(), dz @ wl.double()
    return dgrad_ref(dagg, droot, ei, N, R, reduce, h, agg)


def dgrad_gather_f32(dagg, droot, ei, N, R, reduce, h=None, agg=None):
    """The same sum in fp32 in the order of the deterministic gather: per
    source row sequentially over its edges in original edge order (the stable
    source-grouped CSR), from zero, then droot + acc on rows < R."""
    f32 = np.float32
    dagg_n = np.asarray(dagg[:R], dtype=f32)
    K = dagg.shape[1]
    src, dst = ei[0].numpy(), ei[1].numpy()
    deg = np.bincount(dst, minlength=N)
    g = dagg_n
    if reduce == "max":
        hn, an = np.asarray(h, dtype=f32), np.asarray(agg[:R], dtype=f32)
        ties = (an == 0).astype(f32)
        for s, d in zip(src, dst):
            if d < R:
                ties[d] += (hn[s] == an[d]).astype(f32)
        with np.errstate(all="ignore"):
            g = dagg_n / ties
    acc = np.zeros((N, K), f32)
    for s, d in zip(src, dst):
        if d >= R:
            continue
        if reduce == "mean":
            acc[s] += g[d] / f32(max(deg[d], 1))
        elif reduce == "max":
            acc[s] += (hn[s] == an[d]).astype(f32) * g[d]
        else:
            acc[s] += g[d]
    acc[:R] = np.asarray(droot[:R], dtype=f32) + acc[:R]
    return acc


# ------------------------------------------------------- the bound contracts
def row_extent_ref(g, out0=0):
    """max(out0, 1 + last row of g holding a nonzero or a NaN); -0.0 is zero."""
    g = np.asarray(g)
    rows = np.flatnonzero((g != 0).reshape(g.shape[0], -1).any(axis=1))
    return max(int(out0), int(rows[-1]) + 1 if rows.size else 0)


def prefix_stats_ref(rowptr, col, R, r_next0=0):
    """(max(r_next0, R, 1 + max col[0 .. rowptr[R])), rowptr[R])."""
    nnz = int(rowptr[R])
    m = int(np.asarray(col[:nnz]).max()) + 1 if nnz else 0
    return max(int(r_next0), int(R), m), nnz


# ------------------------------------------------------------ the case inputs
WGRAD_CASES = [(7, 24), (16, 100), (20, 33), (47, 64), (48, 256), (129, 52), (64, 64), (52, 100),
               (68, 132), (256, 100), (64, 131)]
WGRAD_BF16H_CASES = [(64, 128), (128, 64), (48, 64), (16, 64)]
DGRAD_FUSED_CASES = [(64, 64), (32, 100), (10, 48), (33, 35), (512, 40), (64, 65), (40, 1)]
GATHER_K = [1, 3, 4, 7, 13, 20, 64, 100, 132, 260]


def target_grouped(ei, N):
    """(rowptr int64 [N + 1], col int64 [E]) grouped by target, stable."""
    order = torch.argsort(ei[1], stable=True)
    return rowptr_of(ei, N), ei[0][order]


def int_features(N, K, gen):
    """Small-integer rows for max: ties and zero maxima are data."""
    return torch.randn(N, K, generator=gen).relu().round()


def agg_of(h, ei, N, reduce):
    """The saved aggregate in fp32 (float64 sums rounded once; max exact)."""
    s, d = ei[0], ei[1]
    K = h.shape[1]
    if reduce == "max":
        from oracle import c_agg  # (the oracle's plain-C aggregation: test infrastructure)
        return torch.from_numpy(c_agg.agg_fwd(h.numpy(), ei.numpy(), N, "max"))
    out = torch.zeros(N, K, dtype=torch.float64).index_add_(0, d, h[s].double())
    if reduce == "mean":
        out = out / torch.bincount(d, minlength=N).clamp(min=1).double()[:, None]
    return out.float()


def wgrad_inputs(Fo, K, ei, N, table_rows=0):
    """O(1) normal dy, y (mask), h and the mean aggregate of h over the block;
    table_rows > 0: h is a table of that many rows and h_idx (with repeats)
    picks the layer input from it."""
    gen = torch.Generator().manual_seed(1000 * Fo + K)
    dy = torch.randn(N, Fo, generator=gen)
    y = torch.randn(N, Fo, generator=gen)
    h = torch.randn(max(N, table_rows), K, generator=gen)
    h_idx = None
    if table_rows:
        h_idx = torch.randint(0, table_rows // 2, (N,), generator=gen) * 2  # repeats, gaps
    hin = h[h_idx] if table_rows else h
    return dict(dy=dy, y=y, h=h, h_idx=h_idx, agg=agg_of(hin, ei, N, "mean"))


def dgrad_inputs(Fo, K, ei, N, reduce):
    """dy, y, weights (scaled by 0.2), and for max the integer layer input
    with its exact fp32 maximum."""
    gen = torch.Generator().manual_seed(7000 * Fo + K)
    d = dict(dy=torch.randn(N, Fo, generator=gen), y=torch.randn(N, Fo, generator=gen),
             wl=torch.randn(Fo, K, generator=gen) * 0.2, wr=torch.randn(Fo, K, generator=gen) * 0.2,
             h=None, agg=None)
    if reduce == "max":
        d["h"] = int_features(N, K, gen)
        d["agg"] = agg_of(d["h"], ei, N, "max")
    return d


def gather_inputs(K, ei, N, reduce):
    gen = torch.Generator().manual_seed(31 * K + 5)
    d = dict(dagg=torch.randn(N, K, generator=gen), droot=torch.randn(N, K, generator=gen),
             h=None, agg=None)
    if reduce == "max":
        d["h"] = int_features(N, K, gen)
        d["agg"] = agg_of(d["h"], ei, N, "max")
    return d


def poison_rows(t, R, extra_rows=None):
    """A copy of t with NaN in rows >= R (and in extra_rows)."""
    t = t.clone()
    t[R:] = float("nan")
    if extra_rows is not None:
        t[extra_rows] = float("nan")
    return t
