"""Every form of the per-layer forward's epilogue (bias, ReLU, hash dropout,
bf16 rounding) against an fp64 evaluation of the same layer with the host
replica of the mask (test_gpu_fused.dropout_keep).

The epilogue is a family of compile-time specialisations picked from
(dropout threshold, relu, out_bf16, column-slice parity, phase); each route
below is the smallest shape that reaches one group of them, and asserts its
routing through ngnn_sage_fwd_slice_cols / ngnn_sage_wide_preferred:

  A  row-tile kernel, one slice, W_l in LDS           K = 64 -> 48 / 40 / 7
  B  row-tile, even multi-slice, W_l streamed         K = 256 -> 200
  C  row-tile, ODD slices (48 columns)                K = 512 -> 176, 428 -> 100,
                                                      exact fp32: 640 -> 100
  D  no neighbour term: k_root forms 1 / 2 / 3 and the k_sage_rt fallback
                                                      K = 100 -> 256
  E  bf16 rows in, bf16 rows out                      K = 100 -> 64, 256 -> 256
  F  the 64-row kernel (packed weights)               K = 30 -> 40 / 600
  G  the wide path's three GEMM kernels               K = 62 / 30 -> 20 (+ exact)
  H  ngnn_gcn_agg_fwd                                 Fo = 48 / 7

One call per case through fused._fwd_raw / _gemm_layer (sage_layer_fwd's
padding and fallbacks would choose the route).  Per case: values at the
forward bar rtol = 1e-5, atol = 1e-5 max(1, scale) (dropout multiplies an
already-rounded value by the survivor scale); every dropped element exactly
+0.0; every kept element with |pre| > 10 atol nonzero; the columns past F_out,
the rows at or past *n_rows_dev and the guard rows behind the buffer keep a
sentinel bit pattern.  Each test prints its largest |got - ref| / (atol +
rtol |ref|)."""
import functools

import numpy as np
import pytest
import torch

from ngnn import _lib, fused
from ngnn.block import Block
from oracle import pyg_ref

from test_gpu_fused import OUT, dropout_keep, dropout_scale, dropout_thresh
from test_gpu_fwd2 import _block, _oracle, _params, _run_fwd2

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

SEED = 0x9E3779B97F4A7C15
SEED_A, SEED_B = 0xC2B2AE3D27D4EB4F, 0x165667B19E3779F9  # seed, *seed_dev: high words set
PS = (0.0, 0.5, 0.25, 0.3, 1.0 / 512, 1.0)
assert [dropout_thresh(p) for p in PS] == [0, 128, 64, 77, 1, 256]
RTOL = ATOL = 1e-5
SENT = -0x3C5A0FF3  # int32 bits 0xC3A5F00D: a finite float no layer here computes
SENT16 = -0x3C5B    # bf16 rows: 0xC3A5
N_EDGE = 37         # every target below it: the bound falls inside row tile 2
GUARD = 3           # sentinel rows behind the last output row
MEAN, EXACT = _lib.REDUCE["mean"], _lib.MATH_EXACT_F32


@functools.lru_cache(maxsize=None)
def _graph(N, src_max):
    """~400 random target-sorted edges into rows < 37 (rows 3, 17 and 30
    without any), sources below src_max."""
    g = torch.Generator().manual_seed(N * 1000 + src_max)
    dst = torch.randint(0, N_EDGE, (420,), generator=g)
    dst[:4] = N_EDGE - 1  # the last edge row is never empty
    dst = dst[(dst != 3) & (dst != 17) & (dst != 30)]
    dst = torch.sort(dst, stable=True).values
    src = torch.randint(0, src_max, (dst.numel(),), generator=g)
    ei = torch.stack([src, dst])
    return ei, Block(ei.to(DEV), N)


def _agg64(x, ei, N, reduce):
    """[deg > 0] agg(x) in float64 (empty rows: 0)."""
    src, dst = ei[0], ei[1]
    K = x.size(1)
    if reduce == "max":
        out = torch.zeros(N, K, dtype=torch.float64)
        return out.scatter_reduce(0, dst[:, None].expand(-1, K), x[src], "amax", include_self=False)
    out = torch.zeros(N, K, dtype=torch.float64).index_add_(0, dst, x[src])
    if reduce == "mean":
        out /= torch.bincount(dst, minlength=N).clamp(min=1)[:, None]
    return out


@functools.lru_cache(maxsize=None)
def _layer(K, Fo, N, bf16=False):
    """x ~ N(0, 1) and default-initialised SAGEConv weights (bf16: rounded to
    bf16-exact values), on the host (fp32) and the device."""
    g = torch.Generator().manual_seed(K * 131 + Fo)
    x = torch.randn(N, K, generator=g)
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(K * 7 + Fo)
        conv = pyg_ref.SAGEConv(K, Fo)
    wl, wr, b = conv.lin_l.weight.detach(), conv.lin_r.weight.detach(), conv.lin_l.bias.detach()
    if bf16:
        x, wl, wr, b = (t.bfloat16().float() for t in (x, wl, wr, b))
    host = dict(x=x, wl=wl, wr=wr, b=b)
    dev = {k: v.to(DEV) for k, v in host.items()}
    if bf16:
        dev["x"] = dev["x"].bfloat16()
    return host, dev


@functools.lru_cache(maxsize=None)
def _pre64(K, Fo, N, reduce, src_max, root=True, nbr=True, bias=True, bf16=False):
    """b + x W_r^T + [deg > 0] agg(x) W_l^T in float64 from the fp32 inputs;
    computed once per layer and shared (never modified)."""
    h, _ = _layer(K, Fo, N, bf16)
    x = h["x"].double()
    pre = torch.zeros(N, Fo, dtype=torch.float64)
    if bias:
        pre += h["b"].double()
    if root:
        pre += x @ h["wr"].double().T
    if nbr:
        pre += _agg64(x, _graph(N, src_max)[0], N, reduce) @ h["wl"].double().T
    return pre


def _buffer(N, Fo, ldo, bf16=False):
    """A sentinel-filled [N + GUARD, ldo] buffer and its [N, Fo] output view."""
    buf = torch.full((N + GUARD, ldo), SENT16 if bf16 else SENT,
                     dtype=torch.int16 if bf16 else torch.int32, device=DEV)
    return buf, buf.view(torch.bfloat16 if bf16 else torch.float32)[:N, :Fo]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _check(buf, pre, relu, p, seed, Fo, n_live=None, what=""):
    """The assertions of one case; returns the largest error ratio."""
    N = pre.size(0)
    n_live = N if n_live is None else n_live
    raw = buf.cpu()
    got = raw.view(torch.float32)[:n_live, :Fo]
    sent = raw.clone()
    sent[:n_live, :Fo] = SENT
    assert bool((sent == SENT).all()), f"{what}: a store outside out[:{n_live}, :{Fo}]"
    pre = pre[:n_live]
    scale = float(np.float32(dropout_scale(p)))
    atol = ATOL * max(1.0, scale)
    if dropout_thresh(p) == 256:
        assert bool((_bits(got) == 0).all()), f"{what}: p = 1 is all +0.0"
        return 0.0
    keep = dropout_keep(seed, N, Fo, p)[:n_live]
    act = pre.clamp(min=0.0) if relu else pre
    ref = act * keep * scale
    ratio = float(((got.double() - ref).abs() / (atol + RTOL * ref.abs())).max())
    assert not bool(torch.isnan(got).any()), what
    assert ratio <= 1.0, f"{what}: |got - ref| / (atol + rtol |ref|) = {ratio:.3f}"
    assert bool((_bits(got)[~keep] == 0).all()), f"{what}: a dropped element is not +0.0"
    must = keep & (pre.abs() > 10 * atol) & ((pre > 0) if relu else torch.ones_like(keep))
    assert bool((got[must] != 0).all()), f"{what}: a kept element is zero"
    return ratio


def _ws(K, Fo, N):
    return fused._workspace(DEV, "sage_fwd", _lib.load().ngnn_sage_fwd_raw_workspace_bytes(K, Fo, N), zero=True)


def _raw(d, blk, reduce, out, relu, p, seed, *, flags=0, root=True, nbr=True, bias=True, n_rows_dev=None,
         seed_dev=None):
    K, Fo, N = d["x"].size(1), d["wr"].size(0), d["x"].size(0)
    rc = fused._fwd_raw(d["x"], n_rows_dev=n_rows_dev, n_edge_rows=N_EDGE, rowptr=blk.rowptr, col=blk.col,
                        reduce=reduce, flags=flags, wl=d["wl"] if nbr else None, wr=d["wr"] if root else None,
                        bias=d["b"] if bias else None, out=out, relu=relu, p_drop=p, seed=seed,
                        seed_dev=seed_dev, ws=_ws(K, Fo, N))
    assert rc == _lib.OK, f"ngnn_sage_fwd_raw: rc = {rc}"


def _ldos(Fo):
    return (Fo + 4, Fo + 1)  # vector stores where F_out allows them; scalar stores


def _layer_ref(K, Fo, N, reduce, **kw):
    """ref(src_max, bias) of a SAGE layer: its shared fp64 pre-activations."""
    return lambda src_max=N, bias=True: _pre64(K, Fo, N, reduce, src_max, bias=bias, **kw)


def _sweep(route, tag, Fo, N, relu, run, ref):
    """The epilogue matrix of one (layer, reduce, relu): every p, both row
    strides.  run(out, p, seed, **variant) makes the one call; ref(src_max,
    bias) gives the fp64 pre-activations."""
    pre, worst = ref(), 0.0
    for p in PS:
        for ldo in _ldos(Fo):
            buf, out = _buffer(N, Fo, ldo)
            run(out, p, SEED)
            worst = max(worst, _check(buf, pre, relu, p, SEED, Fo,
                                      what=f"{route} {tag} relu={relu} p={p:g} ldo={ldo}"))
    print(f"route {route} {tag} relu={relu}: worst ratio {worst:.3f}")


def _variants(route, tag, Fo, N, nrd, run, ref):
    """One set per route (mean, ReLU, bit and byte mode): a device row bound
    that is no multiple of 16 (the edges' sources below it), seed ^ *seed_dev
    with nonzero high words, and no bias."""
    nrd_t = torch.tensor([nrd], dtype=torch.int32, device=DEV)
    sd_t = torch.tensor([SEED_B], dtype=torch.int64, device=DEV)  # (the device word: SEED_B < 2^63)
    assert nrd % 16 and SEED_A >> 32 and SEED_B >> 32 and (SEED_A ^ SEED_B) >> 32
    worst = 0.0
    for p in (0.5, 0.3):
        for ldo in _ldos(Fo):
            what = f"{route} {tag} p={p:g} ldo={ldo}"
            buf, out = _buffer(N, Fo, ldo)
            run(out, p, SEED, n_rows_dev=nrd_t, src_max=nrd)
            worst = max(worst, _check(buf, ref(src_max=nrd), True, p, SEED, Fo, n_live=nrd,
                                      what=what + " n_rows_dev"))
            buf, out = _buffer(N, Fo, ldo)
            run(out, p, SEED_A, seed_dev=sd_t)
            worst = max(worst, _check(buf, ref(), True, p, SEED_A ^ SEED_B, Fo, what=what + " seed_dev"))
            buf, out = _buffer(N, Fo, ldo)
            run(out, p, SEED, bias=False)
            worst = max(worst, _check(buf, ref(bias=False), True, p, SEED, Fo, what=what + " no bias"))
    print(f"route {route} {tag} variants: worst ratio {worst:.3f}")


def _raw_runner(K, Fo, N, reduce, relu, flags=0, root=True, nbr=True, bf16=False):
    _, d = _layer(K, Fo, N, bf16)

    def run(out, p, seed, src_max=N, **kw):
        _raw(d, _graph(N, src_max)[1], reduce, out, relu, p, seed, flags=flags, root=root, nbr=nbr, **kw)
    return run


def _slice(K, Fo, flags=0):
    return _lib.load().ngnn_sage_fwd_slice_cols(K, Fo, MEAN | flags)


# ---- routes A, B, C: the row-tile kernel (phase 1 on tiles 0..2, phase 2 past row 37)

RT_SHAPES = {
    "A": [(64, 48), (64, 40), (64, 7)],
    "B": [(256, 200)],
    "C": [(512, 176), (428, 100)],
}


def _assert_rt_route(route, K, Fo, flags=0):
    s = _slice(K, Fo, flags)
    assert s > 0 and not _lib.load().ngnn_sage_wide_preferred(K, Fo, int(bool(flags & EXACT)))
    if route == "A":
        assert s >= Fo  # one slice
    elif route == "B":
        assert s == 96 and (Fo - 1) // s == 2 and Fo - 2 * s == 8  # col_base 0, 96, 192; 8 columns last
    else:
        assert s == 48 and Fo > s  # col_base 48 (and 144): odd 16-column tiles
    return s


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("route,K,Fo,reduce", [
    (r, K, Fo, red) for r, shapes in RT_SHAPES.items() for K, Fo in shapes
    for red in (("mean", "max", "sum") if r in "AB" else ("mean",))])
def test_rowtile_forms(route, K, Fo, reduce, relu):
    _assert_rt_route(route, K, Fo)
    _sweep(route, f"K={K} Fo={Fo} {reduce}", Fo, 83, relu, _raw_runner(K, Fo, 83, reduce, relu),
           _layer_ref(K, Fo, 83, reduce))


@pytest.mark.parametrize("relu", [False, True])
def test_rowtile_odd_slices_exact_f32(relu):
    K, Fo = 640, 100
    _assert_rt_route("C", K, Fo, EXACT)
    with fused.exact_f32():
        _sweep("C", f"K={K} Fo={Fo} exact", Fo, 83, relu, _raw_runner(K, Fo, 83, "mean", relu),
               _layer_ref(K, Fo, 83, "mean"))


@pytest.mark.parametrize("route,K,Fo", [("A", 64, 48), ("A", 64, 7), ("B", 256, 200), ("C", 512, 176),
                                        ("C", 428, 100)])
def test_rowtile_variants(route, K, Fo):
    _assert_rt_route(route, K, Fo)
    _variants(route, f"K={K} Fo={Fo}", Fo, 83, 70, _raw_runner(K, Fo, 83, "mean", True),
              _layer_ref(K, Fo, 83, "mean"))


# ---- route D: no neighbour term -- k_root's forms 1 (bit mode + ReLU), 2 (ReLU),
# 3 (plain) with vector stores; every other (p, relu, stride) on k_sage_rt

@pytest.mark.parametrize("relu", [False, True])
def test_root_only_forms(relu):
    K, Fo = 100, 256
    assert _slice(K, Fo) == 256
    _sweep("D", f"K={K} Fo={Fo}", Fo, 83, relu, _raw_runner(K, Fo, 83, "mean", relu, nbr=False),
           _layer_ref(K, Fo, 83, "mean", nbr=False))


def test_root_only_variants():
    K, Fo = 100, 256
    _variants("D", f"K={K} Fo={Fo}", Fo, 83, 70, _raw_runner(K, Fo, 83, "mean", True, nbr=False),
              _layer_ref(K, Fo, 83, "mean", nbr=False))


# ---- route E: bf16 rows in (NGNN_X_BF16 | NGNN_W_BF16) and out (NGNN_OUT_BF16)

@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("K,Fo", [(100, 64), (256, 256)])
def test_bf16_rows_forms(K, Fo, relu):
    """The fp32 rows of the bf16-input call against fp64; the bf16 rows of the
    same call with NGNN_OUT_BF16 bitwise their round-to-nearest-even."""
    N, fl = 83, _lib.X_BF16 | _lib.W_BF16
    assert _slice(K, Fo, fl) == 256
    _, d = _layer(K, Fo, N, True)
    blk = _graph(N, N)[1]
    pre = _pre64(K, Fo, N, "mean", N, bf16=True)
    worst = 0.0
    for p in PS:
        rows32 = None
        for ldo in _ldos(Fo):
            tag = f"E K={K} Fo={Fo} relu={relu} p={p:g} ldo={ldo}"
            buf, out = _buffer(N, Fo, ldo)
            _raw(d, blk, "mean", out, relu, p, SEED, flags=fl)
            worst = max(worst, _check(buf, pre, relu, p, SEED, Fo, what=tag))
            rows32 = out.cpu() if rows32 is None else rows32
            assert torch.equal(_bits(out.cpu()), _bits(rows32)), tag  # the stride changes no value
        # (bf16 rows: 8-B stores of whole tiles, a row stride of a multiple of 4)
        buf, out = _buffer(N, Fo, Fo + 4, bf16=True)
        _raw(d, blk, "mean", out, relu, p, SEED, flags=fl | _lib.OUT_BF16)
        raw = buf.cpu()
        assert torch.equal(raw[:N, :Fo], rows32.bfloat16().view(torch.int16)), f"E K={K} Fo={Fo} p={p:g}: bf16 rows"
        raw[:N, :Fo] = SENT16
        assert bool((raw == SENT16).all())
    print(f"route E K={K} Fo={Fo} relu={relu}: worst ratio {worst:.3f}")


def test_bf16_rows_variants():
    K, Fo, fl = 100, 64, _lib.X_BF16 | _lib.W_BF16
    _variants("E", f"K={K} Fo={Fo}", Fo, 83, 70, _raw_runner(K, Fo, 83, "mean", True, flags=fl, bf16=True),
              _layer_ref(K, Fo, 83, "mean", bf16=True))


# ---- route F: the 64-row kernel (ngnn_sage_fwd, packed weights; K % 4 != 0
# keeps the call off the row-tile kernel)

def _gemm_runner(K, Fo, N, reduce, relu):
    _, d = _layer(K, Fo, N)
    pl, pr = fused.pack_weight(d["wl"]), fused.pack_weight(d["wr"])

    def run(out, p, seed, src_max=N, bias=True, n_rows_dev=None, seed_dev=None):
        fused._gemm_layer(d["x"], K, N, _graph(N, src_max)[1], reduce, pl, pr, d["b"] if bias else None, Fo, out,
                          relu, p, seed, n_rows_dev=n_rows_dev, seed_dev=seed_dev)
    return run


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("reduce", ["mean", "max", "sum"])
@pytest.mark.parametrize("K,Fo", [(30, 40), (30, 600)])
def test_gemm64_forms(K, Fo, reduce, relu):
    assert K % 4 and _slice(K, Fo) == 0
    _sweep("F", f"K={K} Fo={Fo} {reduce}", Fo, 150, relu, _gemm_runner(K, Fo, 150, reduce, relu),
           _layer_ref(K, Fo, 150, reduce))


def test_gemm64_variants():
    _variants("F", "K=30 Fo=600", 600, 150, 101, _gemm_runner(30, 600, 150, "mean", True),
              _layer_ref(30, 600, 150, "mean"))


# ---- route G: the wide path -- k_wide_h2 (an even number of 32-column
# k-stages), k_wide_x3 (odd), k_wide_gemm (exact fp32)

@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("K,exact", [(62, False), (30, False), (30, True)])
def test_wide_forms(K, exact, relu):
    Fo, N = 20, 150
    assert _lib.load().ngnn_sage_wide_preferred(K, Fo, int(exact)) == 1
    assert _slice(K, Fo, EXACT if exact else 0) == 0
    assert (-(-K // 32)) % 2 == (0 if K == 62 else 1)
    with fused.exact_f32(exact):
        _sweep("G", f"K={K} Fo={Fo} exact={exact}", Fo, N, relu, _raw_runner(K, Fo, N, "mean", relu),
               _layer_ref(K, Fo, N, "mean"))


@pytest.mark.parametrize("K,exact", [(62, False), (30, False), (30, True)])
def test_wide_variants(K, exact):
    with fused.exact_f32(exact):
        _variants("G", f"K={K} Fo=20 exact={exact}", 20, 150, 101, _raw_runner(K, 20, 150, "mean", True),
                  _layer_ref(K, 20, 150, "mean"))


# ---- route H: ngnn_gcn_agg_fwd on a random z: act(sum_edges z + b)

@functools.lru_cache(maxsize=None)
def _gcn_case(Fo, N, src_max, bias=True):
    ldz = -(-Fo // 16) * 16
    g = torch.Generator().manual_seed(Fo)
    z = torch.randn(N, ldz, generator=g)
    b = torch.rand(Fo, generator=g) - 0.5
    ei = _graph(N, src_max)[0]
    pre = torch.zeros(N, Fo, dtype=torch.float64).index_add_(0, ei[1], z[:, :Fo].double()[ei[0]])
    if bias:
        pre += b.double()
    return z.to(DEV), b.to(DEV), pre


def _gcn_run(Fo, N, relu):
    def run(out, p, seed, src_max=N, bias=True, n_rows_dev=None, seed_dev=None):
        z, b, _ = _gcn_case(Fo, N, src_max)
        blk = _graph(N, src_max)[1]
        _lib.check(_lib.load().ngnn_gcn_agg_fwd(
            _lib.ptr(z), z.stride(0), Fo, _lib.ptr(blk.rowptr), _lib.ptr(blk.col), N, _lib.ptr(n_rows_dev),
            _lib.ptr(b) if bias else None, int(relu), float(p), seed, _lib.ptr(seed_dev), _lib.ptr(out),
            out.stride(0), _lib.stream_handle(DEV)), "ngnn_gcn_agg_fwd")
    return run


def _gcn_ref(Fo, N):
    return lambda src_max=N, bias=True: _gcn_case(Fo, N, src_max, bias)[2]


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("Fo", [48, 7])
def test_gcn_agg_forms(Fo, relu):
    _sweep("H", f"Fo={Fo}", Fo, 83, relu, _gcn_run(Fo, 83, relu), _gcn_ref(Fo, 83))


def test_gcn_agg_variants():
    _variants("H", "Fo=48", 48, 83, 70, _gcn_run(48, 83, True), _gcn_ref(48, 83))


# ---- non-finite pre-activations (route A): a NaN row and a +inf element

@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("p", [0.0, 0.5, 0.25])
def test_non_finite_rows(relu, p):
    """Row 50 of x all NaN (no in-edge reads it), x[60, 5] = +inf.  A dropped
    element is +0.0 whatever it held.  Kept elements of the NaN row: NaN --
    but in bit mode with ReLU the integer max turns a negative-signed NaN into
    +0.0 (include/ngnn.h, ngnn_sage_fwd), so there NaN or +0.0.  The +inf row
    (the unguarded split of x turns an infinite element into NaN,
    ngnn_sage_rt_kern.h split3): every kept element non-finite or, under ReLU,
    +0.0, never -inf; every other row as without the two."""
    K, Fo, N = 64, 48, 83
    _, d = _layer(K, Fo, N)
    ei, blk = _graph(N, 45)  # (sources below 45: rows 50 and 60 feed no aggregate)
    x = d["x"].clone()
    x[50] = float("nan")
    x[60, 5] = float("inf")
    buf, out = _buffer(N, Fo, Fo + 4)
    _raw(dict(d, x=x), blk, "mean", out, relu, p, SEED)
    got = out.cpu()
    keep = dropout_keep(SEED, N, Fo, p)
    assert bool((_bits(got)[~keep] == 0).all())
    nan_row, k50 = got[50], keep[50]
    if relu and dropout_thresh(p) == 128:
        assert bool((torch.isnan(nan_row[k50]) | (_bits(nan_row[k50]) == 0)).all())
    else:
        assert bool(torch.isnan(nan_row[k50]).all())
    inf_row = got[60][keep[60]]
    if relu:
        assert bool((~torch.isfinite(inf_row) | (_bits(inf_row) == 0)).all())
        assert not bool(torch.isneginf(inf_row).any())
    else:
        assert bool((~torch.isfinite(inf_row)).all())
    rest = torch.ones(N, dtype=torch.bool)
    rest[[50, 60]] = False
    pre = _pre64(K, Fo, N, "mean", 45)
    ref = (pre.clamp(min=0.0) if relu else pre) * keep * float(np.float32(dropout_scale(p)))
    atol = ATOL * max(1.0, dropout_scale(p))
    torch.testing.assert_close(got[rest].double(), ref[rest], rtol=RTOL, atol=atol)


# ---- the two-layer forward at the thresholds its tests do not reach

@pytest.mark.parametrize("p", [1.0 / 512, 1.0])
def test_fwd2_extreme_thresholds(p):
    """thresh = 1 (byte mode, scale 256 / 255) and thresh = 256 (h == 0: the
    per-row fp16 scaling of an all-zero h; the logits are b1 on every row)."""
    K0, H, F1, N, n_act = 100, 256, 47, 83, N_EDGE
    ei, blk = _block(83, N, n_act, zero_rows=(3, 17))
    x = torch.randn(N, K0, generator=torch.Generator().manual_seed(83))
    ref = _params(K0, H, F1, 5)
    h, out, _ = _run_fwd2(x, blk, ref, "mean", p, SEED)
    with torch.no_grad():
        h_r, out_r = _oracle(x, ei, ref, "mean", p, SEED, N, H)
    assert not bool(torch.isnan(h).any()) and not bool(torch.isnan(out).any())
    torch.testing.assert_close(h, h_r, **OUT)
    torch.testing.assert_close(out, out_r, **OUT)
    if p == 1.0:
        assert bool((_bits(h) == 0).all())
        assert torch.equal(out, ref.convs[1].lin_l.bias.detach().expand(N, F1))
