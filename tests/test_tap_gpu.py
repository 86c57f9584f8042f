"""The two hidden-state tap kernels alone (csrc/ngnn_tap.hip).

ngnn_dropout_rows against the host replica of the hash mask
(test_gpu_fused.dropout_keep): every kept element is fl32(h * scale) bit for
bit, every dropped one +0.0, and nothing outside out[:bound, :F] is written;
then against the fused epilogue itself: the layer with (relu = 1, p_drop = 0)
followed by ngnn_dropout_rows equals, with torch.equal, the same layer call
with p_drop -- on the row-tile kernel's one-slice, even multi-slice and odd
48-column-slice routes (the shapes of test_gpu_epilogue_forms.py).

ngnn_tap_grad against fp64 on the host.  Its two products and one sum are
each correctly rounded fp32 operations (the library is built with
-ffp-contract=off), so:
  * where one term is zero the result is the other term exactly;
  * with an exact product (yscale a power of two: 2 for p = 0.5, 4 for
    p = 0.75) the only rounding is the sum's, at most half an ulp of a sum
    below twice the larger term: within 1 ulp of the larger term of fp64;
  * with an inexact yscale (256 / 179, p = 0.3) the result is asserted
    bitwise against the same two fp32 operations on the host.
"""
import numpy as np
import pytest
import torch

from ngnn import _lib

from test_gpu_epilogue_forms import (N_EDGE, SEED, SEED_A, SEED_B, _assert_rt_route, _bits, _buffer, _graph, _layer,
                                     _raw)
from test_gpu_fused import dropout_keep, dropout_scale, dropout_thresh

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

FS = (1, 3, 4, 31, 32, 33, 40, 100, 256)
ROWS = (1, 17, 300)
PS = (0.0, 0.5, 0.25, 0.3, 1.0 / 512, 1.0)
SENT = -0x3C5A0FF3  # int32 bits 0xC3A5F00D: a finite float nothing here computes
GUARD = 3


def _lds(F):
    """(input stride, output stride): dense; 16-B rows with spare columns;
    rows off 16-B alignment (an odd stride)."""
    return ((F, F), (F + (-F) % 4 + 4, F + (-F) % 4 + 8), (F + (-F) % 2 + 1, F + (-F) % 2 + 3))


def _strided(t, ld):
    """t's values in a [rows + GUARD, ld] sentinel-filled buffer; the view of them."""
    buf = torch.full((t.size(0) + GUARD, ld), SENT, dtype=torch.int32, device=DEV)
    view = buf.view(torch.float32)[:t.size(0), :t.size(1)]
    view.copy_(t)
    return buf, view


def _dropout_rows(h, p, seed, out, n_rows_dev=None, seed_dev=None):
    rc = _lib.load().ngnn_dropout_rows(_lib.ptr(h), h.stride(0), h.size(0), _lib.ptr(n_rows_dev), h.size(1), p,
                                       seed, _lib.ptr(seed_dev), _lib.ptr(out), out.stride(0),
                                       _lib.stream_handle(DEV))
    assert rc == _lib.OK, rc


def _expect_dropout(h, p, seed):
    """int32 bits of where(keep, fl32(h * scale), +0.0) on the host."""
    n, F = h.shape
    if dropout_thresh(p) == 0:
        return _bits(h)
    keep = dropout_keep(seed, n, F, p).numpy()
    prod = h.numpy() * np.float32(dropout_scale(p))  # one fp32 product
    assert prod.dtype == np.float32
    return _bits(torch.from_numpy(np.where(keep, prod, np.float32(0.0))))


def _assert_untouched(buf, n_live, F, what):
    raw = buf.cpu().clone()
    raw[:n_live, :F] = SENT
    assert bool((raw == SENT).all()), f"{what}: a store outside out[:{n_live}, :{F}]"


@pytest.mark.parametrize("F", FS)
def test_dropout_rows_matches_host_replica(F):
    for n in ROWS:
        h = torch.randn(n, F, generator=torch.Generator().manual_seed(F * 1000 + n))
        h[::2, ::3] = 0.0  # exact zeros too (a ReLU output)
        for ldh, ldo in _lds(F):
            _, hd = _strided(h, ldh)
            for p in PS:
                what = f"F={F} n={n} ldh={ldh} ldo={ldo} p={p:g}"
                buf, out = _buffer(n, F, ldo)
                _dropout_rows(hd, p, SEED, out)
                _assert_untouched(buf, n, F, what)
                got = _bits(out.cpu())
                assert torch.equal(got, _expect_dropout(h, p, SEED)), what
                if dropout_thresh(p) == 256:
                    assert bool((got == 0).all()), what
    torch.cuda.synchronize()


@pytest.mark.parametrize("F", (3, 33, 100))
def test_dropout_rows_device_bound_and_seed_word(F):
    n, nrd = 300, 211
    h = torch.randn(n, F, generator=torch.Generator().manual_seed(F))
    nrd_t = torch.tensor([nrd], dtype=torch.int32, device=DEV)
    over_t = torch.tensor([n + 50], dtype=torch.int32, device=DEV)  # a bound past n_rows: n_rows holds
    sd_t = torch.tensor([SEED_B], dtype=torch.int64, device=DEV)
    assert SEED_A >> 32 and SEED_B >> 32 and (SEED_A ^ SEED_B) >> 32
    for ldh, ldo in _lds(F):
        _, hd = _strided(h, ldh)
        for p in (0.5, 0.3):
            what = f"F={F} ldh={ldh} ldo={ldo} p={p:g}"
            buf, out = _buffer(n, F, ldo)
            _dropout_rows(hd, p, SEED, out, n_rows_dev=nrd_t)
            _assert_untouched(buf, nrd, F, what + " n_rows_dev")
            assert torch.equal(_bits(out.cpu()[:nrd]), _expect_dropout(h, p, SEED)[:nrd]), what
            buf, out = _buffer(n, F, ldo)
            _dropout_rows(hd, p, SEED, out, n_rows_dev=over_t)
            _assert_untouched(buf, n, F, what + " bound past n_rows")
            assert torch.equal(_bits(out.cpu()), _expect_dropout(h, p, SEED)), what
            buf, out = _buffer(n, F, ldo)
            _dropout_rows(hd, p, SEED_A, out, seed_dev=sd_t)
            assert torch.equal(_bits(out.cpu()), _expect_dropout(h, p, SEED_A ^ SEED_B)), what + " seed_dev"
            assert not torch.equal(_bits(out.cpu()), _expect_dropout(h, p, SEED_A)), what + " seed_dev ignored"


@pytest.mark.parametrize("route,K,Fo", [("A", 64, 48), ("A", 64, 40), ("B", 256, 200), ("C", 428, 100)])
def test_dropout_rows_equals_fused_epilogue(route, K, Fo):
    """layer(relu, p = 0) then ngnn_dropout_rows == layer(relu, p), bit for
    bit.  Route C's second launch starts at column 48: mid-way through a
    32-column hash word."""
    N = 83
    s = _assert_rt_route(route, K, Fo)
    if route == "C":
        assert s % 32 == 16
    _, d = _layer(K, Fo, N)
    blk = _graph(N, N)[1]
    sd_t = torch.tensor([SEED_B], dtype=torch.int64, device=DEV)
    _, h = _buffer(N, Fo, Fo + 4)
    _raw(d, blk, "mean", h, True, 0.0, SEED)
    hc = h.cpu()
    assert bool((hc >= 0).all()) and bool((hc == 0).any()) and bool((hc > 0).any())
    for p in (0.5, 0.3):
        for seed, seed_dev in ((SEED, None), (SEED_A, sd_t)):
            what = f"{route} K={K} Fo={Fo} p={p:g} seed_dev={seed_dev is not None}"
            _, want = _buffer(N, Fo, Fo + 4)
            _raw(d, blk, "mean", want, True, p, seed, seed_dev=seed_dev)
            buf, got = _buffer(N, Fo, Fo + 4)
            _dropout_rows(h, p, seed, got, seed_dev=seed_dev)
            _assert_untouched(buf, N, Fo, what)
            assert torch.equal(_bits(got.cpu()), _bits(want.cpu())), what
            assert bool((got.cpu()[hc > 0] == 0).any()), what + ": nothing dropped"
    assert N_EDGE < N  # (both phases of the row-tile kernel ran)


# ------------------------------------------------------------- ngnn_tap_grad
def _tap_grad(dy, xd, yscale, dh, h, r_ptr, dz, n_rows=None):
    F = h.size(1)
    rc = _lib.load().ngnn_tap_grad(_lib.ptr(dy), dy.stride(0) if dy is not None else F, _lib.ptr(xd),
                                   xd.stride(0) if xd is not None else F, yscale, _lib.ptr(dh), dh.stride(0),
                                   _lib.ptr(h), h.stride(0), h.size(0) if n_rows is None else n_rows,
                                   _lib.ptr(r_ptr), F, _lib.ptr(dz), dz.stride(0), _lib.stream_handle(DEV))
    assert rc == _lib.OK, rc


def _tap_case(n, F, p, seed):
    """Host tensors of one case: h a ReLU output with exact zeros, xd its hash
    dropout, dy and dh with exact zeros of their own (so that each term
    vanishes somewhere the other does not)."""
    g = torch.Generator().manual_seed(seed)
    h = torch.randn(n, F, generator=g).clamp(min=0.0)
    keep = dropout_keep(SEED, n, F, p)
    xd = torch.from_numpy(np.where(keep.numpy(), h.numpy() * np.float32(dropout_scale(p)), np.float32(0.0)))
    dy = torch.randn(n, F, generator=g)
    dh = torch.randn(n, F, generator=g)
    dy[torch.rand(n, F, generator=g) < 0.2] = 0.0
    dh[torch.rand(n, F, generator=g) < 0.2] = 0.0
    return h, xd, dy, dh


def _check_tap(got, dy, xd, ys, dh, h, what):
    """got [rows, F] (host fp32) against the three-form contract."""
    zero = torch.zeros_like(h)
    if dy is None:
        t1, t1_64 = zero, zero.double()
    else:
        m1 = (xd > 0) if xd is not None else (h > 0)
        s = np.float32(ys if xd is not None else 1.0)
        t1 = torch.from_numpy(np.where(m1.numpy(), dy.numpy() * s, np.float32(0.0)))
        t1_64 = torch.where(m1, dy.double() * float(s), zero.double())
    t2 = torch.where(h > 0, dh, zero)
    ref = t1_64 + t2.double()
    f32 = t1 + t2  # the same fp32 operations on the host
    one = (t1 == 0) | (t2 == 0)
    if h.numel() >= 100:  # (the case holds both kinds of element)
        assert bool(one.any()) and (dy is None or bool((~one).any())), what
    # one term zero: the other term, one fp32 product, exactly (0.0 == -0.0)
    assert bool((got[one] == f32[one]).all()), f"{what}: not exact where one term is zero"
    if float(np.log2(ys)).is_integer() or xd is None or dy is None:  # exact products: fp64 is the yardstick
        assert bool((got[one].double() == ref[one]).all()), f"{what}: not exact where one term is zero"
        if bool((~one).any()):
            larger = torch.maximum(t1.abs(), t2.abs())[~one]
            ulp = torch.from_numpy(np.spacing(larger.numpy())).double()
            worst = float(((got.double() - ref)[~one].abs() / ulp).max())
            print(f"{what}: worst |got - fp64| = {worst:.3f} ulp of the larger term")
            assert worst <= 1.0, what
    assert bool((got == f32).all()), f"{what}: differs from the fp32 evaluation"


@pytest.mark.parametrize("F", FS)
def test_tap_grad_three_forms_vs_fp64(F):
    n, bound = 41, 29
    r_t = torch.tensor([bound], dtype=torch.int32, device=DEV)
    for p in (0.5, 0.75, 0.3):
        ys = dropout_scale(p)
        h, xd, dy, dh = _tap_case(n, F, p, F * 10 + int(p * 100))
        for ld, ldz in _lds(F):
            dev = {k: _strided(v, ld)[1] for k, v in dict(h=h, xd=xd, dy=dy, dh=dh).items()}
            for form, (a, x) in (("xd", (dy, xd)), ("no xd", (dy, None)), ("no dy", (None, None))):
                what = f"F={F} p={p:g} ld={ld} ldz={ldz} form '{form}'"
                buf, dz = _buffer(n, F, ldz)
                _tap_grad(dev["dy"] if a is not None else None, dev["xd"] if x is not None else None, ys,
                          dev["dh"], dev["h"], r_t, dz)
                _assert_untouched(buf, bound, F, what)
                _check_tap(dz.cpu()[:bound], None if a is None else a[:bound], None if x is None else x[:bound],
                           ys, dh[:bound], h[:bound], what)
            # in place: dz is dy's buffer; rows at or past the bound keep dy
            buf, dyv = _strided(dy, ldz)
            _tap_grad(dyv, dev["xd"], ys, dev["dh"], dev["h"], r_t, dyv)
            _assert_untouched(buf, n, F, f"F={F} in place")
            got = dyv.cpu()
            assert torch.equal(_bits(got[bound:]), _bits(dy[bound:]))
            _check_tap(got[:bound], dy[:bound], xd[:bound], ys, dh[:bound], h[:bound], f"F={F} p={p:g} in place")
    # no device bound: n_rows alone
    buf, dz = _buffer(n, F, F)
    _tap_grad(dev["dy"], dev["xd"], ys, dev["dh"], dev["h"], None, dz, n_rows=bound)
    _assert_untouched(buf, bound, F, f"F={F} host bound")


def test_capture_and_replay():
    n, F, p = 300, 100, 0.3
    h, xd, dy, dh = _tap_case(n, F, p, 5)
    hd, dyd, dhd = h.to(DEV), dy.to(DEV), dh.to(DEV)
    out = torch.zeros(n, F, device=DEV)
    dz = torch.zeros(n, F, device=DEV)
    r_t = torch.tensor([n], dtype=torch.int32, device=DEV)
    sd_t = torch.tensor([0], dtype=torch.int64, device=DEV)

    def both():
        _dropout_rows(hd, p, SEED, out, seed_dev=sd_t)
        _tap_grad(dyd, out, dropout_scale(p), dhd, hd, r_t, dz)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        both()  # (warm-up: the library is loaded outside the capture)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert torch.equal(_bits(out.cpu()), _expect_dropout(h, p, SEED))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        both()
    for word, bound in ((SEED_B, 123), (0, n)):  # the replay reads the device words afresh
        sd_t.fill_(word)
        r_t.fill_(bound)
        out.zero_()
        dz.fill_(7.0)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(_bits(out.cpu()), _expect_dropout(h, p, SEED ^ word))
        got = dz.cpu()
        assert bool((got[bound:] == 7.0).all())
        _check_tap(got[:bound], dy[:bound], out.cpu()[:bound], dropout_scale(p), dh[:bound], h[:bound],
                   f"replay word={word:#x} bound={bound}")
