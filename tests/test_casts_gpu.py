"""The cast kernels of csrc/ngnn_optim.hip, value for value against torch on
the CPU (compared as int16 / int32 bit patterns), every destination between
sentinels:

* ngnn_cast_f32_bf16 into a destination that is only 8-byte aligned (the
  4-elements-per-thread kernel; fresh allocations always take the 8-element one);
* ngnn_cast_f32_bf16_rows under a device row count;
* ngnn_cast_tensors both ways, ngnn_cast_tensors_ex with its division, mixed
  dtypes and the in-place form, and their Python callers' chunking by 16;
* ngnn_widen_bf16_rows with padded rows on either side and a device row bound.
"""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
F32, BF16 = torch.float32, torch.bfloat16
PAD = 16


def _bits(t):
    return t.view(torch.int16 if t.dtype == BF16 else torch.int32)


def _sent(dtype):
    return 0x5A5A if dtype == BF16 else 0x5A5A5A5A


def _guarded(n, dtype, offset=0):
    """(buffer, its view [offset, offset + n)): sentinel bit patterns everywhere."""
    buf = torch.empty(offset + n + PAD, dtype=dtype, device=DEV)
    _bits(buf).fill_(_sent(dtype))
    return buf, buf[offset:offset + n]


def _untouched(buf, lo, hi):
    """Every element of buf outside [lo, hi) still holds its sentinel."""
    b = _bits(buf).cpu()
    return bool((b[:lo] == _sent(buf.dtype)).all()) and bool((b[hi:] == _sent(buf.dtype)).all())


def _f32_from_bits(bits):
    return torch.tensor(bits, dtype=torch.int64).to(torch.int32).view(F32)


# +-inf, the two tie cases (to even: down, up), four NaN patterns (quiet +/-,
# a signalling payload, low payload bits only)
_NAN_BITS = [0x7FC00000, 0xFFC00000 - (1 << 32), 0x7F800001, 0x7FBFFFFF]
_SPECIAL = torch.cat([torch.tensor([float("inf"), -float("inf"), 1.0 + 2 ** -8, -(1.0 + 3 * 2 ** -8)]),
                      _f32_from_bits(_NAN_BITS)])
# +-0, fp32 subnormals (the smallest, the largest, two bf16 ties among them)
_SMALL = torch.cat([torch.tensor([0.0, -0.0]), _f32_from_bits([0x00000001, 0x007FFFFF, 0x00008000, 0x00018000,
                                                               0x80000001 - (1 << 32), 0x00800000])])


def _f32_input(n, seed, small=False):
    x = torch.randn(n, generator=torch.Generator().manual_seed(seed)) * 3
    sp = torch.cat([_SPECIAL, _SMALL]) if small else _SPECIAL
    k = min(n, sp.numel())
    # (short inputs: a rotating choice of the special values)
    x[:k] = sp.roll(-(seed % sp.numel()))[:k] if n < sp.numel() else sp
    return x


def _want_bf16_bits(x):
    """torch's CPU cast on every non-NaN value; every NaN the canonical quiet
    0x7FC0 (c10's round_to_nearest_even, the header's promise -- the CPU's
    vectorised cast may leave another NaN pattern)."""
    w = _bits(x.to(BF16)).clone()
    w[x.isnan()] = 0x7FC0
    return w


def _lib():
    from ngnn import _lib as L
    return L, L.load(), L.stream_handle(DEV)


@pytest.mark.parametrize("n", [1, 3, 4, 5, 4099, 1 + 4 * 256 * 2048 * 4])
def test_cast_f32_bf16_into_an_8_byte_aligned_destination(n):
    """A destination at element offset 4 of a bf16 buffer: k_cast_bf16<false>
    (8-B stores).  The largest size runs its 4-deep unrolled loop once in
    every thread, plus a 1-element tail."""
    L, lib, st = _lib()
    x = _f32_input(n, seed=n)
    buf, dst = _guarded(n, BF16, offset=4)
    assert dst.data_ptr() % 16 == 8
    xd = x.to(DEV)
    L.check(lib.ngnn_cast_f32_bf16(xd.data_ptr(), dst.data_ptr(), n, st), "cast")
    torch.cuda.synchronize()
    assert torch.equal(_bits(dst).cpu(), _want_bf16_bits(x))
    assert _untouched(buf, 4, 4 + n)
    assert torch.equal(_bits(xd).cpu(), _bits(x))


def test_cast_f32_bf16_refuses_a_2_byte_aligned_destination():
    L, lib, st = _lib()
    x = torch.ones(64, device=DEV)
    buf, dst = _guarded(64, BF16, offset=1)
    assert lib.ngnn_cast_f32_bf16(x.data_ptr(), dst.data_ptr(), 64, st) == L.E_SHAPE
    torch.cuda.synchronize()
    assert _untouched(buf, 0, 0)


@pytest.mark.parametrize("row_elems", [1, 47, 48])
def test_cast_f32_bf16_rows_device_row_count(row_elems):
    """Rows below min(n_rows, max(*n_rows_dev, 0)) are torch's cast, every
    later row keeps its sentinel (both kernels: 16-B and 8-B destinations)."""
    L, lib, st = _lib()
    n_rows = 37
    x = _f32_input(n_rows * row_elems, seed=row_elems)
    want = _want_bf16_bits(x)
    xd = x.to(DEV)
    for offset in (0, 4):
        for dev in (0, 1, 36, 37, 1000, -5):
            buf, dst = _guarded(n_rows * row_elems, BF16, offset=offset)
            cnt = torch.tensor([dev], dtype=torch.int32, device=DEV)
            L.check(lib.ngnn_cast_f32_bf16_rows(xd.data_ptr(), dst.data_ptr(), n_rows, row_elems,
                                                cnt.data_ptr(), st), "cast rows")
            torch.cuda.synchronize()
            done = min(n_rows, max(dev, 0)) * row_elems
            assert torch.equal(_bits(dst).cpu()[:done], want[:done]), (offset, dev)
            assert _untouched(buf, offset, offset + done), (offset, dev)
            assert int(cnt) == dev
    # no device count: every row
    buf, dst = _guarded(n_rows * row_elems, BF16)
    L.check(lib.ngnn_cast_f32_bf16_rows(xd.data_ptr(), dst.data_ptr(), n_rows, row_elems, None, st), "cast rows")
    torch.cuda.synchronize()
    assert torch.equal(_bits(dst).cpu(), want) and _untouched(buf, 0, n_rows * row_elems)


_SIZES16 = [0, 1, 2, 3, 255, 256, 257, 1023, 1024, 1025, 7, 0, 4099, 5, 33, 600]


def _ptrs(ts):
    return (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


def _numels(ts):
    return (ctypes.c_int64 * len(ts))(*[t.numel() for t in ts])


def _on_device(cpu, odd):
    """cpu tensor -> (buffer, device view holding it): at element offset 1 of
    a sentinel buffer when odd, else at offset 0."""
    buf, v = _guarded(cpu.numel(), cpu.dtype, offset=1 if odd else 0)
    v.copy_(cpu)
    return buf, v


@pytest.mark.parametrize("to_bf16", [False, True], ids=["widen", "narrow"])
def test_cast_tensors_16_in_one_launch(to_bf16):
    """bf16 -> fp32 exact (every bit pattern class); fp32 -> bf16 torch's
    .to(bfloat16) on every non-NaN input (+-inf, +-0, subnormals, ties), every
    NaN a NaN (also 0x7F800001, which truncation would make inf).  Sizes
    around the workgroup, empty tensors, odd-offset views on both sides."""
    L, lib, st = _lib()
    g = torch.Generator().manual_seed(5)
    if to_bf16:
        srcs = [_f32_input(n, seed=k, small=True) for k, n in enumerate(_SIZES16)]
        wants = [s.to(BF16) for s in srcs]
    else:
        srcs = [torch.randint(-32768, 32768, (n,), generator=g).to(torch.int16).view(BF16) for n in _SIZES16]
        wants = [s.float() for s in srcs]
    S = [_on_device(s, odd=k % 2 == 1) for k, s in enumerate(srcs)]
    D = [_guarded(s.numel(), BF16 if to_bf16 else F32, offset=1 if k % 3 == 1 else 0) for k, s in enumerate(srcs)]
    L.check(lib.ngnn_cast_tensors(16, _ptrs([v for _, v in S]), _ptrs([v for _, v in D]),
                                  _numels(srcs), int(to_bf16), st), "cast_tensors")
    torch.cuda.synchronize()
    for k, (src, want, (dbuf, dv), (sbuf, sv)) in enumerate(zip(srcs, wants, D, S)):
        got = dv.cpu()
        off = 1 if k % 3 == 1 else 0
        assert _untouched(dbuf, off, off + src.numel()), k
        assert torch.equal(_bits(sv).cpu(), _bits(src)), k  # (the source is read only)
        if to_bf16:
            nan = src.isnan()
            assert bool(got[nan].isnan().all()), k
            assert torch.equal(_bits(got)[~nan], _bits(want)[~nan]), k
        else:
            assert torch.equal(_bits(got), _bits(want)), k
    if to_bf16:
        assert sum(int(s.isnan().sum()) for s in srcs) >= 8


def test_cast_tensors_refuses_17():
    L, lib, st = _lib()
    a = [torch.zeros(4, device=DEV) for _ in range(17)]
    b = [torch.zeros(4, dtype=BF16, device=DEV) for _ in range(17)]
    assert lib.ngnn_cast_tensors(17, _ptrs(a), _ptrs(b), _numels(a), 1, st) == L.E_ARG
    sd = (ctypes.c_int32 * 17)(*([L.F32] * 17))
    dd = (ctypes.c_int32 * 17)(*([L.BF16] * 17))
    assert lib.ngnn_cast_tensors_ex(17, _ptrs(a), _ptrs(b), _numels(a), sd, dd, 1.0, st) == L.E_ARG


def test_fused_cast_tensors_chunks_33():
    from ngnn import fused
    g = torch.Generator().manual_seed(6)
    srcs = [torch.randn(1 + 37 * k, generator=g) for k in range(33)]
    dst = [torch.empty(s.numel(), dtype=BF16, device=DEV) for s in srcs]
    fused._cast_tensors([s.to(DEV) for s in srcs], dst, to_bf16=True)
    back = [torch.empty(s.numel(), device=DEV) for s in srcs]
    fused._cast_tensors(dst, back, to_bf16=False)
    torch.cuda.synchronize()
    for s, d, b in zip(srcs, dst, back):
        assert torch.equal(_bits(d.cpu()), _bits(s.to(BF16)))
        assert torch.equal(_bits(b.cpu()), _bits(s.to(BF16).float()))


def _ex_input(n, dtype, seed):
    x = torch.randn(n, generator=torch.Generator().manual_seed(seed)) * 3
    sp = torch.tensor([float("inf"), -float("inf"), 0.0, -0.0, 1.0 + 2 ** -8, -(1.0 + 3 * 2 ** -8),
                       3.0 * (1.0 + 2 ** -8), 3.0 * (1.0 + 3 * 2 ** -8), 1e-30, 3e38])
    if n >= sp.numel():
        x[:sp.numel()] = sp
    return x.to(dtype)


def _ex_want(src, dst_dtype, d):
    """(src.float() / d) rounded ONCE to the destination dtype (divisor 1: no
    division)."""
    v = src.float()
    if d != 1:
        v = v / torch.tensor(float(d))
    return v.to(dst_dtype)


@pytest.mark.parametrize("d", [1, 2, 3, 8])
def test_cast_tensors_ex_mixed_dtypes_and_division(d):
    """All four (source, destination) dtype pairs in one 16-tensor call: the
    IEEE quotient in fp32, rounded once (a division after the bf16 rounding
    differs on the tie inputs and on random ones)."""
    L, lib, st = _lib()
    pairs = [(F32, F32), (F32, BF16), (BF16, F32), (BF16, BF16)]
    srcs = [_ex_input(n, pairs[k % 4][0], seed=20 + k) for k, n in enumerate(_SIZES16)]
    dts = [pairs[k % 4][1] for k in range(16)]
    S = [_on_device(s, odd=k % 5 == 2) for k, s in enumerate(srcs)]
    D = [_guarded(s.numel(), dt, offset=1 if k % 3 == 1 else 0) for k, (s, dt) in enumerate(zip(srcs, dts))]
    code = {F32: L.F32, BF16: L.BF16}
    sd = (ctypes.c_int32 * 16)(*[code[s.dtype] for s in srcs])
    dd = (ctypes.c_int32 * 16)(*[code[dt] for dt in dts])
    L.check(lib.ngnn_cast_tensors_ex(16, _ptrs([v for _, v in S]), _ptrs([v for _, v in D]), _numels(srcs),
                                     sd, dd, float(d), st), "cast_tensors_ex")
    torch.cuda.synchronize()
    for k, (src, dt, (dbuf, dv)) in enumerate(zip(srcs, dts, D)):
        off = 1 if k % 3 == 1 else 0
        assert _untouched(dbuf, off, off + src.numel()), k
        assert torch.equal(_bits(dv.cpu()), _bits(_ex_want(src, dt, d))), (k, src.dtype, dt)


@pytest.mark.parametrize("d", [1, 3])
def test_cast_tensors_ex_in_place(d):
    """src[k] == dst[k] with equal dtypes (the fp32 gradients that ARE bucket
    views): fp32 and bf16, an empty entry, an odd-offset view; in place with
    a width change is refused."""
    L, lib, st = _lib()
    srcs = [_ex_input(1025, F32, 1), _ex_input(257, BF16, 2), _ex_input(0, F32, 3), _ex_input(33, BF16, 4),
            _ex_input(7, F32, 5)]
    S = [_on_device(s, odd=k >= 3) for k, s in enumerate(srcs)]
    code = {F32: L.F32, BF16: L.BF16}
    dts = (ctypes.c_int32 * 5)(*[code[s.dtype] for s in srcs])
    P = _ptrs([v for _, v in S])
    L.check(lib.ngnn_cast_tensors_ex(5, P, P, _numels(srcs), dts, dts, float(d), st), "in place")
    torch.cuda.synchronize()
    for k, (src, (buf, v)) in enumerate(zip(srcs, S)):
        off = 1 if k >= 3 else 0
        assert _untouched(buf, off, off + src.numel()), k
        assert torch.equal(_bits(v.cpu()), _bits(_ex_want(src, src.dtype, d))), k
    other = (ctypes.c_int32 * 5)(*[code[BF16 if s.dtype == F32 else F32] for s in srcs])
    assert lib.ngnn_cast_tensors_ex(5, P, P, _numels(srcs), dts, other, 1.0, st) == L.E_ARG


def test_distributed_cast_tensors_chunks_and_falls_back(monkeypatch):
    """20 tensors, one not contiguous: that one by ATen, the other 19 in two
    ngnn_cast_tensors_ex launches (16 + 3), every value (src / 2) rounded once."""
    from ngnn import distributed
    L, lib, _ = _lib()
    srcs = [_ex_input(10 + 13 * k, BF16 if k % 2 else F32, seed=40 + k) for k in range(20)]
    dev_src = [s.to(DEV) for s in srcs]
    dst = [torch.empty(s.numel(), dtype=F32 if k % 3 else BF16, device=DEV) for k, s in enumerate(srcs)]
    srcs[7] = torch.randn(6, 4, generator=torch.Generator().manual_seed(9))
    dev_src[7] = srcs[7].to(DEV).t()  # (not contiguous)
    dst[7] = torch.empty(4, 6, device=DEV)
    calls, orig = [], lib.ngnn_cast_tensors_ex

    def spy(n, *a):
        calls.append(n)
        return orig(n, *a)

    monkeypatch.setattr(lib, "ngnn_cast_tensors_ex", spy)
    distributed.cast_tensors(dev_src, dst, divisor=2.0)
    torch.cuda.synchronize()
    assert calls == [16, 3]
    for k, (s, d) in enumerate(zip(srcs, dst)):
        if k == 7:
            assert torch.equal(d.cpu(), s.t() / 2)
        else:
            assert torch.equal(_bits(d.cpu()), _bits(_ex_want(s, d.dtype, 2))), k


@pytest.mark.parametrize("F", [1, 47])
def test_widen_bf16_rows_strides_and_row_bound(F):
    """Rows of F values out of rows lds apart into rows ldd apart, below
    min(n_rows, *n_rows_dev): exact values; padding columns and later rows
    keep their sentinels."""
    L, lib, st = _lib()
    n_rows = 29
    g = torch.Generator().manual_seed(F)
    for lds in (F, F + 3):
        src = torch.randint(-32768, 32768, (n_rows, lds), generator=g).to(torch.int16).view(BF16)
        sd = src.to(DEV)
        want = _bits(src[:, :F].float())
        for ldd in (F, F + 5):
            for dev in (None, 0, 10, 29, 1000):
                buf, dst = _guarded(n_rows * ldd, F32)
                cnt = None if dev is None else torch.tensor([dev], dtype=torch.int32, device=DEV)
                L.check(lib.ngnn_widen_bf16_rows(sd.data_ptr(), lds, F, n_rows, L.ptr(cnt), dst.data_ptr(), ldd,
                                                 st), "widen")
                torch.cuda.synchronize()
                rows = n_rows if dev is None else min(n_rows, dev)
                got = _bits(buf).cpu()
                exp = torch.full_like(got, _sent(F32))
                exp[:n_rows * ldd].view(n_rows, ldd)[:rows, :F] = want[:rows]
                assert torch.equal(got, exp), (lds, ldd, dev)
    buf, dst = _guarded(n_rows * F, F32)
    assert lib.ngnn_widen_bf16_rows(sd.data_ptr(), F - 1, F, n_rows, None, dst.data_ptr(), F, st) == L.E_ARG
    assert lib.ngnn_widen_bf16_rows(sd.data_ptr(), F, F, n_rows, None, dst.data_ptr(), F - 1, st) == L.E_ARG
    torch.cuda.synchronize()
    assert _untouched(buf, 0, 0)
