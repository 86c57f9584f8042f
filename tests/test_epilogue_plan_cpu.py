"""ngnn_sage_fwd_slice_cols (include/ngnn.h): the row-tile kernel's column
slicing of a per-layer forward, pinned on the shapes the epilogue tests
(test_gpu_epilogue_forms.py) rely on.  No device: the query is pure.

The table follows rt_root_image (csrc/ngnn_sage_rt.hip) and kRtLdsCap =
160 KiB - 1280 = 162,560 B.  One 16-column tile of the split-bf16 root image
is 3 KiB per 32-column chunk of K (1 KiB with NGNN_W_BF16) + 256 B per fp32
tail step of 4 columns (at most 3 steps; a longer tail is one more zero-padded
chunk); of the exact-fp32 image 1 KiB per 16 columns of K.  The slice is the
first of 16, 8, 6, 4, 3, 2 tiles whose image fits."""
import pytest

from ngnn import _lib

SUM, MEAN, MAX = 0, 1, 2
CAP = 160 * 1024 - 1280

# (K, flags, slice columns)
TABLE = [
    (100, 0, 256),   # 3 chunks + 1 tail step: 9,472 B a tile, 16 tiles
    (128, 0, 128),   # 4 chunks: 12 KiB a tile, 16 tiles = 192 KiB > cap
    (200, 0, 128),   # 6 chunks + 2 tail steps
    (256, 0, 96),    # 8 chunks: 24 KiB, 6 tiles = 144 KiB
    (300, 0, 64),    # 9 chunks + 3 tail steps
    (424, 0, 64),    # 13 chunks + 2 tail steps: 40,448 B, 4 tiles
    (428, 0, 48),    # 13 chunks + 3 tail steps: 40,704 B -> 3 tiles
    (444, 0, 48),    # a 28-column tail: 14 chunks, zero padded
    (512, 0, 48),    # 16 chunks: 48 KiB, 3 tiles = 144 KiB
    (556, 0, 48),    # 17 chunks + 3 tail steps: 52,992 B, 3 tiles = 158,976 B
    (560, 0, 32),    # 17 chunks + 4 steps -> 18 chunks: 54 KiB, 2 tiles
    (640, _lib.MATH_EXACT_F32, 48),  # 40 KiB a tile
    (256, _lib.W_BF16, 256),         # one part: 8 KiB a tile
]


@pytest.mark.parametrize("K,flags,want", TABLE)
def test_slice_table(K, flags, want):
    q = _lib.load().ngnn_sage_fwd_slice_cols
    # (an F_out of at most four slices: more prefers the wide path, whose
    # routing counts slices of the three-part image -- 96 columns at K = 256)
    for Fo in (1, want, want + 1, 4 * (96 if flags & _lib.W_BF16 else want)):
        for reduce in (SUM, MEAN, MAX):
            got = q(K, Fo, reduce | flags)
            if flags & _lib.W_BF16 and reduce == MAX:
                assert got == 96, (K, Fo, got)  # (max layers keep the three-part image)
            else:
                assert got == want, (K, Fo, reduce, got)


def test_slice_parity_of_the_odd_routes():
    """The shapes the epilogue tests run for odd column slices: a 48-column
    slice puts every second launch at an odd 16-column tile."""
    q = _lib.load().ngnn_sage_fwd_slice_cols
    for K, Fo, flags in ((512, 176, 0), (428, 100, 0), (640, 100, _lib.MATH_EXACT_F32)):
        s = q(K, Fo, MEAN | flags)
        assert s == 48 and (s >> 4) & 1 and Fo > s


def test_more_than_four_slices_or_unaligned_k_leave_the_kernel():
    lib = _lib.load()
    q = lib.ngnn_sage_fwd_slice_cols
    assert q(512, 192, MEAN) == 48
    assert q(512, 193, MEAN) == 0 and lib.ngnn_sage_wide_preferred(512, 193, 0) == 1
    assert q(256, 384, MEAN) == 96 and q(256, 385, MEAN) == 0
    for K in (30, 62, 101, 127, 767):
        assert q(K, 20, MEAN) == 0 and q(K, 20, MEAN | _lib.MATH_EXACT_F32) == 0
    # bf16 rows never take the wide path, and not the exact-fp32 root term
    assert q(512, 193, MEAN | _lib.X_BF16 | _lib.W_BF16) == 128
    assert q(100, 64, MEAN | _lib.X_BF16 | _lib.MATH_EXACT_F32) == 0


def test_query_agrees_with_the_wide_routing_and_the_cap():
    """Over a sweep: 0 exactly where ngnn_sage_wide_preferred says wide; else a
    multiple of 16 from the tile ladder whose split-bf16 image fits the cap
    while the next wider one does not (the image size as the module docstring
    states it)."""
    lib = _lib.load()
    ladder = (16, 8, 6, 4, 3, 2)

    def tile_bytes(K, exact):
        if exact:
            return -(-K // 16) * 1024
        C, T4 = K // 32, -(-(K % 32) // 4)
        if T4 > 3:
            C, T4 = C + 1, 0
        return 3 * C * 1024 + T4 * 256

    n_rt = 0
    for exact in (0, 1):
        fl = _lib.MATH_EXACT_F32 if exact else 0
        for K in list(range(4, 1200, 4)) + [1, 2, 3, 5, 99, 511]:
            for Fo in (1, 16, 47, 48, 49, 96, 97, 192, 193, 256, 257, 512, 1024, 1025):
                got = lib.ngnn_sage_fwd_slice_cols(K, Fo, MEAN | fl)
                wide = lib.ngnn_sage_wide_preferred(K, Fo, exact)
                assert (got == 0) == bool(wide), (K, Fo, exact, got, wide)
                if got:
                    n_rt += 1
                    fit = [c for c in ladder if c * tile_bytes(K, exact) <= CAP]
                    assert got == 16 * fit[0], (K, Fo, exact, got)
                    assert -(-Fo // got) <= 4
    assert n_rt > 1000


def test_narrow_mode_is_one_launch_of_both_halves():
    q = _lib.load().ngnn_sage_fwd_slice_cols
    assert q(256, 47, MEAN | _lib.FWD_NARROW) == 47   # 3 + 3 tiles of the 6 that fit
    assert q(256, 49, MEAN | _lib.FWD_NARROW) == 96   # 4 + 4 do not: the plain form
    assert q(256, 47, MAX | _lib.FWD_NARROW) == 96    # (max is not linear)


def test_query_refuses_bad_arguments():
    q = _lib.load().ngnn_sage_fwd_slice_cols
    assert q(0, 64, MEAN) == _lib.E_ARG and q(64, 0, MEAN) == _lib.E_ARG
    assert q(-4, 64, MEAN) == _lib.E_ARG and q(64, -1, MEAN) == _lib.E_ARG
    assert q(64, 64, 3) == _lib.E_ARG and q(64, 64, 3 | _lib.W_BF16) == _lib.E_ARG
    assert q(64, 64, MEAN | 0x4000) == _lib.E_ARG     # (an unknown flag bit)
    assert q(2**31, 64, MEAN) == _lib.E_RANGE and q(64, 2**31, MEAN) == _lib.E_RANGE
