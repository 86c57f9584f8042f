"""ngnn_sage_dgrad_route (include/ngnn.h): the one copy of the per-layer
backward's input-gradient route rule, against a restatement of it and against
the envelope checks of the two entry points it stands for.  No device: the
query is pure, and the entries return before any launch with n_rows = 0."""
import numpy as np

from ngnn import _lib

SUM, MEAN, MAX = 0, 1, 2
FD_MAXF, LDS_MAX, LD_ROWS = 512, 150 * 1024, 64


def _route(Fo, K, reduce, deterministic):
    """The rule as the header states it; the lowdim envelope restated from
    the kernel's layout: ntw column tiles per wave (a power of two, two waves
    cover ceil(K / 16) tiles), LDS = the [C4 / 2][2 ntw][64] weight image +
    one 64-row stage of [dz | g | 4 pad] floats."""
    if deterministic:
        return _lib.DGRAD_GEMM_GATHER
    if Fo < K and reduce in (SUM, MEAN):
        half = -(-(-(-K // 16)) // 2)
        ntw = 1
        while ntw < half:
            ntw *= 2
        C4 = (Fo + 3) & ~3
        lds = 4 * ((C4 // 2) * 2 * ntw * 64 + LD_ROWS * (2 * C4 + 4))
        if ntw <= 16 and lds <= LDS_MAX:
            return _lib.DGRAD_LOWDIM
    if Fo <= FD_MAXF and 8 * Fo * K + 16 * FD_MAXF <= LDS_MAX:
        return _lib.DGRAD_FUSED
    return _lib.DGRAD_GEMM_SCATTER


def test_route_matches_restatement():
    route = _lib.load().ngnn_sage_dgrad_route
    for reduce in (SUM, MEAN, MAX):
        count = np.zeros(4, dtype=np.int64)
        for Fo in range(1, 601):
            for K in range(1, 1101):
                got = route(Fo, K, reduce, 0)
                assert got == _route(Fo, K, reduce, 0), (Fo, K, reduce, got)
                count[got] += 1
        assert count[_lib.DGRAD_GEMM_GATHER] == 0
        assert count[_lib.DGRAD_FUSED] > 0 and count[_lib.DGRAD_GEMM_SCATTER] > 0
        assert (count[_lib.DGRAD_LOWDIM] > 0) == (reduce != MAX)


def test_route_deterministic_is_always_gather():
    route = _lib.load().ngnn_sage_dgrad_route
    for Fo in (1, 7, 32, 47, 64, 256, 512, 513, 600):
        for K in (1, 16, 64, 100, 256, 257, 512, 513, 1100):
            for reduce in (SUM, MEAN, MAX):
                assert route(Fo, K, reduce, 1) == _lib.DGRAD_GEMM_GATHER


def test_route_refuses_bad_arguments():
    route = _lib.load().ngnn_sage_dgrad_route
    assert route(0, 64, MEAN, 0) == _lib.E_ARG
    assert route(64, 0, MEAN, 0) == _lib.E_ARG
    assert route(64, 64, 3, 0) == _lib.E_ARG and route(64, 64, -1, 1) == _lib.E_ARG
    assert route(64, 2**31, MEAN, 0) == _lib.E_RANGE


def _edge_pairs():
    pairs = {(Fo, K) for Fo in (32, 33, 36, 37) for K in (256, 257, 300, 512, 513)}
    # the fused budget: 8 Fo K + 8 KiB <= 150 KiB  <=>  Fo K <= 18,176
    for Fo in (16, 32, 47, 64, 71, 100, 128, 142, 200, 256, 284, 300, 400, 511, 512):
        k0 = 18176 // Fo
        pairs |= {(Fo, K) for K in range(max(1, k0 - 3), k0 + 5)}
    # Fo around the fused kernel's row slot, Fo around K, K around the lowdim tile limit
    pairs |= {(Fo, K) for Fo in (510, 511, 512, 513, 514, 600) for K in (1, 8, 35, 36, 600, 700)}
    pairs |= {(Fo, K) for K in (8, 47, 64, 100, 256) for Fo in (K - 1, K, K + 1)}
    pairs |= {(Fo, K) for Fo in (1, 3, 4, 5, 47, 100, 200) for K in (511, 512, 513, 514, 1024)}
    # the lowdim LDS budget along K = 257..512 (ntw = 16)
    pairs |= {(Fo, K) for Fo in range(24, 44) for K in (257, 400, 512)}
    pairs |= {(Fo, K) for Fo in (60, 64, 68, 100, 104, 136, 140, 200, 280) for K in (128, 129, 256)}
    return sorted(p for p in pairs if p[0] > 0)


def test_route_agrees_with_the_entry_points():
    """With n_rows = 0 (and dummy non-null aligned pointers) an entry returns
    after its envelope check and before any launch: lowdim answers OK exactly
    where the query says LOWDIM (for Fo < K, sum and mean), and the fused
    entry refuses exactly Fo > 512."""
    lib = _lib.load()
    P = 256  # a non-null 16-B aligned address, never dereferenced
    pairs = _edge_pairs()
    assert len(pairs) >= 300
    n_low = 0
    for Fo, K in pairs:
        for reduce in (SUM, MEAN):
            want = lib.ngnn_sage_dgrad_route(Fo, K, reduce, 0)
            rc = lib.ngnn_sage_dgrad_lowdim(P, Fo, None, Fo, 1.0, P, P, K, Fo, K, P, P, 0, P, P, reduce,
                                            P, K, 0, P, 1 << 40, None)
            assert rc in (_lib.OK, _lib.E_SHAPE), (Fo, K, rc)
            if Fo < K:
                assert (rc == _lib.OK) == (want == _lib.DGRAD_LOWDIM), (Fo, K, reduce, rc, want)
                n_low += rc == _lib.OK
            else:
                assert want != _lib.DGRAD_LOWDIM
        for reduce in (SUM, MEAN, MAX):
            rc = lib.ngnn_sage_dgrad_fused(P, Fo, None, Fo, 1.0, P, P, Fo, K, P, P, 0, P, P, reduce,
                                           P, K, P, K, P, K, 0, None)
            assert rc == (_lib.E_SHAPE if Fo > FD_MAXF else _lib.OK), (Fo, K, reduce, rc)
    assert 0 < n_low < 2 * len(pairs)
