"""Restatement for the flip_label tests (a helper, not a test): the draw of
ngnn_flip_labels as include/ngnn.h states it, in numpy uint64 and float64,
written from the header and not from ngnn/noise.py; the statistics the tests
hold both this draw and the reference's own labels to; the fixture cases."""
import numpy as np

_U = np.uint64
LABEL_SALT = _U(0xA0761D6478BD642F)
TWO32 = 1 << 32

# name -> (noise_type, C, prob): tests/golden/label_noise.npz (make_golden_label_noise.py)
CASES = {
    "sym_c47": ("sym", 47, 0.3),
    "rand_pair_c10": ("rand_pair", 10, 0.45),
    "next_pair_c7": ("next_pair", 7, 0.45),
    "aim_pair_c10": ("aim_pair", 10, 0.2),
    "aim_pair_c4": ("aim_pair", 4, 0.2),
}
N_LABELS, N_FIXTURE = 200000, 20000


def case_labels(C: int) -> np.ndarray:
    return np.random.RandomState(5).randint(0, C, N_LABELS)


def mix64(z):
    """The sampler's mixer (ngnn_sample_dev.h), on uint64 arrays, modulo 2^64."""
    with np.errstate(over="ignore"):
        z = np.asarray(z, dtype=_U) + _U(0x9E3779B97F4A7C15)
        z = (z ^ (z >> _U(30))) * _U(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> _U(27))) * _U(0x94D049BB133111EB)
        return z ^ (z >> _U(31))


def thresholds_ref(M) -> np.ndarray:
    """T uint64 [C, C], row by row: below the row's last non-zero class jl the
    float64 cumulative sum scaled by 2^32, floored and capped at 2^32 - 1;
    from jl on 2^32, which no 32-bit draw reaches."""
    M = np.asarray(M, dtype=np.float64)
    C = M.shape[0]
    T = np.empty((C, C), dtype=_U)
    for l in range(C):
        cs = np.cumsum(M[l])
        jl = int(np.nonzero(M[l] > 0)[0][-1])
        for k in range(C):
            T[l, k] = TWO32 if k >= jl else min(int(np.floor(cs[k] * TWO32)), TWO32 - 1)
    return T


def draws(n: int, seed: int, i0: int = 0) -> np.ndarray:
    """r of nodes i0 .. i0 + n - 1, uint64 below 2^32."""
    with np.errstate(over="ignore"):
        i = np.arange(n, dtype=_U) + _U(i0)
        return mix64(_U(seed & 0xFFFFFFFFFFFFFFFF) ^ mix64(i + LABEL_SALT)) >> _U(32)


def flip_labels_ref(y, M, seed: int, i0: int = 0, chunk: int = 1 << 17):
    """(out, bad) of ngnn_flip_labels on a numpy int64 vector: a label in
    [0, C) becomes the number of thresholds of its row at or below its draw;
    any other label is copied and counted."""
    y = np.asarray(y, dtype=np.int64)
    C = np.asarray(M).shape[0]
    T = thresholds_ref(M)
    out = y.copy()
    r = draws(y.size, seed, i0)
    good = (y >= 0) & (y < C)
    for a in range(0, y.size, chunk):
        g = np.nonzero(good[a:a + chunk])[0] + a
        out[g] = (T[y[g]] <= r[g, None]).sum(axis=1)
    return out, int((~good).sum())


def count_matrix(y, out, C: int) -> np.ndarray:
    """K[l][j]: nodes with clean label l and noisy label j, labels outside
    [0, C) left out."""
    y, out = np.asarray(y, dtype=np.int64), np.asarray(out, dtype=np.int64)
    good = (y >= 0) & (y < C)
    return np.bincount(y[good] * C + out[good], minlength=C * C).reshape(C, C)


def flip_statistics(K, M):
    """(p, z, zero_hits) of a count matrix K against the transition matrix M
    read by ROWS: the chi-square tail p of X^2 = sum over cells with M > 0 of
    (K - n_l M)^2 / (n_l M) at sum_l (nnz_l - 1) degrees of freedom; z, the
    kept-label count trace(K) against sum_l n_l M[l][l] in standard deviations
    of that sum of binomials; the count on cells with M == 0."""
    from scipy.stats import chi2
    K, M = np.asarray(K, dtype=np.float64), np.asarray(M, dtype=np.float64)
    n_l = K.sum(axis=1, keepdims=True)
    pos = M > 0
    E = n_l * M
    x2 = float((((K - E) ** 2)[pos] / E[pos]).sum())
    dof = int((pos.sum(axis=1) - 1).sum())
    p = float(chi2.sf(x2, dof))
    d = np.diag(M)
    z = float((np.trace(K) - (n_l[:, 0] * d).sum()) / np.sqrt((n_l[:, 0] * d * (1 - d)).sum()))
    return p, z, int(K[~pos].sum())


def holds(p, z, zero_hits) -> bool:
    return p >= 0.01 and abs(z) <= 3 and zero_hits == 0
