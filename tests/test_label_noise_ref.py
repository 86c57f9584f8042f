"""flip_label on the CPU: the transition matrix against the reference's
(tests/golden/label_noise.npz), the product code's threshold table against
the restatement's, and the statistics of the restated draw -- row l of the
matrix, not column l, is the distribution of the new label -- held to the
same conditions as the reference's own 20,000 labels, with controls that
must fail them.

Measured on the fixture's inputs (200,000 labels, seeds 0, 1, 2; the four
cases the reference can build): the restated draw has p between 0.23 and
0.96 and |z| <= 2.09, the reference's own labels p between 0.14 and 0.47 and
|z| <= 1.85; against the matrix built with prob + 0.01 |z| is 7.4 to 13.0,
against the transpose p is 0 and 31,671 to 89,935 labels land on zero cells.

The fifth case, aim_pair with 4 classes, is one the reference cannot build:
its fixed pairs name classes 0..5, so it raises an IndexError while it fills
the matrix (the fixture records that).  Here it is a ValueError, as every
aim_pair below 6 classes."""
import os

import numpy as np
import pytest

import label_noise_ref as R
from ngnn import noise

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "label_noise.npz")
BUILDABLE = [k for k in R.CASES if k != "aim_pair_c4"]
ASYMMETRIC = [k for k in BUILDABLE if R.CASES[k][0] != "sym"]
SEEDS = (0, 1, 2)


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def flips(golden):
    """name -> (labels, matrix, {seed: count matrix of the restated draw}), computed once."""
    out = {}
    for name in BUILDABLE:
        C = R.CASES[name][1]
        y, M = R.case_labels(C), golden[name + "/noise_mat"]
        out[name] = (y, M, {s: R.count_matrix(y, R.flip_labels_ref(y, M, s)[0], C) for s in SEEDS})
    return out


# ------------------------------------------------------------ the matrix

def test_fixture_holds_all_five_cases(golden):
    assert os.path.getsize(GOLDEN) < 200 * 1024
    for name, (_, C, _) in R.CASES.items():
        assert golden[name + "/seed"].shape == ()
        if name in BUILDABLE:
            assert golden[name + "/noise_mat"].shape == (C, C) and golden[name + "/noise_mat"].dtype == np.float64
            assert golden[name + "/noisy"].shape == (R.N_FIXTURE,) and golden[name + "/noisy"].dtype == np.uint8
        else:
            assert str(golden[name + "/reference_raised"]) == "IndexError"


@pytest.mark.parametrize("name", list(R.CASES))
def test_noise_matrix_is_bitwise_the_references(golden, name):
    noise_type, C, prob = R.CASES[name]
    state = np.random.get_state()
    try:
        np.random.seed(int(golden[name + "/seed"]))
        if name in BUILDABLE:
            assert np.array_equal(noise.noise_matrix(C, noise_type, prob), golden[name + "/noise_mat"])
        else:  # the reference raised an IndexError (recorded in the fixture)
            with pytest.raises(ValueError):
                noise.noise_matrix(C, noise_type, prob)
    finally:
        np.random.set_state(state)


@pytest.mark.parametrize("noise_type", noise.NOISE_TYPES)
@pytest.mark.parametrize("C,prob", [(6, 0.2), (10, 0.45), (47, 0.3), (70, 0.1)])
def test_rows_and_columns_sum_to_one(noise_type, C, prob):
    M = noise.noise_matrix(C, noise_type, prob)
    assert M.shape == (C, C) and M.dtype == np.float64 and (M >= 0).all()
    np.testing.assert_allclose(M.sum(axis=1), 1.0, rtol=0, atol=1e-12)
    np.testing.assert_allclose(M.sum(axis=0), 1.0, rtol=0, atol=1e-12)


def test_value_errors():
    with pytest.raises(ValueError):
        noise.noise_matrix(10, "pair", 0.3)
    for C in (1, 2, 3, 4, 5):
        with pytest.raises(ValueError):
            noise.noise_matrix(C, "aim_pair", 0.2)
    assert noise.noise_matrix(6, "aim_pair", 0.2).shape == (6, 6)
    ok = np.full((3, 3), 1 / 3)
    assert noise._checked_matrix(ok, 3) is not None
    assert noise._checked_matrix(ok * (1 + 5e-7), 3) is not None
    for bad in (np.full((3, 4), 0.25), np.full((2, 2), 0.5), ok * 1.001, ok * (1 - 1e-5),
                np.array([[1.5, -0.5, 0], [0, 1, 0], [0, 0, 1.0]]), np.full((3, 3), np.nan)):
        with pytest.raises(ValueError):
            noise._checked_matrix(bad, 3)


# ------------------------------------------------------------ thresholds

def _matrices(golden):
    ms = [golden[name + "/noise_mat"] for name in BUILDABLE]
    ms.append(np.array([[0.5, 0.5, 0.0], [0.0, 0.25, 0.75], [1.0, 0.0, 0.0]]))  # zero last columns, a one-class row
    ms.append(np.eye(5))
    ms.append(noise.noise_matrix(128, "sym", 0.3))
    rs = np.random.RandomState(9).rand(33, 33) ** 8
    ms.append(rs / rs.sum(axis=1, keepdims=True))
    return ms


def test_threshold_table_is_the_restatements(golden):
    for M in _matrices(golden):
        C = M.shape[0]
        thr, last = noise.threshold_table(M)
        assert thr.shape == (C, C) and thr.dtype == np.uint32 and last.shape == (C,) and last.dtype == np.int32
        T = R.thresholds_ref(M)
        k = np.arange(C)[None, :]
        # the product's storage, read as the header says: thr below last, 2^32 from last on
        full = np.where(k < last[:, None], thr.astype(np.uint64), np.uint64(R.TWO32))
        assert np.array_equal(full, T)
        assert (np.diff(T.astype(np.int64), axis=1) >= 0).all()
        for l in range(C):
            jl = int(np.nonzero(M[l] > 0)[0][-1])
            assert last[l] == jl
            assert (T[l, jl:] == R.TWO32).all()       # unreachable: r < 2^32
            assert (T[l, :jl] < R.TWO32).all()


# ------------------------------------------------------------ statistics

@pytest.mark.parametrize("name", BUILDABLE)
def test_restated_draw_follows_the_rows(flips, name):
    _, M, by_seed = flips[name]
    for seed, K in by_seed.items():
        p, z, zero_hits = R.flip_statistics(K, M)
        print(f"{name} seed {seed}: p {p:.4f} z {z:+.3f} zero-cell hits {zero_hits}")
        assert p >= 0.01 and abs(z) <= 3 and zero_hits == 0
        assert K.sum() == R.N_LABELS


@pytest.mark.parametrize("name", BUILDABLE)
def test_reference_labels_pass_the_same_conditions(golden, name):
    C = R.CASES[name][1]
    y, M = R.case_labels(C)[:R.N_FIXTURE], golden[name + "/noise_mat"]
    p, z, zero_hits = R.flip_statistics(R.count_matrix(y, golden[name + "/noisy"], C), M)
    print(f"{name} reference: p {p:.4f} z {z:+.3f} zero-cell hits {zero_hits}")
    assert p >= 0.01 and abs(z) <= 3 and zero_hits == 0


@pytest.mark.parametrize("name", BUILDABLE)
def test_control_a_shifted_prob_fails(golden, flips, name):
    noise_type, C, prob = R.CASES[name]
    state = np.random.get_state()
    try:
        np.random.seed(int(golden[name + "/seed"]))
        shifted = noise.noise_matrix(C, noise_type, prob + 0.01)
    finally:
        np.random.set_state(state)
    assert np.array_equal(shifted > 0, flips[name][1] > 0)  # the same pairs, another rate
    for seed, K in flips[name][2].items():
        p, z, zero_hits = R.flip_statistics(K, shifted)
        print(f"{name} seed {seed} against prob + 0.01: p {p:.2e} z {z:+.2f}")
        assert abs(z) > 3 and not R.holds(p, z, zero_hits)


@pytest.mark.parametrize("name", ASYMMETRIC)
def test_control_the_transposed_matrix_fails(flips, name):
    _, M, by_seed = flips[name]
    assert not np.array_equal(M, M.T)
    for seed, K in by_seed.items():
        p, z, zero_hits = R.flip_statistics(K, M.T)
        print(f"{name} seed {seed} against the transpose: p {p:.2e} zero-cell hits {zero_hits}")
        assert p < 0.01 and zero_hits > 0 and not R.holds(p, z, zero_hits)


def test_next_pair_moves_to_the_next_class_only(flips):
    y, M, _ = flips["next_pair_c7"]
    for seed in SEEDS:
        out, bad = R.flip_labels_ref(y, M, seed)
        assert bad == 0 and ((out == y) | (out == (y + 1) % 7)).all()
        assert (out != y).any() and (out == y).any()


def test_restatement_shards_and_bad_labels():
    M = noise.noise_matrix(10, "sym", 0.3)
    y = R.case_labels(10)[:5000].copy()
    y[[3, 77, 4000]] = (-1, 10, 1 << 40)
    whole, bad = R.flip_labels_ref(y, M, 11)
    assert bad == 3 and whole[3] == -1 and whole[77] == 10 and whole[4000] == 1 << 40
    part, _ = R.flip_labels_ref(y[1000:3000], M, 11, i0=1000)
    assert np.array_equal(part, whole[1000:3000])
    assert not np.array_equal(R.flip_labels_ref(y, M, 12)[0], whole)
