"""flip_label on the device, bit for bit against the numpy restatement of its
draw (tests/label_noise_ref.py): the labels, noise_or_not and counts (a
bincount of the restatement's output) over sizes around a wave, the largest
LDS footprint, a second trip of every workgroup, label layouts, bad labels,
index_offset, seeds, out=, the path without statistics, a hand-written
matrix, and one loader batch carrying the flipped labels."""
import numpy as np
import pytest
import torch

import label_noise_ref as R
from ngnn import noise
from ngnn.loader import NeighborLoader, synthetic_graph

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _labels(N, C, seed=5):
    return np.random.RandomState(seed).randint(0, C, N).astype(np.int64)


def _check(y, C, M, seed, i0=0):
    """One flip with statistics against the restatement; returns the device labels."""
    yd = torch.from_numpy(y).to(DEV)
    before = noise.label_noise_bad_labels(DEV, reset=True)
    assert before >= 0
    out, mat, st = noise.flip_label(yd, C, noise_mat=M, seed=seed, index_offset=i0, return_stats=True)
    want, bad = R.flip_labels_ref(y, M, seed, i0)
    assert mat is M and out.dtype == torch.int64 and out.shape == (y.size,) and out.device == yd.device
    assert np.array_equal(out.cpu().numpy(), want)
    assert st.noise_or_not.dtype == torch.bool and np.array_equal(st.noise_or_not.cpu().numpy(), want == y)
    assert st.counts.dtype == torch.int64 and np.array_equal(st.counts.cpu().numpy(), R.count_matrix(y, want, C))
    assert int(st.counts.sum()) == y.size - bad
    assert noise.label_noise_bad_labels(DEV, reset=True) == bad and int(st.bad) == 0
    return out


@pytest.mark.parametrize("C", [2, 47])
def test_sizes_around_a_wave(C):
    M = noise.noise_matrix(C, "sym", 0.3)
    for N in (0, 1, 63, 64, 65, 257, 4099):
        _check(_labels(N, C), C, M, seed=7 + N)


def test_largest_lds_footprint():
    C = noise.max_classes()
    assert C >= 100
    rs = np.random.RandomState(3).rand(C, C) ** 4  # every cell non-zero, rows far from uniform
    _check(_labels(4099, C), C, rs / rs.sum(axis=1, keepdims=True), seed=21)
    _check(_labels(4099, C), C, noise.noise_matrix(C, "next_pair", 0.45), seed=22)


def test_every_workgroup_makes_a_second_trip():
    """The geometry include/ngnn.h documents: 1024-thread workgroups, one per
    compute unit at most, four nodes per thread and trip.  One whole trip of
    the full grid, then every workgroup starts a second one, the last of them
    on a ragged tail; every workgroup flushes its histogram."""
    cus = torch.cuda.get_device_properties(DEV).multi_processor_count
    per_pass = noise.BLOCK_THREADS * cus
    N = noise.NODES_PER_THREAD_TRIP * per_pass + per_pass - 37
    C = 47
    out = _check(_labels(N, C), C, noise.noise_matrix(C, "sym", 0.3), seed=5)
    assert out.numel() == N


def test_label_layouts_give_the_contiguous_result():
    C, N = 47, 4099
    y = torch.from_numpy(_labels(N, C)).to(DEV)
    want, M = noise.flip_label(y, C, "sym", 0.3, seed=9)
    col, _ = noise.flip_label(y.view(-1, 1), C, "sym", 0.3, seed=9)
    wide = torch.stack([y, y + 1], dim=1)  # [N, 2]: column 0 is a stride-2 view
    assert wide[:, 0].stride(0) == 2
    strided, _ = noise.flip_label(wide[:, 0], C, "sym", 0.3, seed=9)
    strided_col, _ = noise.flip_label(wide[:, :1], C, "sym", 0.3, seed=9)
    i32, _ = noise.flip_label(y.to(torch.int32), C, "sym", 0.3, seed=9)
    moved, _ = noise.flip_label(y.cpu(), C, "sym", 0.3, seed=9, device=DEV)
    for got in (col, strided, strided_col, i32, moved):
        assert got.shape == (N,) and got.device == y.device and torch.equal(got, want)
    assert np.array_equal(want.cpu().numpy(), R.flip_labels_ref(y.cpu().numpy(), M, 9)[0])


def test_bad_labels_are_copied_counted_and_left_out_of_counts():
    C, N = 47, 4099
    y = _labels(N, C)
    where = [0, 63, 64, 1000, 1023, 1024, N - 1]
    y[where] = [-1, C, 1 << 40, -(1 << 40), C + 1, -1, C]
    out = _check(y, C, noise.noise_matrix(C, "sym", 0.3), seed=13).cpu().numpy()
    assert np.array_equal(out[where], y[where])


def test_index_offset_shards_the_whole_flip():
    C, N = 10, 4099
    y = torch.from_numpy(_labels(N, C)).to(DEV)
    M = noise.noise_matrix(C, "sym", 0.3)
    whole, _ = noise.flip_label(y, C, noise_mat=M, seed=17)
    for a, b in ((0, 1), (1, 65), (1023, 2049), (4000, N)):
        part, _, st = noise.flip_label(y[a:b], C, noise_mat=M, seed=17, index_offset=a, return_stats=True)
        assert torch.equal(part, whole[a:b])
        assert torch.equal(st.noise_or_not, whole[a:b] == y[a:b])
    big = 1 << 40  # a global index far past 2^31
    far, _ = noise.flip_label(y[:257], C, noise_mat=M, seed=17, index_offset=big)
    assert np.array_equal(far.cpu().numpy(), R.flip_labels_ref(y[:257].cpu().numpy(), M, 17, big)[0])


def test_seeds_repeat_and_differ():
    C, N = 47, 4099
    y = torch.from_numpy(_labels(N, C)).to(DEV)
    a, _ = noise.flip_label(y, C, "sym", 0.3, seed=1)
    b, _ = noise.flip_label(y, C, "sym", 0.3, seed=1)
    c, _ = noise.flip_label(y, C, "sym", 0.3, seed=2)
    assert torch.equal(a, b) and not torch.equal(a, c)
    torch.manual_seed(123)
    d, _ = noise.flip_label(y, C, "sym", 0.3)
    e, _ = noise.flip_label(y, C, "sym", 0.3)
    torch.manual_seed(123)
    f, _ = noise.flip_label(y, C, "sym", 0.3)
    assert torch.equal(d, f) and not torch.equal(d, e)
    big, _ = noise.flip_label(y, C, "sym", 0.3, seed=(1 << 64) - 1)
    assert np.array_equal(big.cpu().numpy(),
                          R.flip_labels_ref(y.cpu().numpy(), noise.noise_matrix(C, "sym", 0.3), (1 << 64) - 1)[0])


def test_out_is_written_in_place():
    C, N = 47, 4099
    y = torch.from_numpy(_labels(N, C)).to(DEV)
    buf = torch.full((N,), -7, dtype=torch.int64, device=DEV)
    p = buf.data_ptr()
    got, M = noise.flip_label(y, C, "sym", 0.3, seed=1, out=buf)
    assert got is buf and buf.data_ptr() == p
    first = buf.clone()
    assert np.array_equal(first.cpu().numpy(), R.flip_labels_ref(y.cpu().numpy(), M, 1)[0])
    again, _ = noise.flip_label(y, C, "sym", 0.3, seed=2, out=buf)
    assert again is buf and buf.data_ptr() == p and not torch.equal(buf, first)
    assert np.array_equal(buf.cpu().numpy(), R.flip_labels_ref(y.cpu().numpy(), M, 2)[0])
    with pytest.raises(ValueError):
        noise.flip_label(y, C, "sym", 0.3, seed=1, out=y)
    both = torch.cat([y, y])
    with pytest.raises(ValueError):
        noise.flip_label(both[:N], C, "sym", 0.3, seed=1, out=both[1:N + 1])
    with pytest.raises(ValueError):
        noise.flip_label(y, C, "sym", 0.3, seed=1, out=buf[:-1])
    with pytest.raises(ValueError):
        noise.flip_label(y, C, "sym", 0.3, seed=1, out=buf.to(torch.int32))


def test_without_statistics_gives_the_same_labels():
    C, N = 47, 4099
    y = torch.from_numpy(_labels(N, C)).to(DEV)
    res = noise.flip_label(y, C, "rand_pair", 0.45, seed=3, return_stats=False)
    assert len(res) == 2
    M = res[1]
    full = noise.flip_label(y, C, noise_mat=M, seed=3, return_stats=True)
    assert len(full) == 3 and torch.equal(res[0], full[0])
    assert np.array_equal(res[0].cpu().numpy(), R.flip_labels_ref(y.cpu().numpy(), M, 3)[0])


def test_hand_written_matrix_never_draws_a_zero_class():
    M = np.array([[0.5, 0.5, 0.0],
                  [0.0, 0.25, 0.75],
                  [1.0, 0.0, 0.0]])
    y = _labels(4099, 3)
    out = _check(y, 3, M, seed=4).cpu().numpy()
    K = R.count_matrix(y, out, 3)
    assert (K[M == 0] == 0).all() and (K[M > 0] > 0).all()
    assert not (out[y == 0] == 2).any()
    yd = torch.from_numpy(y).to(DEV)
    for bad in (np.eye(4), M * 1.01, M - np.eye(3) * 0.75):
        with pytest.raises(ValueError):
            noise.flip_label(yd, 3, noise_mat=bad, seed=4)
    with pytest.raises(ValueError):
        noise.flip_label(yd, noise.max_classes() + 1, "sym", 0.3, seed=4)


def test_a_loader_batch_carries_the_flipped_labels():
    g = synthetic_graph("ogbn-arxiv", DEV, seed=4, scale=0.02)
    yhn, _ = noise.flip_label(g.y, 40, "sym", 0.3, seed=8)
    assert not torch.equal(yhn, g.y.view(-1))
    g.node_attrs["yhn"] = yhn
    batch = next(iter(NeighborLoader(g, g.train_idx, [10, 5], 128, shuffle=True, seed=3)))
    assert torch.equal(batch.yhn, yhn[batch.n_id.long()])
    assert torch.equal(batch.y.view(-1), g.y.view(-1)[batch.n_id.long()])
