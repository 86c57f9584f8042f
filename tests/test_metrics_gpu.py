"""ngnn.metrics on the device against the reference's lines restated on the
CPU (tests/metrics_ref.py).  Every comparison is exact: integer counts, and
fp64 sums of the same fp32 values in the same order.

Step kernel: C in {1, 2, 47, 70, 129} x B in {1, 63, 64, 65, 1025} x ld in
{C, C + 1, C + 3} (a column slice of a wider buffer, so rows are only 4-byte
aligned, 2-byte for bf16) x {fp32, bf16}; logits of integers in [-3, 3]
(nearly every row has tied maxima) and of bf16 randn, the hand-written rows
of the tie rule scattered among them; valid labels, ignore_index rows and the
labels C, -1 and 2^40."""
import copy
import ctypes

import pytest
import torch

import metrics_ref as R
import ngnn
from ngnn import _lib, metrics

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
IGNORE = -100


def _logits(kind, B, C, ld, dtype, gen):
    """[B, C] logits as a column slice of a [B, ld] buffer; what lies beyond
    column C is huge, so a kernel reading past a row's end would answer C."""
    buf = torch.full((B, ld), 1e30)
    if kind == "ints":
        vals = torch.randint(-3, 4, (B, C), generator=gen).float()
    else:
        vals = torch.randn(B, C, generator=gen).bfloat16().float()
    if C >= 4 and B >= 63:
        hand = R.hand_rows(C)
        for k in range(hand.size(0)):
            vals[(11 * k + 5) % B] = hand[k]
    buf[:, :C] = vals
    return buf.to(dtype).to(DEV)[:, :C]


def _labels(out_cpu, B, C, gen):
    """Half the rows get their argmax (so `correct` is far from 0), the rest
    a random class; then ignore_index rows and the labels C, -1 and 2^40."""
    y = torch.randint(0, C, (B,), generator=gen)
    am = R.argmax_rows(out_cpu)
    half = torch.rand(B, generator=gen) < 0.5
    y[half] = am[half]
    if B >= 63:
        y[3::17] = IGNORE
        y[7], y[20], y[41] = C, -1, 1 << 40
    return y


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("C", [1, 2, 47, 70, 129])
def test_epoch_meter_matches_the_reference_lines(C, dtype):
    gen = torch.Generator().manual_seed(1000 + C)
    names = ("loss_1", "loss_2", "pure_ratio_1", "pure_ratio_2")
    for B in (1, 63, 64, 65, 1025):
        for ld in (C, C + 1, C + 3):
            meter = metrics.EpochMeter(DEV, names=names)
            want = [0, 0, 0]
            fed = {n: [] for n in names}
            for u in range(5):
                if u == 4:  # four updates, the result, then a reset and one more
                    r = meter.result()
                    assert (r["steps"], r["rows"], r["correct"], r["bad_labels"]) == (4, *want), (B, ld)
                    for n in names:
                        assert r["sums"][n] == R.running_sum(fed[n]), (B, ld, n)
                        assert r["means"][n] == R.running_sum(fed[n]) / 4
                    assert want[0] > 0 and meter.accuracy() == want[1] / want[0]
                    assert meter.accuracy(12345) == want[1] / 12345
                    meter.reset()
                    want, fed = [0, 0, 0], {n: [] for n in names}
                out = _logits("ints" if u % 2 == 0 else "randn", B, C, ld, dtype, gen)
                assert out.stride(0) == ld or B == 1
                y = _labels(out.cpu(), B, C, gen)
                # rows past batch_size are there but not read: the step's whole output, no slice
                bs = B if u != 1 else max(B - 2, 0)
                scal = [(torch.randn((), generator=gen) * 10 ** (u - 1)).to(DEV) for _ in names]
                if u == 2:
                    scal[1] = None
                if u == 3:
                    scal = scal[:2]
                yd = y.to(DEV).view(-1, 1) if u == 0 else y.to(DEV)
                assert meter.update(out, yd, *scal, batch_size=None if bs == B else bs, ignore_index=IGNORE) is None
                for k, v in enumerate(R.step_counts(out, y, bs, IGNORE)):
                    want[k] += v
                for n, s in zip(names, scal):
                    if s is not None:
                        fed[n].append(s.cpu())
            r = meter.result()
            assert (r["steps"], r["rows"], r["correct"], r["bad_labels"]) == (1, *want), (B, ld)
            for n in names:
                assert r["sums"][n] == R.running_sum(fed[n])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_hand_written_rows_on_the_device(dtype):
    """The tie rule itself, through pred: every hand-written row alone and
    widened, at the three row alignments."""
    for C in (4, 5, 47):
        for ld in (C, C + 1, C + 3):
            buf = torch.full((6, ld), 1e30)
            buf[:, :C] = R.hand_rows(C)
            out = buf.to(dtype).to(DEV)[:, :C]
            res = metrics.split_accuracy(out, torch.tensor(R.HAND_ARGMAX, device=DEV), return_pred=True)
            assert res.pred["all"].tolist() == R.HAND_ARGMAX, (C, ld)
            assert res.accuracy["all"] == 1.0 and res.counts["all"] == (6, 6, 0, 0)


def test_empty_batch_advances_steps_and_sums():
    meter = metrics.EpochMeter(DEV)
    loss = torch.tensor(0.75, device=DEV)
    meter.update(torch.zeros(0, 47, device=DEV), torch.zeros(0, dtype=torch.int64, device=DEV), loss)
    meter.update(torch.randn(5, 47, device=DEV), torch.zeros(5, dtype=torch.int64, device=DEV), loss, batch_size=0)
    r = meter.result()
    assert (r["steps"], r["rows"], r["correct"], r["bad_labels"]) == (2, 0, 0, 0)
    assert r["sums"]["loss"] == 1.5 and r["means"]["loss"] == 0.75
    assert meter.accuracy() != meter.accuracy()  # (0 / 0)
    with pytest.raises(RuntimeError):
        meter.update(torch.zeros(4, 3), torch.zeros(4, dtype=torch.int64, device=DEV))
    with pytest.raises(RuntimeError):
        meter.update(torch.zeros(4, 3, device=DEV), torch.zeros(4, dtype=torch.int64))
    with pytest.raises(TypeError):
        meter.update(torch.zeros(4, 3, device=DEV), torch.zeros(4, dtype=torch.int64, device=DEV), 0.5)


def test_update_captured_in_a_graph_of_its_own():
    B, C, gen = 65, 47, torch.Generator().manual_seed(7)
    batches = []
    for k in range(4):
        out = _logits("ints", B, C, C + 1, torch.float32, gen)
        batches.append((out, _labels(out.cpu(), B, C, gen), torch.randn((), generator=gen)))
    s_out = torch.zeros(B, C + 1, device=DEV)[:, :C]
    s_y = torch.zeros(B, dtype=torch.int64, device=DEV)
    s_loss = torch.zeros((), device=DEV)
    meter = metrics.EpochMeter(DEV)

    def load(k):
        s_out.copy_(batches[k][0])
        s_y.copy_(batches[k][1])
        s_loss.copy_(batches[k][2])

    load(0)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        meter.update(s_out, s_y, s_loss)  # (warm-up: the library is loaded outside the capture)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    meter.reset()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        meter.update(s_out, s_y, s_loss)
    want = [0, 0, 0]
    for k in (1, 2, 3):
        load(k)
        g.replay()
        for i, v in enumerate(R.step_counts(batches[k][0], batches[k][1], B, IGNORE)):
            want[i] += v
    r = meter.result()
    assert (r["steps"], r["rows"], r["correct"], r["bad_labels"]) == (3, *want)
    assert r["sums"]["loss"] == R.running_sum(b[2] for b in batches[1:])


def test_update_makes_no_host_sync():
    """update() under torch's sync debug mode "error".  Whether this torch
    build honours the mode is checked once with .item(); where it does not,
    update() has still run under it, and the test says so by skipping."""
    out = torch.randn(64, 47, device=DEV)
    y = torch.randint(0, 47, (64,), device=DEV)
    loss = torch.tensor(1.25, device=DEV)
    meter = metrics.EpochMeter(DEV)
    meter.update(out, y, loss)  # (first use: loads the library)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            loss.item()
            honoured = False
        except RuntimeError:
            honoured = True
        meter.update(out, y, loss)
        meter.update(out.bfloat16()[:, :46], y.view(-1, 1), loss, batch_size=60)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert meter.result()["steps"] == 3
    if not honoured:
        pytest.skip("this torch build does not raise on .item() under set_sync_debug_mode('error'): "
                    "update() ran under the mode, but the mode proves nothing here")


# ------------------------------------------------------------ split_accuracy
N_BIG, C_BIG = 70_001, 47


@pytest.fixture(scope="module")
def big():
    """N = 70,001, C = 47 logits and labels inside larger allocations whose
    padding rows hold a huge value in column 0 and the label 0: a kernel that
    read the row of a bad id (-1, N, N + 1) would count it evaluated and
    correct."""
    gen = torch.Generator().manual_seed(3)
    N, C, pad = N_BIG, C_BIG, 2
    vals = torch.randint(-3, 4, (N, C), generator=gen).float()
    vals[1000:1006] = R.hand_rows(C)
    y = torch.randint(0, C, (N,), generator=gen)
    am = R.argmax_rows(vals)
    half = torch.rand(N, generator=gen) < 0.5
    y[half] = am[half]
    y[5::101] = IGNORE
    buf = torch.zeros(N + 2 * pad, C)
    buf[:, 0] = 1e30
    buf[pad:N + pad] = vals
    ybuf = torch.zeros(N + 2 * pad, dtype=torch.int64)
    ybuf[pad:N + pad] = y
    a = torch.randint(0, N, (30_000,), generator=gen)
    lists = {"train": a,
             "valid": torch.cat([a[:5_000], torch.arange(100).repeat(3), torch.tensor([1000, 1001, 1002, 1003])]),
             "none": torch.zeros(0, dtype=torch.int64),
             "test": torch.arange(N - 1, -1, -1)}
    return dict(out=buf.to(DEV)[pad:N + pad], y=ybuf.to(DEV)[pad:N + pad], out_cpu=vals, y_cpu=y, lists=lists,
                am=am)


def _raw_split(out, y, rows, bounds, want_pred=False, want_conf=False):
    """ngnn_split_accuracy at the C ABI: (rc, counts, pred, confusion)."""
    N, C = out.shape
    S, M = len(bounds) - 1, bounds[-1]
    counts = torch.full((S, 4), -7, dtype=torch.int64, device=DEV)  # (overwritten, not added to)
    pred = torch.full((M,), -7, dtype=torch.int64, device=DEV) if want_pred else None
    conf = torch.full((C, C), -7, dtype=torch.int64, device=DEV) if want_conf else None
    rc = _lib.load().ngnn_split_accuracy(out.data_ptr(), out.stride(0), _lib.BF16 if out.dtype == torch.bfloat16
                                         else _lib.F32, N, C, y.data_ptr(), IGNORE, _lib.ptr(rows), M, S,
                                         (ctypes.c_int64 * (S + 1))(*bounds), counts.data_ptr(), _lib.ptr(pred),
                                         _lib.ptr(conf), _lib.stream_handle(DEV))
    torch.cuda.synchronize()
    return rc, counts.cpu(), None if pred is None else pred.cpu(), None if conf is None else conf.cpu()


def test_split_accuracy_overlapping_lists(big):
    lists = big["lists"]
    res = metrics.split_accuracy(big["out"], big["y"], lists, return_pred=True, confusion=True)
    want = R.split_accuracy(big["out_cpu"], big["y_cpu"], lists, IGNORE)
    assert list(res.accuracy) == list(lists)
    for k in lists:
        if lists[k].numel():
            assert res.accuracy[k] == want[k], k
        else:
            assert res.accuracy[k] != res.accuracy[k]
        assert tuple(res.counts[k]) == R.split_counts(big["out_cpu"], big["y_cpu"], lists[k], IGNORE), k
        assert torch.equal(res.pred[k].cpu(), big["am"][lists[k]]), k
    assert res.pred["valid"][-4:].tolist() == R.HAND_ARGMAX[:4]
    every = torch.cat(list(lists.values()))
    assert torch.equal(res.confusion.cpu(), R.confusion(big["out_cpu"], big["y_cpu"], every, IGNORE))
    # the plain call returns the accuracies alone; the list is built once per dict of tensors
    kept = len(metrics._splits)
    rows_before = next(reversed(metrics._splits.values()))[2]
    plain = metrics.split_accuracy(big["out"], big["y"], lists)
    assert isinstance(plain, dict) and all(plain[k] == res.accuracy[k] for k in lists if k != "none")
    assert len(metrics._splits) == kept and next(reversed(metrics._splits.values()))[2] is rows_before
    # ... and again after one of them changed in place
    lists["train"][0] = (int(lists["train"][0]) + 1) % N_BIG
    got = metrics.split_accuracy(big["out"], big["y"], lists)
    assert next(reversed(metrics._splits.values()))[2] is not rows_before
    assert got["train"] == R.split_accuracy(big["out_cpu"], big["y_cpu"], lists, IGNORE)["train"]


def test_split_accuracy_without_a_list(big):
    res = metrics.split_accuracy(big["out"], big["y"].view(-1, 1), return_pred=True, confusion=True)
    ev, ok, bad, ign = R.split_counts(big["out_cpu"], big["y_cpu"], torch.arange(N_BIG), IGNORE)
    assert tuple(res.counts["all"]) == (ev, ok, 0, ign) and bad == 0 and ign > 0
    assert res.accuracy == {"all": ok / N_BIG}
    assert torch.equal(res.pred["all"].cpu(), big["am"])
    assert torch.equal(res.confusion.cpu(), R.confusion(big["out_cpu"], big["y_cpu"], torch.arange(N_BIG), IGNORE))
    assert int(res.confusion.sum()) == ev


def test_split_accuracy_bad_ids_are_counted_and_never_read(big):
    N = N_BIG
    gen = torch.Generator().manual_seed(9)
    a = torch.cat([torch.tensor([-1, N, N + 1, 0, N - 1]), torch.randint(0, N, (2_000,), generator=gen)])
    b = torch.cat([torch.randint(0, N, (999,), generator=gen), torch.tensor([N + 1, -1])])
    c = torch.randint(0, N, (500,), generator=gen)
    rows = torch.cat([a, b, c])
    bounds = [0, a.numel(), a.numel() + b.numel(), rows.numel()]
    for want_pred in (False, True):
        rc, counts, pred, conf = _raw_split(big["out"], big["y"], rows.to(DEV), bounds, want_pred, True)
        assert rc == 0
        for s, idx in enumerate((a, b, c)):
            assert tuple(counts[s].tolist()) == R.split_counts(big["out_cpu"], big["y_cpu"], idx, IGNORE), s
        assert counts[:, 2].tolist() == [3, 2, 0]
        assert torch.equal(conf, R.confusion(big["out_cpu"], big["y_cpu"], rows, IGNORE))
        if want_pred:
            assert torch.equal(pred, R.pred_rows(big["out_cpu"], rows))
            assert pred[:3].tolist() == [-1, -1, -1]
    with pytest.raises(ValueError, match="'first'"):
        metrics.split_accuracy(big["out"], big["y"], {"first": a, "second": c})
    with pytest.raises(ValueError, match="'second'"):
        metrics.split_accuracy(big["out"], big["y"], {"first": c, "second": b})
    # a label outside [0, C) that is not ignore_index is bad too
    y2 = big["y"].clone()
    y2[c[0]] = C_BIG
    with pytest.raises(ValueError, match="'first'"):
        metrics.split_accuracy(big["out"], y2, {"first": c})
    # nothing to evaluate: success with the counts zeroed
    rc, counts, _, _ = _raw_split(big["out"], big["y"], torch.zeros(0, dtype=torch.int64, device=DEV), [0, 0, 0])
    assert rc == 0 and counts.tolist() == [[0] * 4] * 2


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("C", [128, 129])
def test_confusion_at_and_beyond_the_class_limit(C, dtype):
    gen = torch.Generator().manual_seed(C)
    N, ld = 5_003, C + 1
    out = _logits("randn" if dtype == torch.bfloat16 else "ints", N, C, ld, dtype, gen)
    y = _labels(out.cpu(), N, C, gen)
    y[(y < 0) | (y >= C)] = IGNORE
    idx = {"a": torch.randint(0, N, (3_000,), generator=gen), "b": torch.arange(N)}
    want = R.split_accuracy(out, y, idx, IGNORE)
    assert metrics.split_accuracy(out, y.to(DEV), idx) == want
    assert metrics.confusion_max_classes() == 128
    if C <= 128:
        res = metrics.split_accuracy(out, y.to(DEV), idx, confusion=True)
        assert res.accuracy == want
        assert torch.equal(res.confusion.cpu(), R.confusion(out, y, torch.cat(list(idx.values())), IGNORE))
    else:
        with pytest.raises(ValueError):
            metrics.split_accuracy(out, y.to(DEV), idx, confusion=True)
        rows = torch.cat(list(idx.values())).to(DEV)
        conf = torch.zeros(C, C, dtype=torch.int64, device=DEV)
        counts = torch.zeros(2, 4, dtype=torch.int64, device=DEV)
        rc = _lib.load().ngnn_split_accuracy(out.data_ptr(), ld, _lib.BF16 if dtype == torch.bfloat16 else _lib.F32,
                                             N, C, y.to(DEV).data_ptr(), IGNORE, rows.data_ptr(), rows.numel(), 2,
                                             (ctypes.c_int64 * 3)(0, 3_000, rows.numel()), counts.data_ptr(), None,
                                             conf.data_ptr(), _lib.stream_handle(DEV))
        assert rc == _lib.E_SHAPE


# -------------------------------------------------------------- co-teaching
def test_coteaching_step_exposes_both_logits():
    """step.out1 / step.out2 after a replay and after an eager short block
    are the two models' logits on that block (against the same models run
    eagerly on it, at the 1e-5 of tests/test_coteaching_gpu.py's loss bar),
    and a meter fed from them gives the reference's total_correct_1/2,
    total_loss_1/2 and total_ratio_1/2 sums."""
    from ngnn.graphs import GraphedCoTeachingStep, slot_size
    from ngnn.loader import sample_block, synthetic_graph
    from ngnn.losses import CTLoss
    from ngnn.optim import Adam
    g = synthetic_graph("ogbn-products", DEV, seed=1, scale=0.01)
    torch.manual_seed(3)
    m1 = ngnn.SAGE(100, 64, 47, 2, dropout=0.0).to(DEV).train()
    m2 = ngnn.SAGE(100, 64, 47, 2, dropout=0.0).to(DEV).train()
    n_cap, e_cap = slot_size(256, [5, 4])
    step = GraphedCoTeachingStep(m1, Adam(m1.parameters()), m2, Adam(m2.parameters()), CTLoss(DEV), 256,
                                 n_cap, e_cap, 100, DEV,
                                 noise_or_not=torch.ones(g.num_nodes, dtype=torch.bool, device=DEV))
    assert step.out1 is None and step.out2 is None
    full = sample_block(g, g.train_idx[:256], [5, 4], seed=1)
    short = sample_block(g, g.train_idx[256:356], [5, 4], seed=2)
    step.capture(full.x, full.edge_index, g.y[full.n_id], full.n_id, 0.25)  # (restores both models)
    names = ("loss_1", "loss_2", "pure_ratio_1", "pure_ratio_2")
    meters = [metrics.EpochMeter(DEV, names=names[0::2]), metrics.EpochMeter(DEV, names=names[1::2])]
    want = [[0, 0, 0], [0, 0, 0]]
    fed = {n: [] for n in names}
    for blk, bs in ((full, 256), (short, 100)):
        before = []
        for m in (m1, m2):  # the models as they are before this step
            ref = ngnn.SAGE(100, 64, 47, 2, dropout=0.0).to(DEV).train()
            ref.load_state_dict(copy.deepcopy(m.state_dict()))
            before.append(ref)
        yb = g.y[blk.n_id]
        res = step(blk.x, blk.edge_index, yb, blk.n_id, 0.25, batch_size=bs)
        with torch.no_grad():
            x = blk.x.materialize() if hasattr(blk.x, "materialize") else blk.x
            eager = [m(x, blk.edge_index) for m in before]
        for k, (got, ref) in enumerate(zip((step.out1, step.out2), eager)):
            assert not got.requires_grad and got.size(0) >= bs
            torch.testing.assert_close(got[:bs], ref[:bs], rtol=0, atol=1e-5)
            meters[k].update(got, yb, res[k], res[2 + k], batch_size=bs)
            for i, v in enumerate(R.step_counts(got, yb, bs, IGNORE)):
                want[k][i] += v
            fed[names[k]].append(res[k].cpu())
            fed[names[2 + k]].append(res[2 + k].cpu())
    for k, meter in enumerate(meters):
        r = meter.result()
        assert (r["steps"], r["rows"], r["correct"], r["bad_labels"]) == (2, *want[k])
        assert r["rows"] == 356
        assert r["sums"][names[k]] == R.running_sum(fed[names[k]])
        assert r["sums"][names[2 + k]] == R.running_sum(fed[names[2 + k]])
