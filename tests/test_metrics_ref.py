"""CPU checks of tests/metrics_ref.py, the reference lines the GPU tests of
ngnn.metrics compare against: the tie rule of its argmax on hand-written rows
(tied maxima, +-0, the first NaN, +-inf, a row of -inf), and how ignored,
out-of-range and repeated entries are counted."""
import pytest
import torch

import metrics_ref as R
from ngnn import metrics


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_tie_rule_on_hand_written_rows(dtype):
    assert R.HAND_ARGMAX == [1, 0, 0, 3, 0, 0]
    rows = torch.tensor(R.HAND_ROWS).to(dtype)
    assert R.argmax_rows(rows).tolist() == R.HAND_ARGMAX
    # widened with -inf columns (how the GPU tests scatter them among C-wide rows): the same answers
    for C in (4, 47, 129):
        assert R.argmax_rows(R.hand_rows(C, dtype)).tolist() == R.HAND_ARGMAX
    # one row at a time, too (no dependence on the batch)
    for row, want in zip(rows, R.HAND_ARGMAX):
        assert int(R.argmax_rows(row[None])[0]) == want


def test_step_counts_ignored_and_out_of_range_labels():
    out = torch.tensor([[0., 1, 0], [2, 1, 0], [0, 0, 3], [1, 1, 1], [0, 5, 0], [0, 0, 0], [9, 0, 0]])
    y = torch.tensor([1, 0, 1, -100, 3, -1, 1 << 40])
    # rows 0, 1 correct; row 2 wrong; row 3 ignored; rows 4, 5, 6 bad (C, -1, 2^40)
    assert R.step_counts(out, y) == (3, 2, 3)
    assert R.step_counts(out, y.view(-1, 1)) == (3, 2, 3)
    assert R.step_counts(out, y, batch_size=2) == (2, 2, 0)
    assert R.step_counts(out, y, batch_size=0) == (0, 0, 0)
    assert R.step_counts(out, y, ignore_index=-1) == (3, 2, 3)  # (-100 is bad now, -1 ignored)
    assert R.running_sum([torch.tensor(0.1), torch.tensor(0.2)]) == float(torch.tensor(0.1)) + float(torch.tensor(0.2))


def test_split_counts_repeats_bad_ids_and_ignored():
    out = torch.tensor([[0., 1], [1, 0], [0, 1], [1, 1]])
    y = torch.tensor([1, 1, -100, 0])
    idx = torch.tensor([0, 0, 1, 2, 3, 3, 3, -1, 4, 5])
    # 0 twice (correct), 1 (wrong), 2 ignored, 3 three times (tie -> 0, correct), three bad ids
    assert R.split_counts(out, y, idx) == (6, 5, 3, 1)
    assert R.pred_rows(out, idx).tolist() == [1, 1, 0, 1, 0, 0, 0, -1, -1, -1]
    assert R.confusion(out, y, idx).tolist() == [[3, 0], [1, 2]]
    y2 = torch.tensor([1, 2, -100, 0])  # a label C: bad, left out of evaluated and of the matrix
    assert R.split_counts(out, y2, idx) == (5, 5, 4, 1)
    assert R.confusion(out, y2, idx).tolist() == [[3, 0], [0, 2]]
    good = {"a": torch.tensor([0, 1]), "b": torch.tensor([3, 3, 0, 1]), "c": torch.zeros(0, dtype=torch.int64)}
    acc = R.split_accuracy(out, y, good)
    assert acc["a"] == 0.5 and acc["b"] == 0.75 and acc["c"] != acc["c"]
    # an ignored entry stays in the denominator, as in y_pred[idx] == y[idx]
    assert R.split_accuracy(out, y, {"d": torch.tensor([0, 2])})["d"] == 0.5


def test_helper_and_module_agree_on_the_layout():
    """The helper's tuples are in the order of the module's records."""
    assert metrics.SplitCounts._fields == ("evaluated", "correct", "bad", "ignored")
    assert metrics.SplitCounts(*R.split_counts(torch.zeros(2, 2), torch.tensor([0, 5]), torch.tensor([0, 1, 1]))) \
        == metrics.SplitCounts(evaluated=1, correct=1, bad=2, ignored=0)
    assert metrics.MAX_SCALARS == 4 and metrics.MAX_SEGMENTS == 8
