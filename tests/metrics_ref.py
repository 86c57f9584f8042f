"""The reference's metric lines restated in torch on the CPU, for the tests of
ngnn.metrics (pipeline.py:120-125, :164-165, :182-195):

    total_loss += float(loss)
    total_correct += int(out.argmax(dim=-1).eq(y).sum())
    acc = correct / len(idx)          (Evaluator.eval / accuracy_score)

and the confusion matrix as bincount(y * C + pred).  Everything here is exact:
integer counts, and Python-float (fp64) running sums of fp32 values in the
order they were produced."""
import torch

NAN, INF = float("nan"), float("inf")
# hand-written rows for the tie rule and the index torch.argmax gives for each
HAND_ROWS = [[1.0, NAN, 5.0, NAN],
             [0.0, -0.0, 0.0, -1.0],
             [-INF] * 4,
             [INF, 3.0, INF, NAN],
             [2.0] * 4,
             [-0.0, 0.0, -1.0, -2.0]]
HAND_ARGMAX = [1, 0, 0, 3, 0, 0]


def hand_rows(C: int, dtype=torch.float32) -> torch.Tensor:
    """HAND_ROWS widened to C >= 4 columns with -inf, which changes no argmax."""
    t = torch.full((len(HAND_ROWS), C), -INF)
    t[:, :4] = torch.tensor(HAND_ROWS)
    return t.to(dtype)


def argmax_rows(out: torch.Tensor) -> torch.Tensor:
    """out.argmax(dim=-1) on the CPU, bf16 widened exactly first."""
    return out.detach().cpu().float().argmax(dim=-1)


def step_counts(out, y, batch_size=None, ignore_index=-100):
    """(rows, correct, bad_labels) of one batch: the reference's
    int(out.argmax(dim=-1).eq(y).sum()) over the first batch_size rows, the
    rows whose label is a class, and the labels that are neither a class nor
    ignore_index."""
    y = y.detach().cpu().reshape(-1)
    B = y.numel() if batch_size is None else batch_size
    out, y = out.detach().cpu()[:B], y[:B]
    C = out.size(1)
    correct = int(argmax_rows(out).eq(y).sum()) if B else 0
    valid = (y >= 0) & (y < C)
    return int(valid.sum()), correct, int((~valid & (y != ignore_index)).sum())


def running_sum(values) -> float:
    """total = 0; total += float(v) for each: the reference's epoch sums."""
    total = 0.0
    for v in values:
        total += float(v)
    return total


def split_counts(out, y, idx, ignore_index=-100):
    """(evaluated, correct, bad, ignored) of one index list: every entry
    counts, repeated ids too; an id outside [0, N) or a label outside [0, C)
    that is not ignore_index is bad and its row is not looked at."""
    out, y, idx = out.detach().cpu(), y.detach().cpu().reshape(-1), idx.detach().cpu()
    N, C = out.shape
    ok = (idx >= 0) & (idx < N)
    ids = idx[ok]
    lab = y[ids]
    valid = (lab >= 0) & (lab < C)
    ignored = int((lab == ignore_index).sum())
    bad = int((~ok).sum()) + int((~valid).sum()) - ignored
    pred = argmax_rows(out[ids[valid]]) if int(valid.sum()) else torch.zeros(0, dtype=torch.int64)
    return int(valid.sum()), int(pred.eq(lab[valid]).sum()), bad, ignored


def split_accuracy(out, y, split_idx, ignore_index=-100):
    """{name: correct / len(idx)}: the OGB Evaluator's and accuracy_score's quotient."""
    return {k: (split_counts(out, y, idx, ignore_index)[1] / idx.numel() if idx.numel() else float("nan"))
            for k, idx in split_idx.items()}


def pred_rows(out, idx):
    """argmax of row idx[p], -1 for an id outside [0, N)."""
    out, idx = out.detach().cpu(), idx.detach().cpu()
    ok = (idx >= 0) & (idx < out.size(0))
    pred = torch.full((idx.numel(),), -1, dtype=torch.int64)
    if int(ok.sum()):
        pred[ok] = argmax_rows(out[idx[ok]])
    return pred


def confusion(out, y, idx, ignore_index=-100):
    """bincount(y * C + pred) over the evaluated entries of idx, [C, C]."""
    out, y, idx = out.detach().cpu(), y.detach().cpu().reshape(-1), idx.detach().cpu()
    N, C = out.shape
    ids = idx[(idx >= 0) & (idx < N)]
    lab = y[ids]
    valid = (lab >= 0) & (lab < C)
    ids, lab = ids[valid], lab[valid]
    if not ids.numel():
        return torch.zeros(C, C, dtype=torch.int64)
    return torch.bincount(lab * C + argmax_rows(out[ids]), minlength=C * C).view(C, C)
