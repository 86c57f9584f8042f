"""The fp64 restatement of topk_rewire (tests/rewire_ref.py) against the
reference's own function (tests/golden/rewire_*.npz, written by
tests/golden/make_golden_rewire.py), under the admissibility rule; and the
rule's precondition -- at most CAP undecided entries per selection -- on every
case the device tests use."""
import os

import numpy as np
import pytest
import torch

import rewire_ref as rr

FIXTURES = ("rewire_relu_333", "rewire_signed_257", "rewire_relu_130")


def load_fixture(golden_dir, name):
    rec = np.load(os.path.join(golden_dir, name + ".npz"))
    return (torch.as_tensor(rec["h"]), torch.as_tensor(rec["edge_index"]), float(rec["k_percent"]),
            torch.as_tensor(rec["pos_edge"]), torch.as_tensor(rec["neg_edge"]))


def flat_set(edges, n):
    return set((edges[0] * n + edges[1]).tolist())


def assert_edges_admissible(h, ei, kp, got_pos, got_neg):
    """Edge lists without their selections (the reference returns none): they
    may differ from the fp64 restatement's only in undecided entries."""
    n = h.size(0)
    k2 = rr.k2_of(n, kp)
    pos, neg, sels = rr.topk_rewire_ref(h, ei, kp)
    s64, a, delta = rr.similarity(h, torch.float64), rr.adjacency(ei, n), rr.delta_of(h)
    mults = rr.multipliers(a)
    und = []
    for w in range(4):
        u, _, _ = rr.undecided_mask(rr.keys_of(s64, a, w, sels[0]), mults[w], k2, rr.LARGEST[w], delta)
        assert int(u.sum()) <= rr.CAP, f"selection {w + 1}: {int(u.sum())} undecided entries"
        und.append(set(torch.nonzero(u).flatten().tolist()))
    for name, got, want, free in (("pos", got_pos, pos, und[0] | und[1]), ("neg", got_neg, neg, und[2] | und[3])):
        assert got.dtype == torch.int64 and got.size(0) == 2
        flat = got[0] * n + got[1]
        assert bool((flat[1:] > flat[:-1]).all()), f"{name}: not sorted by (row, column) without duplicates"
        diff = flat_set(got, n) ^ flat_set(want, n)
        assert diff <= free, f"{name}: differs in decided entries {sorted(diff - free)[:8]}"


@pytest.mark.parametrize("name", FIXTURES)
def test_restatement_matches_reference_fixture(golden_dir, name):
    h, ei, kp, pos, neg = load_fixture(golden_dir, name)
    assert ei.size(1) - torch.unique(ei, dim=1).size(1) >= 10  # duplicated edges
    assert int((ei[0] == ei[1]).sum()) >= 5                      # self-loops
    assert_edges_admissible(h, ei, kp, pos, neg)


@pytest.mark.parametrize("name", FIXTURES)
def test_restatement_passes_its_own_rule(golden_dir, name):
    h, ei, kp, _, _ = load_fixture(golden_dir, name)
    pos, neg, sels = rr.topk_rewire_ref(h, ei, kp)
    counts = rr.check_result(h, ei, kp, pos, neg, sels)
    assert max(counts) <= rr.CAP


def test_grid_cases_are_usable():
    """Every device-grid case leaves at most CAP undecided entries per
    selection in fp64, and delta is of fp32's size."""
    for n, f, relu, seed in rr.grid_cases():
        h, ei = rr.make_case(n, f, relu, seed)
        pos, neg, sels = rr.topk_rewire_ref(h, ei, rr.GRID_K)
        counts = rr.check_result(h, ei, rr.GRID_K, pos, neg, sels)
        assert max(counts) <= rr.CAP, (n, f, relu, counts)
        assert rr.delta_of(h) < 1e-5, (n, f, relu)


def test_rule_rejects_a_wrong_selection():
    h, ei = rr.make_case(64, 33, False, 5)
    pos, neg, sels = rr.topk_rewire_ref(h, ei, 0.1)
    bad = [s.clone() for s in sels]
    key = rr.keys_of(rr.similarity(h, torch.float64), rr.adjacency(ei, 64), 3)
    bad[3][0] = torch.argmax(key)  # the worst entry of a k2-smallest selection
    with pytest.raises(AssertionError):
        rr.check_result(h, ei, 0.1, pos, neg, bad)
    with pytest.raises(AssertionError):  # outputs that do not follow from the selections
        rr.check_result(h, ei, 0.1, pos[:, :-1], neg, sels)


def test_semantics_by_hand():
    """Four nodes: rows 0 and 1 parallel, 2 orthogonal to them, 3 a zero row."""
    h = torch.tensor([[1.0, 0.0], [2.0, 0.0], [0.0, 1.0], [0.0, 0.0]])
    ei = torch.tensor([[0, 0, 2, 0], [2, 2, 2, 1]])  # (0,2) twice, the self-loop (2,2), (0,1)
    pos, neg, sels = rr.topk_rewire_ref(h, ei, 0.3)  # k2 = 2
    # selection 1: key 0 wherever S = 0 (the zero row's diagonal included), taken in flat-index
    # order: the edge (0,2), then the non-edge (0,3)
    assert sels[0].tolist() == [2, 3]
    # selection 2: the one S = 1 entry without a penalty is (1,0); then the zeros in index order,
    # the removed edge (0,2) first -- it comes straight back
    assert sels[1].tolist() == [4, 2]
    assert pos.tolist() == [[0, 0, 1, 2], [1, 2, 0, 2]]
    # selection 3: the edge (0,1) with S = 1, then the zeros: the edge (0,2); the self-loop (2,2)
    # has key -999 and stays
    assert sels[2].tolist() == [1, 2]
    # selection 4: zeros in index order; (0,2) was just removed and is added again
    assert sels[3].tolist() == [2, 3]
    assert neg.tolist() == [[0, 0, 2], [2, 3, 2]]
    assert pos.dtype == torch.int64 and neg.dtype == torch.int64
