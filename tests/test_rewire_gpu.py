"""ngnn.ops.topk_rewire on the device: the reference's own fixtures, a grid of
shapes at tile and vector boundaries against the fp64 restatement under the
admissibility rule (tests/rewire_ref.py), the edge cases of k2 and E, the tie
rule, determinism, bad endpoints, the refusals, and SAGEPL run on the
returned edge lists."""
import pytest
import torch

import ngnn
from ngnn import _lib, ops

import rewire_ref as rr
import sagepl_ref
from test_rewire_cpu import FIXTURES, assert_edges_admissible, load_fixture

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def run(h, ei, kp):
    pos, neg, sel = ops.topk_rewire(h.to(DEV), ei.to(DEV), DEV, k_percent=kp, return_selections=True)
    for t in (pos, neg):
        assert t.is_cuda and t.dtype == torch.int64 and t.is_contiguous() and t.dim() == 2 and t.size(0) == 2
    assert sel.shape == (4, rr.k2_of(h.size(0), kp)) and sel.dtype == torch.int64
    return pos, neg, sel


@pytest.mark.parametrize("name", FIXTURES)
def test_reference_fixture(golden_dir, name):
    h, ei, kp, _, _ = load_fixture(golden_dir, name)
    pos, neg, sel = run(h, ei, kp)
    rr.check_result(h, ei, kp, pos, neg, sel)
    # and against the reference's own edge lists, which come without selections
    assert_edges_admissible(h, ei, kp, pos.cpu(), neg.cpu())
    p2, n2 = ngnn.topk_rewire(h.to(DEV), ei.to(DEV), "cpu", kp)  # the reference's positional call
    assert torch.equal(p2, pos) and torch.equal(n2, neg)


@pytest.mark.parametrize("n,f,relu,seed", rr.grid_cases())
def test_grid(n, f, relu, seed):
    h, ei = rr.make_case(n, f, relu, seed)
    pos, neg, sel = run(h, ei, rr.GRID_K)
    rr.check_result(h, ei, rr.GRID_K, pos, neg, sel)


@pytest.mark.parametrize("n,f", [(130, 33), (257, 100)])
def test_padded_rows_and_offset_base(n, f):
    """h as a view: leading dimension f + 3, base one element into its buffer."""
    h, ei = rr.make_case(n, f, False, 77)
    buf = torch.full((n * (f + 3) + 1,), float("nan"), device=DEV)
    view = buf[1:].view(n, f + 3)[:, :f]
    view.copy_(h)
    assert view.data_ptr() % 16 == 4 and view.stride(0) == f + 3
    pos, neg, sel = ops.topk_rewire(view, ei.to(DEV), k_percent=0.1, return_selections=True)
    rr.check_result(h, ei, 0.1, pos, neg, sel)
    want = run(h, ei, 0.1)
    for a, b in zip((pos, neg, sel), want):
        assert torch.equal(a, b)


def test_no_edges():
    h, _ = rr.make_case(130, 32, False, 11)
    ei = torch.empty(2, 0, dtype=torch.int64)
    pos, neg, sel = run(h, ei, 0.1)
    # selection 3 multiplies every non-edge by 0: one mass tie at its threshold, by construction
    rr.check_result(h, ei, 0.1, pos, neg, sel, cap_exempt=(2,))
    k2 = rr.k2_of(130, 0.1)
    assert pos.size(1) == k2 and neg.size(1) == k2
    # the tie rule on that mass tie: the first k2 off-diagonal entries in flat-index order
    assert k2 < 130 and sel[2].tolist() == list(range(1, k2 + 1))


def test_k2_zero_returns_sorted_unique_edges():
    h, ei = rr.make_case(257, 33, True, 12)
    pos, neg, sel = run(h, ei, 0.001)  # int(0.257) = 0
    assert sel.shape == (4, 0)
    n = h.size(0)
    want = torch.unique(ei[0] * n + ei[1])
    want = torch.stack([want // n, want % n])
    assert torch.equal(pos.cpu(), want) and torch.equal(neg.cpu(), want)


def test_k2_larger_than_distinct_edges():
    h, ei = rr.make_case(64, 33, False, 13, deg=1, dup=2, loops=1)
    n, kp = 64, 0.9
    k2 = rr.k2_of(n, kp)
    a = rr.adjacency(ei, n)
    assert k2 > int(a.sum())
    pos, neg, sel = run(h, ei, kp)
    # selection 3 runs out of edges and into the non-edges' zeros: a mass tie by construction
    rr.check_result(h, ei, kp, pos, neg, sel, cap_exempt=(2,))
    # the tie rule there: after the entries with a positive key, zeros in ascending flat index --
    # bitwise what the restatement takes
    _, _, ref = rr.topk_rewire_ref(h, ei, kp)
    key = rr.keys_of(rr.similarity(h, torch.float64), a, 2)
    got = sel[2].cpu()
    zeros = got[key[got] == 0]
    assert zeros.numel() > 0 and bool((zeros[1:] > zeros[:-1]).all())
    assert torch.equal(zeros, ref[2][key[ref[2]] == 0])


def test_zero_row():
    h, ei = rr.make_case(130, 100, True, 14)
    h[7] = 0.0
    h[129] = 0.0
    pos, neg, sel = run(h, ei, 0.1)
    # every entry of a zero row has S = 0 exactly (its diagonal too, not 1): with ReLU'd rows
    # elsewhere these 2 * 2 * 130 zeros are the smallest keys of selections 1 and 4 -- a tie
    # larger than k2 by construction, resolved by flat index
    rr.check_result(h, ei, 0.1, pos, neg, sel, cap_exempt=(0, 3))
    _, _, ref = rr.topk_rewire_ref(h, ei, 0.1)
    assert torch.equal(sel[0].cpu(), ref[0]) and torch.equal(sel[3].cpu(), ref[3])
    assert sel[0].tolist() == sorted(sel[0].tolist())
    assert all(i // 130 in (7, 129) or i % 130 in (7, 129) for i in sel[0].tolist())


def test_concentrated_similarities_take_the_refinement_pass():
    """All of N*N similarities inside one histogram bucket (rows 1 + 0.007 *
    noise: S = 1 - O(5e-5)), more than a candidate list holds (k2 + 2^20): the
    threshold buckets are split and the selection still passes the rule.  At
    that density thousands of entries are within delta of any threshold, so the
    cap on undecided entries does not apply; decided entries are still held to
    the rule and the edge lists to their selections."""
    n, f, kp = 1100, 32, 0.1
    g = torch.Generator().manual_seed(21)
    h = 1.0 + 0.007 * torch.randn(n, f, generator=g)
    _, ei = rr.make_case(n, f, False, 21, deg=2)
    s = rr.similarity(h, torch.float64)
    assert float(s.min()) > 1.0 - 2.0 / 8192 and n * n > rr.k2_of(n, kp) + (1 << 20)
    pos, neg, sel = run(h, ei, kp)
    rr.check_result(h, ei, kp, pos, neg, sel, cap=None)
    again = run(h, ei, kp)
    for x, y in zip((pos, neg, sel), again):
        assert torch.equal(x, y)


def test_a_mass_tie_beyond_the_lists_is_reported():
    """1100 identical rows: 1.21 M equal similarities at every threshold, more
    than a candidate list holds.  Nothing is returned; the call says why."""
    h = torch.ones(1100, 32)
    ei = torch.tensor([[0, 1], [1, 2]])
    with pytest.raises(_lib.NGNNError, match="tie"):
        ops.topk_rewire(h.to(DEV), ei.to(DEV), k_percent=0.1)
    # the same tie below the lists' size is resolved by flat index: without edges, selection 2
    # takes the first k2 = 12 off-diagonal entries
    pos, neg, sel = run(torch.ones(64, 32), torch.empty(2, 0, dtype=torch.int64), 0.1)
    assert sel[1].tolist() == list(range(1, 13))
    assert pos.tolist() == [[0] * 12, list(range(1, 13))]


def test_two_calls_are_bitwise_equal():
    h, ei = rr.make_case(700, 131, True, 15)
    a = run(h, ei, 0.2)
    b = run(h, ei, 0.2)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_ties_go_by_flat_index():
    """Rows 3 and 40 are identical: S[i,3] == S[i,40] and S[3,j] == S[40,j]
    bitwise, and S is symmetric.  Within a selection, entries with equal keys
    appear in ascending flat index, and an entry is never taken while an
    equal-keyed entry with a smaller index is left out."""
    n = 64
    h, ei = rr.make_case(n, 33, False, 16)
    h[40] = h[3]
    pos, neg, sel = run(h, ei, 0.25)
    rr.check_result(h, ei, 0.25, pos, neg, sel, cap=None)
    a = rr.adjacency(ei, n)
    hn = torch.nn.functional.normalize(h.double(), dim=1)
    s = hn @ hn.t()
    twin = torch.arange(n)
    twin[3], twin[40] = 40, 3
    seen_pairs = 0
    for w in (0, 1, 3):  # the selections that range over the non-edges' similarities
        got = sel[w].cpu().tolist()
        rank = {idx: r for r, idx in enumerate(got)}
        for idx in got:
            i, j = divmod(idx, n)
            for oi, oj in ((j, i), (twin[i].item(), j), (i, twin[j].item())):  # entries with the same S
                o = oi * n + oj
                if o == idx or oi == oj or i == j or a[i, j] or a[oi, oj]:
                    continue  # (only plain non-edges: same class, so the same key)
                assert s[i, j] == s[oi, oj] or abs(float(s[i, j] - s[oi, oj])) < 1e-15
                if o in rank:
                    seen_pairs += 1
                    assert (rank[o] < rank[idx]) == (o < idx), (w, idx, o)
                else:
                    # the twin was left out: only possible at the cut, and only for the larger index
                    assert o > idx, (w, idx, o)
    assert seen_pairs > 0


def test_out_of_range_endpoint_is_ignored_and_counted():
    h, ei = rr.make_case(130, 32, False, 17)
    n = 130
    bad = torch.tensor([[0, n, -1, 5], [n, 3, 2, 1 << 40]])
    ei_bad = torch.cat([ei[:, :50], bad, ei[:, 50:]], dim=1)
    ops.rewire_bad_endpoints(DEV, reset=True)
    want = run(h, ei, 0.1)
    assert ops.rewire_bad_endpoints(DEV) == 0
    got = run(h, ei_bad, 0.1)
    assert ops.rewire_bad_endpoints(DEV, reset=True) == 4
    for x, y in zip(got, want):
        assert torch.equal(x, y)
    assert int(got[0].max()) < n and int(got[0].min()) >= 0


def test_refusals():
    h, ei = rr.make_case(64, 32, False, 18)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.topk_rewire(h, ei)
    with pytest.raises(TypeError, match="float32"):
        ops.topk_rewire(h.to(DEV).bfloat16(), ei.to(DEV))
    with pytest.raises(NotImplementedError, match="directed"):
        ops.topk_rewire(h.to(DEV), ei.to(DEV), directed=True)
    with pytest.raises(ValueError):
        ops.topk_rewire(h.to(DEV), ei.to(DEV).int())
    # N > 65535: refused by the entry's argument check, before any workspace exists
    lib = _lib.load()
    assert lib.ngnn_topk_rewire_workspace_bytes(65536, 4, 0, 0) == 0
    big = torch.zeros(65536, 1, device=DEV)
    with pytest.raises(_lib.NGNNError, match="rc=-5"):
        ops.topk_rewire(big, torch.empty(2, 0, dtype=torch.int64, device=DEV), k_percent=0.0)
    # N == 0
    pos, neg = ops.topk_rewire(torch.empty(0, 8, device=DEV), torch.empty(2, 0, dtype=torch.int64, device=DEV))
    assert pos.shape == (2, 0) and neg.shape == (2, 0)


def test_sagepl_runs_on_the_rewired_graphs():
    """The pipelines' use: h_pure of a SAGEPL call rewires the block's edges,
    and the model runs again on pos_edge / neg_edge (source-sorted lists)."""
    torch.manual_seed(19)
    n, f, hid, c = 257, 33, 64, 7
    _, ei = rr.make_case(n, f, False, 19)
    x = torch.randn(n, f)
    ref = sagepl_ref.SAGEPL(f, hid, c, 2, nbr_nodes=n, dropout=0.0).eval()
    mine = ngnn.SAGEPL(f, hid, c, 2, nbr_nodes=n, dropout=0.0)
    mine.load_state_dict(ref.state_dict(), strict=True)
    mine.to(DEV).eval()
    n_id = torch.arange(n)
    with torch.no_grad():
        h_pure = mine(x.to(DEV), ei.to(DEV), noise_rate=0.1, n_id=n_id.to(DEV))[0]
        pos, neg, sel = ops.topk_rewire(h_pure, ei.to(DEV), DEV, k_percent=0.2, return_selections=True)
        rr.check_result(h_pure.cpu(), ei, 0.2, pos, neg, sel)
        for edges in (pos, neg):
            assert bool((edges[0][1:] >= edges[0][:-1]).all())  # source-sorted
            outs = mine(x.to(DEV), edges, noise_rate=0.1, n_id=n_id.to(DEV))
            want = ref(x, edges.cpu(), noise_rate=0.1, n_id=n_id)
            for nm, o, wv in zip(sagepl_ref.OUT_NAMES, outs, want):
                torch.testing.assert_close(o.cpu(), wv, rtol=1e-5, atol=1e-5, msg=lambda s: f"{nm}: {s}")
