"""fp64 restatement of the reference's ``topk_rewire(..., directed=False)``
(src/utils/augmentation.py:36-86) and the admissibility rule its discrete
outputs are judged by (TEST INFRASTRUCTURE: only tests import it; the product
path is ngnn.ops.topk_rewire on the device).

With ``hn = F.normalize(h)``, ``S = hn hn^T``, ``A`` the adjacency of
``edge_index`` (duplicates collapse, self-loops count), ``D`` the diagonal
and ``k2 = 2 * int(N * k_percent)``, four selections of ``k2`` of the ``N*N``
entries:

    1 pos-remove  k2 smallest of  S * (1 if A and not D else 1000)
    2 pos-add     k2 largest  of  S - 100 [A and not sel1] - 100 [D]
    3 neg-remove  k2 largest  of  S * ([A] - 1000 [D])
    4 neg-add     k2 smallest of  S * ((1000 if A else 1) + 1000 [D])

``pos = (A and not sel1) or sel2``, ``neg = (A and not sel3) or sel4``, each
as ``torch.nonzero`` lists it.  Equal keys are taken in ascending flat index.

The rule (selections are discrete, so no tolerance on the outputs):
``delta = 4 * max |S_fp32 - S_fp64|``, both by torch on the CPU -- a property
of the inputs and of the reference's own arithmetic.  An entry of selection
``s`` is UNDECIDED if ``|key64 - t_s| <= delta * |multiplier of its class|``
(``t_s``: the k2-th fp64 key; selection 2 is additive: multiplier 1).  A
selection passes if it has exactly k2 distinct entries, holds every decided-in
entry and no decided-out entry.  Selection 2's keys are formed from the
selection 1 under test, so a boundary flip does not cascade.  ``pos`` and
``neg`` must equal, exactly and in order, what follows from the tested
selections.  A case is usable only if each selection has at most ``CAP``
undecided entries (the threshold entry and its symmetric twin give 1-2).
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

CAP = 4
LARGEST = (False, True, True, False)  # selections 1..4


def k2_of(n: int, k_percent: float) -> int:
    return 2 * int(n * k_percent)


def similarity(h: torch.Tensor, dtype) -> torch.Tensor:
    hn = F.normalize(h.detach().cpu().to(dtype), dim=1)
    return hn @ hn.t()


def adjacency(edge_index: torch.Tensor, n: int) -> torch.Tensor:
    a = torch.zeros(n, n, dtype=torch.bool)
    ei = edge_index.cpu()
    ok = (ei[0] >= 0) & (ei[0] < n) & (ei[1] >= 0) & (ei[1] < n)
    a[ei[0][ok], ei[1][ok]] = True
    return a


def delta_of(h: torch.Tensor) -> float:
    return 4.0 * float((similarity(h, torch.float32).double() - similarity(h, torch.float64)).abs().max()) \
        if h.numel() else 0.0


def multipliers(a: torch.Tensor):
    """|multiplier| per entry for the four selections (selection 2: additive, 1)."""
    n = a.size(0)
    d = torch.eye(n, dtype=torch.bool)
    one = torch.ones(n, n, dtype=torch.float64)
    m1 = torch.where(a & ~d, 1.0, 1000.0).double()
    m3 = a.double() - 1000.0 * d.double()
    m4 = torch.where(a, 1000.0, 1.0).double() + 1000.0 * d.double()
    return m1, one, m3, m4


def keys_of(s64: torch.Tensor, a: torch.Tensor, which: int, sel1: torch.Tensor | None = None) -> torch.Tensor:
    """Flattened fp64 keys of selection ``which`` (0-based); selection 2 needs
    the flat indices selection 1 took."""
    n = a.size(0)
    d = torch.eye(n, dtype=torch.bool)
    m1, _, m3, m4 = multipliers(a)
    if which == 0:
        return (s64 * m1).view(-1)
    if which == 2:
        return (s64 * m3).view(-1) + 0.0
    if which == 3:
        return (s64 * m4).view(-1)
    kept = a.clone().view(-1)
    kept[sel1] = False
    return (s64 - 100.0 * kept.view(n, n).double() - 100.0 * d.double()).view(-1)


def take(key: torch.Tensor, k2: int, largest: bool) -> torch.Tensor:
    """The k2 best flat indices, best first, equal keys in ascending index."""
    order = torch.argsort(-key if largest else key, stable=True)
    return order[:k2]


def edges_from(a: torch.Tensor, removed: torch.Tensor, added: torch.Tensor) -> torch.Tensor:
    m = a.clone().view(-1)
    m[removed] = False
    m[added] = True
    return torch.stack(torch.nonzero(m.view_as(a), as_tuple=True))


def topk_rewire_ref(h, edge_index, k_percent):
    """(pos_edge, neg_edge, [sel1..sel4]) in fp64."""
    n = h.size(0)
    k2 = k2_of(n, k_percent)
    s64 = similarity(h, torch.float64)
    a = adjacency(edge_index, n)
    sels = [None] * 4
    for w in (0, 2, 3):
        sels[w] = take(keys_of(s64, a, w), k2, LARGEST[w])
    sels[1] = take(keys_of(s64, a, 1, sels[0]), k2, True)
    return edges_from(a, sels[0], sels[1]), edges_from(a, sels[2], sels[3]), sels


def undecided_mask(key: torch.Tensor, mult: torch.Tensor, k2: int, largest: bool, delta: float):
    """(undecided, decided_in, decided_out) masks over the flat entries."""
    if k2 == 0:
        z = torch.zeros_like(key, dtype=torch.bool)
        return z, z, ~z
    srt = torch.sort(key, descending=largest).values
    t = srt[k2 - 1]
    und = (key - t).abs() <= delta * mult.view(-1).abs()
    better = (key > t) if largest else (key < t)
    return und, better & ~und, ~better & ~und


def check_selection(sel, key, mult, k2, largest, delta, what=""):
    """The rule for one selection; returns how many entries were undecided."""
    sel = sel.cpu().view(-1)
    assert sel.numel() == k2, f"{what}: {sel.numel()} entries, expected {k2}"
    assert torch.unique(sel).numel() == k2, f"{what}: repeated entries"
    assert k2 == 0 or (int(sel.min()) >= 0 and int(sel.max()) < key.numel()), f"{what}: index out of range"
    und, din, dout = undecided_mask(key, mult, k2, largest, delta)
    chosen = torch.zeros_like(und)
    chosen[sel] = True
    assert not bool((din & ~chosen).any()), \
        f"{what}: misses decided-in entries {torch.nonzero(din & ~chosen).flatten()[:8].tolist()}"
    assert not bool((dout & chosen).any()), \
        f"{what}: holds decided-out entries {torch.nonzero(dout & chosen).flatten()[:8].tolist()}"
    return int(und.sum())


def check_result(h, edge_index, k_percent, pos, neg, sels, cap=CAP, cap_exempt=()):
    """The whole rule for one call's outputs (selections: [4, k2] or a list of
    four).  ``cap_exempt``: 0-based selections whose threshold is a mass tie by
    construction (the caller then checks the tie rule itself).  Returns the
    undecided counts."""
    n = h.size(0)
    k2 = k2_of(n, k_percent)
    s64 = similarity(h, torch.float64)
    a = adjacency(edge_index, n)
    delta = delta_of(h)
    mults = multipliers(a)
    sels = [s.cpu() for s in sels]
    counts = []
    for w in (0, 1, 2, 3):  # (selection 2's keys from the tested selection 1, already checked)
        key = keys_of(s64, a, w, sels[0])
        counts.append(check_selection(sels[w], key, mults[w], k2, LARGEST[w], delta, f"selection {w + 1}"))
        if cap is not None and w not in cap_exempt:
            assert counts[-1] <= cap, f"selection {w + 1}: {counts[-1]} undecided entries (unusable case)"
    want_pos, want_neg = edges_from(a, sels[0], sels[1]), edges_from(a, sels[2], sels[3])
    for name, got, want in (("pos", pos, want_pos), ("neg", neg, want_neg)):
        got = got.cpu()
        assert got.dtype == torch.int64 and got.dim() == 2 and got.size(0) == 2, (name, got.dtype, got.shape)
        assert got.shape == want.shape and torch.equal(got, want), \
            f"{name}: {tuple(got.shape)} differs from what its selections give {tuple(want.shape)}"
    return counts


def make_case(n, f, relu, seed, deg=8, dup=10, loops=5):
    """Random h [n, f] (ReLU'd or signed) and about deg * n edges with ``dup``
    duplicated edges and ``loops`` self-loops, shuffled."""
    g = torch.Generator().manual_seed(seed)
    h = torch.randn(n, f, generator=g)
    if relu:
        h = torch.relu(h)
    e = deg * n
    ei = torch.randint(0, n, (2, e), generator=g)
    if e:
        d = min(dup, e)
        lp = torch.randint(0, n, (min(loops, n),), generator=g)
        ei = torch.cat([ei, ei[:, :d], torch.stack([lp, lp])], dim=1)
        ei = ei[:, torch.randperm(ei.size(1), generator=g)]
    return h, ei


# the device grid (tests/test_rewire_gpu.py), listed here so that the CPU suite
# can assert that every case is usable under the cap
GRID_N = (1, 64, 130, 257, 700)
GRID_F = (32, 33, 100, 131, 256)
GRID_K = 0.1


def grid_cases():
    """(n, f, relu, seed): every (N, F) pair, ReLU'd and signed alternating,
    plus the other kind on one diagonal of the grid."""
    out = []
    for i, n in enumerate(GRID_N):
        for j, f in enumerate(GRID_F):
            relu = (i + j) % 2 == 0
            out.append((n, f, relu, 1000 + 10 * i + j))
            if i == j:
                out.append((n, f, not relu, 2000 + 10 * i + j))
    return out
