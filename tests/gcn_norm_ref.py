"""Two independent host restatements of PyG 2.5.1's ``gcn_norm`` + ``GCNConv``
(Tensor ``edge_index``, flow source -> target), and the case table the GCN
normalisation tests share.

* ``pyg_gcn_conv``: PyG's op sequence in torch, any dtype -- the self-loop
  rewrite of ``add_remaining_self_loops``, ``scatter_add_`` degree, ``pow``,
  two ``index_select``, ``mul``, the ``[E, F]`` messages and ``index_add_``.
* ``dense_gcn_conv``: ``D^-1/2 A^ D^-1/2 (X W^T) + b`` with a dense float64
  adjacency built entry by entry in numpy -- no scatter, no edge rewrite.

Several weighted self-loops on one node are unspecified in PyG (an
``index_put`` with duplicates): both restatements keep the LAST in edge
order, as the kernels document; the case table holds at most one per node.
"""
import numpy as np
import torch

N_SIZES = (1, 3, 65, 300, 1025)
WIDTHS = ((1, 1), (7, 5), (64, 65), (100, 47), (130, 16), (767, 10))
GRAPHS = ("empty", "tail_isolated", "self_loops", "duplicates", "unsorted", "target_sorted", "hub")
MODES = ((True, False), (True, True), (False, False), (False, True))  # (add_self_loops, weighted)


def pyg_norm(edge_index, edge_weight, N, add_self_loops, dtype):
    """gcn_norm: (edge_index', edge_weight') with the symmetric coefficients."""
    src, dst = edge_index[0], edge_index[1]
    w = torch.ones(src.numel(), dtype=dtype) if edge_weight is None else edge_weight.to(dtype)
    if add_self_loops:
        # add_remaining_self_loops(fill_value=1): drop the loops, append one per
        # node whose weight is the dropped loop's (the last one wins), else 1
        mask = src != dst
        loop_w = torch.ones(N, dtype=dtype)
        if edge_weight is not None:
            for s, v in zip(src[~mask].tolist(), w[~mask].tolist()):
                loop_w[s] = v
        ar = torch.arange(N, dtype=src.dtype)
        src, dst = torch.cat([src[mask], ar]), torch.cat([dst[mask], ar])
        w = torch.cat([w[mask], loop_w])
    deg = torch.zeros(N, dtype=dtype).scatter_add_(0, dst, w)
    dinv = deg.pow(-0.5)
    dinv.masked_fill_(dinv == float("inf"), 0)
    return src, dst, dinv.index_select(0, src) * w * dinv.index_select(0, dst)


def pyg_gcn_conv(x, edge_index, edge_weight, W, b, add_self_loops=True, normalize=True):
    """GCNConv.forward in PyG's order (transform first); differentiable."""
    N, dtype = x.size(0), x.dtype
    if normalize:
        src, dst, coef = pyg_norm(edge_index, edge_weight, N, add_self_loops, dtype)
    else:
        src, dst = edge_index[0], edge_index[1]
        coef = (torch.ones(src.numel(), dtype=dtype) if edge_weight is None else edge_weight.to(dtype))
    z = torch.nn.functional.linear(x, W)
    msg = z.index_select(0, src) * coef.unsqueeze(1)
    out = torch.zeros(N, W.size(0), dtype=dtype).index_add_(0, dst, msg)
    return out + b


def dense_adj(edge_index, edge_weight, N, add_self_loops=True, normalize=True):
    """float64 [N, N] numpy: row = target, column = source."""
    A = np.zeros((N, N), dtype=np.float64)
    loop = np.ones(N, dtype=np.float64)
    src, dst = edge_index[0].tolist(), edge_index[1].tolist()
    w = [1.0] * len(src) if edge_weight is None else [float(v) for v in edge_weight.double().tolist()]
    for s, t, v in zip(src, dst, w):
        if normalize and add_self_loops and s == t:
            if edge_weight is not None:
                loop[s] = v
            continue
        A[t, s] += v
    if normalize and add_self_loops:
        A[np.arange(N), np.arange(N)] += loop
    if normalize:
        deg = A.sum(axis=1)
        with np.errstate(divide="ignore", invalid="ignore"):
            dinv = np.where(deg == 0, 0.0, 1.0 / np.sqrt(deg))
        A = dinv[:, None] * A * dinv[None, :]
    return A


def dense_gcn_conv(x, edge_index, edge_weight, W, b, add_self_loops=True, normalize=True, dout=None):
    """(out, dx, dW, db) in float64 numpy; the gradients for the output
    gradient ``dout`` (None: forward only)."""
    A = dense_adj(edge_index, edge_weight, x.shape[0], add_self_loops, normalize)
    X, Wd, bd = (np.asarray(t.detach().double().cpu().numpy()) for t in (x, W, b))
    out = A @ (X @ Wd.T) + bd
    if dout is None:
        return out
    G = np.asarray(dout.detach().double().cpu().numpy())
    AtG = A.T @ G
    return out, AtG @ Wd, AtG.T @ X, G.sum(axis=0)


def make_graph(kind: str, N: int, seed: int = 0):
    """int64 edge_index [2, E] of the case table.  Every kind but
    ``self_loops`` may still hold a few self-loops by chance; callers that
    weight the edges pass the result through ``one_loop_per_node``."""
    g = torch.Generator().manual_seed(1000 + seed)
    E = 0 if kind == "empty" else max(4 * N, 8)

    def rnd(n, hi=N):
        return torch.randint(0, max(hi, 1), (n,), generator=g)
    if kind == "empty":
        return torch.zeros(2, 0, dtype=torch.int64)
    if kind == "tail_isolated":  # the last N/8 nodes receive no edge
        return torch.stack([rnd(E), rnd(E, N - N // 8)])
    if kind == "self_loops":
        loops = torch.randperm(N, generator=g)[:max(N // 3, 1)]
        ei = torch.cat([torch.stack([rnd(E), rnd(E)]), torch.stack([loops, loops])], dim=1)
        return ei[:, torch.randperm(ei.size(1), generator=g)]
    if kind == "duplicates":
        ei = torch.stack([rnd(E // 2), rnd(E // 2)])
        return torch.cat([ei, ei], dim=1)
    if kind == "unsorted":
        return torch.stack([rnd(E), rnd(E)])
    if kind == "target_sorted":
        ei = torch.stack([rnd(E), rnd(E)])
        return ei[:, torch.argsort(ei[1], stable=True)]
    if kind == "hub":  # one row of 1,000 in-edges
        hub = N // 2
        ei = torch.cat([torch.stack([rnd(E), rnd(E)]),
                        torch.stack([rnd(1000), torch.full((1000,), hub, dtype=torch.int64)])], dim=1)
        return ei[:, torch.randperm(ei.size(1), generator=g)]
    raise ValueError(kind)


def one_loop_per_node(ei):
    """Drops all but the first self-loop edge of every node."""
    keep, seen = [], set()
    for i, (s, t) in enumerate(zip(ei[0].tolist(), ei[1].tolist())):
        if s == t:
            if s in seen:
                continue
            seen.add(s)
        keep.append(i)
    return ei[:, torch.tensor(keep, dtype=torch.int64)] if ei.size(1) else ei


def make_case(kind, N, widths, mode, seed=0):
    """(edge_index, edge_weight or None, x, W, b, dout) on the host, float32
    (x, W, b, dout exactly representable inputs of both precisions)."""
    Fi, Fo = widths
    loops, weighted = mode
    g = torch.Generator().manual_seed(seed)
    ei = make_graph(kind, N, seed)
    ew = None
    if weighted:
        ei = one_loop_per_node(ei)
        ew = 0.1 + 1.9 * torch.rand(ei.size(1), generator=g)
    x = torch.randn(N, Fi, generator=g)
    a = (6.0 / (Fi + Fo)) ** 0.5
    W = (torch.rand(Fo, Fi, generator=g) * 2 - 1) * a
    b = torch.randn(Fo, generator=g) * 0.1
    dout = torch.randn(N, Fo, generator=g)
    return ei, ew, x, W, b, dout


def shapes():
    """Every (N, (F_in, F_out)) of the table: the tests' parametrisation; each
    runs ``graph_modes()`` inside."""
    return [(N, wd) for N in N_SIZES for wd in WIDTHS]


def graph_modes():
    """Every graph kind with every (add_self_loops, weighted) combination."""
    return [(kind, mode) for kind in GRAPHS for mode in MODES]
