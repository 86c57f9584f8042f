"""Block-free layer-wise inference (ngnn.infer, ABI 22) against the loader and
the reference loop.

The fused plan's draws must be BITWISE the in-edges NeighborLoader's blocks
give their seed rows, and its outputs must match the loop (and the CPU
oracle's ``inference`` fed the same blocks) at the project's output bar,
rtol = atol = 1e-5.  ``ngnn.models.last_inference_plan`` is asserted
throughout, so a silent fallback to the loop cannot pass.
"""
import pytest
import torch

import ngnn
from ngnn import infer, models, ops
from ngnn.loader import Graph, NeighborLoader
from oracle import pyg_ref

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
OUT_TOL = dict(rtol=1e-5, atol=1e-5)
N, F, BS = 300, 100, 64  # 5 batches, the last with 44 seeds
SEED = 5


def build_graph():
    """N = 300 nodes; in-degrees 0, 1, f - 1, f, f + 1, 2 f for every fanout
    the tests draw with, one hub of 1000 (so its row repeats neighbours), a
    few rows of one neighbour repeated, the rest random."""
    g = torch.Generator().manual_seed(11)
    degs = [0, 1, 1000]
    for f in (3, 5, 10, 15, 16, 64):
        degs += [f - 1, f, f + 1, 2 * f]
    degs += torch.randint(0, 41, (N - len(degs),), generator=g).tolist()
    degs = torch.tensor(degs)[torch.randperm(N, generator=g)]
    rowptr = torch.zeros(N + 1, dtype=torch.int64)
    rowptr[1:] = torch.cumsum(degs, 0)
    col = torch.randint(0, N, (int(rowptr[-1]),), generator=g, dtype=torch.int64)
    for v in (7, 100, 250):  # duplicate neighbours, deg above and below the fanouts
        col[rowptr[v]:rowptr[v + 1]] = (v * 13) % N
    x = torch.randn(N, F, generator=g)
    y = torch.randint(0, 47, (N,), generator=g)
    return Graph(rowptr.to(DEV), col.to(torch.int32).to(DEV), x.to(DEV), y.to(DEV),
                 torch.arange(N, device=DEV), 47)


@pytest.fixture(scope="module")
def graph():
    return build_graph()


class Wrapped:
    """A plain iterable over a loader's batches: forces the reference loop."""

    def __init__(self, loader, device=None):
        self.loader, self.device = loader, device

    def __iter__(self):
        for b in self.loader:
            yield b if self.device is None else b.to(self.device)


def loader_of(graph, fanouts, **kw):
    return NeighborLoader(graph, None, num_neighbors=fanouts, batch_size=BS, seed=SEED, **kw)


def seed_row_edges(batch):
    """(count per seed row, global sources in order) of a block's seed rows."""
    ei, B = batch.edge_index, batch.batch_size
    m = ei[1] < B
    return torch.bincount(ei[1][m], minlength=B), batch.n_id[ei[0][m]]


# ------------------------------------------------------------------ draws
@pytest.mark.parametrize("fanouts", [[15, 10], [5, 3], [16], [64]])
@pytest.mark.parametrize("permuted", [False, True])
def test_draws_are_the_loaders_bitwise(graph, fanouts, permuted):
    nodes = None
    if permuted:
        nodes = torch.randperm(N, generator=torch.Generator().manual_seed(2)).to(DEV)
    twin = NeighborLoader(graph, nodes, num_neighbors=fanouts, batch_size=BS, seed=SEED)
    twin.epoch = 3
    cnts, cols = zip(*(seed_row_edges(b) for b in twin))
    cnt, col = torch.cat(cnts), torch.cat(cols)
    assert cnt.numel() == N and len(cnts) == 5 and cnts[-1].numel() == 44
    want_rp = torch.zeros(N + 1, dtype=torch.int64, device=DEV)
    want_rp[1:] = torch.cumsum(cnt, 0)
    s0 = twin.batch_seed(3, 0)
    stride = twin.batch_seed(3, 1) - s0
    rp, c = ops.sample_seed_rows(graph, fanouts[0], BS, s0, stride, 0, N, seeds=nodes)
    assert rp.dtype == torch.int32 and c.dtype == torch.int32
    assert torch.equal(rp.long(), want_rp)
    assert torch.equal(c.long(), col)
    # the tail alone: positions 128 .. 299
    rp2, c2 = ops.sample_seed_rows(graph, fanouts[0], BS, s0, stride, 128, N - 128, seeds=nodes)
    assert torch.equal(rp2.long(), want_rp[128:] - want_rp[128])
    assert torch.equal(c2.long(), col[int(want_rp[128]):])


def test_draw_refuses_a_start_inside_a_batch(graph):
    with pytest.raises(ngnn._lib.NGNNError):
        ops.sample_seed_rows(graph, 15, BS, 1, 1, 32, 64)


# ------------------------------------------------------------- end to end
def make_model(kind, dims, aggr):
    torch.manual_seed(0)
    m = ngnn.SAGE(*dims, aggr=aggr) if kind == "sage" else ngnn.SimpleGCN(*dims)
    m.reset_parameters()
    ref = pyg_ref.SAGE(*dims, aggr=aggr) if kind == "sage" else pyg_ref.SimpleGCN(*dims)
    ref.load_state_dict(m.state_dict())
    return m.to(DEV).eval(), ref.eval()


MODELS = {
    "sage_mean": ("sage", (100, 256, 47, 2), "mean", ["rowtile", "narrow"]),
    "sage_sum3": ("sage", (100, 32, 16, 3), "sum", ["narrow", "rowtile", "narrow"]),
    "sage_max": ("sage", (100, 64, 8, 2), "max", ["rowtile", "rowtile"]),
    "gcn": ("gcn", (100, 256, 47, 2), None, ["rowtile", "narrow"]),
}


@pytest.mark.parametrize("name", sorted(MODELS))
def test_end_to_end_matches_loop_and_oracle(graph, name):
    kind, dims, aggr, plan = MODELS[name]
    m, ref = make_model(kind, dims, aggr)
    fan = [15, 10]
    out = m.inference(graph.x, loader_of(graph, fan), DEV)
    assert models.last_inference_plan == plan
    assert out.shape == (N, dims[2]) and out.device == graph.x.device
    loop = m.inference(graph.x, Wrapped(loader_of(graph, fan)), DEV)
    assert models.last_inference_plan == ["loop"] * dims[3]
    with torch.no_grad():
        want = ref.inference(graph.x.cpu(), Wrapped(loader_of(graph, fan), "cpu"))
    d_loop = float((out - loop).abs().max())
    d_ref = float((out.cpu() - want).abs().max())
    d_lr = float((loop.cpu() - want).abs().max())
    bad = lambda a, b: int((~torch.isclose(a, b, **OUT_TOL)).sum())  # noqa: E731
    print(f"{name}: elements outside the bar: fused/loop {bad(out, loop)}, fused/oracle {bad(out.cpu(), want)}, "
          f"loop/oracle {bad(loop.cpu(), want)} of {want.numel()}")
    print(f"{name}: max |fused - loop| = {d_loop:.3e}, max |fused - oracle| = {d_ref:.3e}, "
          f"max |loop - oracle| = {d_lr:.3e}, max |out| = {float(want.abs().max()):.3e}")
    torch.testing.assert_close(out, loop, **OUT_TOL)
    torch.testing.assert_close(out.cpu(), want, **OUT_TOL)


def test_host_features_come_back_on_the_host(graph):
    m, _ = make_model(*MODELS["sage_mean"][:3])
    out = m.inference(graph.x.cpu(), loader_of(graph, [15, 10]), DEV)
    assert models.last_inference_plan == ["rowtile", "narrow"]
    assert out.device.type == "cpu"


# --------------------------------------------------------------- chunking
@pytest.mark.parametrize("name", ["sage_mean", "sage_sum3"])
def test_one_batch_per_chunk_matches_single_chunk(graph, name, monkeypatch):
    kind, dims, aggr, plan = MODELS[name]
    m, _ = make_model(kind, dims, aggr)
    one = m.inference(graph.x, loader_of(graph, [15, 10]), DEV)
    monkeypatch.setattr(infer, "_max_chunk_batches", 1)
    assert len(infer._chunks(N, BS, 256, 15)) == 5
    many = m.inference(graph.x, loader_of(graph, [15, 10]), DEV)
    assert models.last_inference_plan == plan
    torch.testing.assert_close(many, one, **OUT_TOL)


# ------------------------------------------------------- epoch accounting
def test_epoch_advances_as_iterating_would(graph):
    m, _ = make_model(*MODELS["sage_sum3"][:3])
    a, b = loader_of(graph, [15, 10]), loader_of(graph, [15, 10])
    a.epoch = b.epoch = 2
    m.inference(graph.x, a, DEV)
    assert models.last_inference_plan == MODELS["sage_sum3"][3]
    m.inference(graph.x, Wrapped(b), DEV)
    assert a.epoch == b.epoch == 2 + 3
    for p, q in zip(list(a), list(b), strict=True):
        assert torch.equal(p.n_id, q.n_id) and torch.equal(p.edge_index, q.edge_index)


# ------------------------------------------------------ ineligible inputs
def test_ineligible_loaders_run_the_loop_unchanged(graph):
    m, _ = make_model(*MODELS["sage_mean"][:3])
    perm = torch.randperm(N, generator=torch.Generator().manual_seed(4)).to(DEV)
    cases = {
        "shuffle": lambda: loader_of(graph, [15, 10], shuffle=True),
        "permuted": lambda: NeighborLoader(graph, perm, num_neighbors=[15, 10], batch_size=BS, seed=SEED),
        "list": lambda: list(loader_of(graph, [15, 10])),
    }
    for name, make in cases.items():
        out = m.inference(graph.x, make(), DEV)
        assert models.last_inference_plan == ["loop", "loop"], name
        want = models._layerwise_inference(m.convs, m.num_layers, graph.x, make(), DEV)
        assert torch.equal(out, want), name


@pytest.mark.parametrize("aggr,plan", [("mean", ["loop", "narrow"]), ("max", ["loop", "rowtile"])])
def test_k767_layer_runs_the_loop(graph, aggr, plan):
    """K = 767 is outside the row-tile kernel's envelope (K % 4 != 0): that
    layer alone takes the loop, in either plan."""
    torch.manual_seed(1)
    x = torch.randn(N, 767, device=DEV)
    m = ngnn.SAGE(767, 32, 8, 2, aggr=aggr).to(DEV).eval()
    out = m.inference(x, loader_of(graph, [15, 10]), DEV)
    assert models.last_inference_plan == plan
    want = m.inference(x, Wrapped(loader_of(graph, [15, 10])), DEV)
    assert models.last_inference_plan == ["loop", "loop"]
    torch.testing.assert_close(out, want, **OUT_TOL)
    # the layer that ran the loop computed exactly what the loop computes
    h_fused = infer._loop_layer(m.convs[0], x, loader_of(graph, [15, 10]), DEV, True)
    h_loop = models._layerwise_inference(m.convs[:1], 1, x, Wrapped(loader_of(graph, [15, 10])), DEV).relu()
    assert torch.equal(h_fused, h_loop)
