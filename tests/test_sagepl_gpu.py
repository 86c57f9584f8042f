"""ngnn.SAGEPL on the device: the reference's own fixtures
(tests/golden/sagepl_*.npz), its checkpoint keys, the NGNN factory, one
co-teaching step in the shape of PipelineTE.train_ct against the CPU
restatement (tests/sagepl_ref.py + oracle.losses_ref + torch.optim.Adam),
where dropout sits relative to the returned hidden state, layer-wise
inference, and what the model refuses."""
import pytest
import torch

import ngnn
from ngnn import models
from ngnn.loader import Graph, NeighborLoader, sample_block
from ngnn.losses import CTLoss
from ngnn.optim import Adam
from oracle.losses_ref import ct_loss

import sagepl_ref
from gradbar import assert_wgrad
from test_sagepl_cpu import CASES, load_case

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
TOL = dict(rtol=1e-5, atol=1e-5)


def small_graph(n, f, c, seed):
    g = torch.Generator().manual_seed(seed)
    degs = torch.randint(0, 9, (n,), generator=g)
    rowptr = torch.zeros(n + 1, dtype=torch.int64)
    rowptr[1:] = torch.cumsum(degs, 0)
    col = torch.randint(0, n, (int(rowptr[-1]),), generator=g).to(torch.int32)
    x = torch.randn(n, f, generator=g)
    y = torch.randint(0, c, (n,), generator=g)
    return Graph(rowptr.to(DEV), col.to(DEV), x.to(DEV), y.to(DEV), torch.arange(n, device=DEV), c)


# ------------------------------------------------------------------ fixtures
@pytest.mark.parametrize("name", sorted(CASES))
def test_reference_fixture(golden_dir, name):
    rec, state, n_id = load_case(golden_dir, name)
    nbr_nodes = state["noise"].shape[0]
    m = ngnn.SAGEPL(*CASES[name]["sizes"], nbr_nodes=nbr_nodes, dropout=0.0)
    m.load_state_dict(state, strict=True)
    m.to(DEV).eval()
    outs = m(torch.as_tensor(rec["x"]).to(DEV), torch.as_tensor(rec["edge_index"]).to(DEV),
             noise_rate=float(rec["noise_rate"]), n_id=None if n_id is None else n_id.to(DEV))
    assert len(outs) == 6
    for nm, o in zip(sagepl_ref.OUT_NAMES, outs):
        torch.testing.assert_close(o.detach().cpu(), torch.as_tensor(rec["out/" + nm]), msg=lambda s: f"{nm}: {s}",
                                   **TOL)
    sagepl_ref.fixture_loss(outs, rec).backward()
    rows = torch.arange(nbr_nodes) if n_id is None else n_id
    gn = m.noise.grad.cpu()
    rest = torch.ones(nbr_nodes, dtype=torch.bool)
    rest[rows] = False
    assert (gn[rest] == 0).all()
    got, want = gn[rows], torch.as_tensor(rec["grad/noise_rows"])
    clamped = want.abs().amax(dim=1) > 1e3  # the zero noise row: g * rate / 1e-12
    assert int(clamped.sum()) == (1 if name == "sagepl_block" else 0)
    for r in torch.nonzero(clamped).flatten().tolist():
        assert_wgrad(got[r], want[r], msg=f"noise row {r} (clamped)")
    assert_wgrad(got[~clamped], want[~clamped], msg="noise rows")
    for k, p in m.named_parameters():
        if k != "noise":
            assert_wgrad(p.grad, torch.as_tensor(rec["grad/" + k]), msg=k)


def test_reference_checkpoint_loads_strict(golden_dir):
    _, state, _ = load_case(golden_dir, "sagepl_block")
    want = {"noise"} | {f"convs.{i}.{p}" for i in range(3) for p in ("lin_l.weight", "lin_l.bias", "lin_r.weight")}
    assert set(state) == want
    m = ngnn.SAGEPL(100, 32, 47, 3, nbr_nodes=250).to(DEV)
    m.load_state_dict({k: v.to(DEV) for k, v in state.items()}, strict=True)
    assert torch.equal(m.noise.detach().cpu(), state["noise"])
    bn = ngnn.SAGEPL(8, 8, 3, 2, nbr_nodes=5, use_bn=True)
    assert {"bn1.weight", "bn2.running_var"} <= set(bn.state_dict())


def test_factory_builds_sagepl_and_adam_sees_noise():
    f = ngnn.NGNN(in_size=24, hidden_size=16, out_size=5, num_layers=2, module="sagePL", nbr_nodes=300)
    assert isinstance(f.network, ngnn.SAGEPL) and tuple(f.network.noise.shape) == (300, 24)
    held = {id(p) for grp in f.optimizer.param_groups for p in grp["params"]}
    assert id(f.network.noise) in held
    with pytest.raises(ValueError):
        ngnn.NGNN(module="sageFC")


# ------------------------------------------------------- one train_ct step
B, FAN, N_TAB, F_IN, HID, C = 16, [4, 3], 300, 24, 16, 5


def _ct_step(noisy_term: bool):
    g = small_graph(N_TAB, F_IN, C, seed=3)
    blk = sample_block(g, torch.randperm(N_TAB, generator=torch.Generator().manual_seed(4))[:B].to(DEV), FAN,
                       seed=9)
    gen = torch.Generator().manual_seed(6)
    y_noise = torch.randint(0, C, (N_TAB,), generator=gen)
    clean = torch.rand(N_TAB, generator=gen) < 0.7
    forget = 0.25
    gpu, cpu = [], []
    for s in (1, 2):
        torch.manual_seed(s)
        ref = sagepl_ref.SAGEPL(F_IN, HID, C, 2, nbr_nodes=N_TAB, dropout=0.0).train()
        m = ngnn.SAGEPL(F_IN, HID, C, 2, nbr_nodes=N_TAB, dropout=0.0)
        m.load_state_dict(ref.state_dict(), strict=True)
        gpu.append(m.to(DEV).train())
        cpu.append(ref)
    opts = [Adam(m.parameters(), lr=1e-3) for m in gpu]
    ropts = [torch.optim.Adam(r.parameters(), lr=1e-3) for r in cpu]
    before = [m.noise.detach().clone() for m in gpu]
    # the device step
    outs = [m(blk.x, blk.edge_index, noise_rate=0.1, n_id=blk.n_id) for m in gpu]
    res = CTLoss(DEV)(outs[0][2][:B], outs[1][2][:B], y_noise.to(DEV)[blk.n_id[:B]], forget, blk.n_id[:B],
                      clean.to(DEV))
    losses = [res[i] + 0.1 * outs[i][3].mean() if noisy_term else res[i] for i in range(2)]
    for o, l in zip(opts, losses):
        o.zero_grad()
        l.backward()
    grads_none = [m.noise.grad is None for m in gpu]
    for o in opts:
        o.step()
    torch.cuda.synchronize()
    # the CPU step
    x, ei, n_id = blk.x.cpu(), blk.edge_index.cpu(), blk.n_id.cpu()
    routs = [r(x, ei, noise_rate=0.1, n_id=n_id) for r in cpu]
    rres = ct_loss(routs[0][2][:B], routs[1][2][:B], y_noise[n_id[:B]], forget, n_id[:B], clean)
    rlosses = [rres[i] + 0.1 * routs[i][3].mean() if noisy_term else rres[i] for i in range(2)]
    for o, l in zip(ropts, rlosses):
        o.zero_grad()
        l.backward()
        o.step()
    return gpu, cpu, losses, rlosses, before, grads_none


def test_train_ct_step_matches_cpu():
    gpu, cpu, losses, rlosses, before, grads_none = _ct_step(noisy_term=True)
    assert grads_none == [False, False]
    for i in range(2):
        got, want = float(losses[i].detach()), float(rlosses[i].detach())
        print(f"model {i + 1}: loss {got:.7f} (cpu {want:.7f})")
        assert abs(got - want) <= 1e-5
        for (k, p), (_, q) in zip(gpu[i].named_parameters(), cpu[i].named_parameters()):
            d = float((p.detach().cpu() - q.detach()).abs().max())
            print(f"model {i + 1} {k}: max |p - p_cpu| after the step = {d:.3e}")
            torch.testing.assert_close(p.detach().cpu(), q.detach(), msg=lambda s: f"model {i + 1} {k}: {s}", **TOL)
        assert not torch.equal(gpu[i].noise.detach(), before[i])  # the table trained


def test_pure_only_loss_leaves_noise_alone():
    """The reference's first ct_tk epochs: the loss reads z_pure only."""
    gpu, cpu, losses, rlosses, before, grads_none = _ct_step(noisy_term=False)
    assert grads_none == [True, True]
    for i in range(2):
        assert abs(float(losses[i].detach()) - float(rlosses[i].detach())) <= 1e-5
        assert torch.equal(gpu[i].noise.detach(), before[i])
        for (k, p), (_, q) in zip(gpu[i].named_parameters(), cpu[i].named_parameters()):
            torch.testing.assert_close(p.detach().cpu(), q.detach(), msg=lambda s: f"model {i + 1} {k}: {s}", **TOL)


# ----------------------------------------------------------------- dropout
def test_hidden_state_is_returned_before_dropout():
    g = small_graph(200, 24, C, seed=7)
    blk = sample_block(g, torch.arange(32, device=DEV), FAN, seed=2)
    torch.manual_seed(5)
    m = ngnn.SAGEPL(24, 32, C, 2, nbr_nodes=200, dropout=0.5).to(DEV)
    m.eval()
    ev = m(blk.x, blk.edge_index, noise_rate=0.1, n_id=blk.n_id)
    m.train()
    tr = m(blk.x, blk.edge_index, noise_rate=0.1, n_id=blk.n_id)
    for i in (0, 3):  # h: no element rescaled or dropped
        torch.testing.assert_close(tr[i], ev[i], rtol=1e-6, atol=1e-6)
        assert float(ev[i].detach().abs().max()) > 0
    for i in (2, 5):  # z: computed from the dropped-out hidden state
        assert not torch.allclose(tr[i], ev[i], rtol=1e-3, atol=1e-3)
    for i in (1, 4):
        torch.testing.assert_close(tr[i], torch.log_softmax(tr[i + 1], 1), **TOL)


# --------------------------------------------------------------- inference
def test_inference_is_sages_bitwise():
    g = small_graph(300, 100, 47, seed=8)
    torch.manual_seed(1)
    pl = ngnn.SAGEPL(100, 64, 47, 2, nbr_nodes=300).to(DEV).eval()
    sage = ngnn.SAGE(100, 64, 47, 2).to(DEV).eval()
    sage.load_state_dict({k: v for k, v in pl.state_dict().items() if k != "noise"}, strict=True)
    mk = lambda: NeighborLoader(g, None, num_neighbors=[15, 10], batch_size=64, seed=5)  # noqa: E731
    want = sage.inference(g.x, mk(), DEV)
    plan = list(models.last_inference_plan)
    models.last_inference_plan[:] = []
    got = pl.inference(g.x, mk(), DEV)
    assert models.last_inference_plan == plan and len(plan) == 2
    assert got.shape == (300, 47) and torch.equal(got, want)


# ---------------------------------------------------------------- refusals
def test_refusals():
    with pytest.raises(ValueError, match="num_layers"):
        ngnn.SAGEPL(8, 8, 3, 1, nbr_nodes=10)
    g = small_graph(200, 24, C, seed=7)
    blk = sample_block(g, torch.arange(16, device=DEV), FAN, seed=2)
    m = ngnn.SAGEPL(24, 16, C, 2, nbr_nodes=200).to(DEV)
    with pytest.raises((ValueError, ngnn._lib.NGNNError)):  # n_id=None: x must have the table's rows
        assert blk.x.size(0) != 200
        m(blk.x, blk.edge_index)
    half = ngnn.SAGEPL(24, 16, C, 2, nbr_nodes=200).to(DEV)
    half.noise.data = half.noise.data.bfloat16()
    with pytest.raises((ValueError, ngnn._lib.NGNNError)):
        half(blk.x, blk.edge_index, n_id=blk.n_id)
    sf = list(NeighborLoader(g, g.train_idx, FAN, batch_size=64, sync_free=True))[0]
    with pytest.raises(ValueError, match="sync_free"):
        m(sf.x, sf.edge_index, n_id=sf.n_id)
