"""GPU checks of the fused ReLU-BatchNorm-dropout kernels and of the models
that run on them (``ngnn.ops.batch_norm_act``; include/ngnn.h).

Bars: plain ``randn`` columns against the float64 restatement (tests/bn_ref.py)
at the project's output bar (rtol = atol = 1e-5) and gradient bars (dx: rtol
1e-4 / atol 1e-5; dgamma, dbeta: tests/gradbar.py).  The columns whose error
cancellation decides -- (i) randn + 4096, (ii) randn * 1e-3 + 100, (iii)
constant -- follow the rule pinned by tests/test_bn_ref_cpu.py: per-column
error <= max(1e-5, 2 * e_torch), e_torch the error of torch's own fp32 CPU
BatchNorm on the same input.  Dropout is checked element for element against
the host replica of the hash RNG.
"""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import bn_ref
import ngnn
import sagepl_ref
from gradbar import assert_wgrad
from ngnn import _lib, fused, ops
from oracle import pyg_ref

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
OUT = dict(rtol=1e-5, atol=1e-5)
GRAD = dict(rtol=1e-4, atol=1e-5)
EPS = 1e-5
S = _lib.load().ngnn_bn_slab_rows()
SHAPES = [(2, 8), (63, 37), (777, 37), (3 * S + 5, 100), (S + 1, 256), (130, 767)]
SEED = 0x1234_5678_9ABC_DEF


def params(f, seed=1):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(f, generator=g) + 0.5, torch.randn(f, generator=g)


def fwd_train(x, gamma, beta, relu, p=0.0, seed=0, momentum=0.1, state=None):
    """ngnn_bn_fwd_train on the device view `x` (its stride is the leading
    dimension): (out, mean, invstd, (running_mean, running_var, nbt))."""
    lib = _lib.load()
    n, f = x.shape
    rm, rv, nbt = state or (torch.zeros(f, device=DEV), torch.ones(f, device=DEV),
                            torch.zeros((), dtype=torch.int64, device=DEV))
    out = torch.full((n, f), float("nan"), device=DEV)
    mean, mean_lo, invstd = torch.empty(f, device=DEV), torch.empty(f, device=DEV), torch.empty(f, device=DEV)
    nb = lib.ngnn_bn_workspace_bytes(n, f)
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    g, b = gamma.to(DEV), beta.to(DEV)
    rc = lib.ngnn_bn_fwd_train(x.data_ptr(), x.stride(0), n, f, int(relu), g.data_ptr(), b.data_ptr(), EPS,
                               momentum, rm.data_ptr(), rv.data_ptr(), nbt.data_ptr(), p, seed, None,
                               out.data_ptr(), f, mean.data_ptr(), mean_lo.data_ptr(), invstd.data_ptr(), ws.data_ptr(), nb,
                               _lib.stream_handle(DEV))
    _lib.check(rc, "ngnn_bn_fwd_train")
    torch.cuda.synchronize()
    return out.cpu(), mean.cpu(), invstd.cpu(), (rm, rv, nbt)


def torch_fp32(x, gamma, beta, relu):
    """torch's own fp32 CPU batch norm: (out, save_mean, save_invstd)."""
    a = torch.relu(x) if relu else x
    return torch.native_batch_norm(a, gamma, beta, None, None, True, 0.1, EPS)


def check_forward(got, x, gamma, beta, relu, hard, plain):
    want = bn_ref.forward(x, gamma, beta, EPS, relu)[:3]
    base = torch_fp32(x, gamma, beta, relu)
    for what, g, w, b in zip(("out", "mean", "invstd"), got, want, base):
        print(what, "plain max err", float(bn_ref.col_err(g, w)[plain].max()) if plain else 0.0)
        torch.testing.assert_close(g.double()[..., plain], w[..., plain], **OUT, msg=lambda m: f"{what}: {m}")
        if hard:
            e, bar = bn_ref.col_err(g, w)[hard], bn_ref.column_bar(bn_ref.col_err(b, w))[hard]
            print(what, "hard err", e.tolist(), "bar", bar.tolist())
            assert bool((e <= bar).all()), (what, e.tolist(), bar.tolist())
    if relu and x.size(1) >= 5:  # class (iv): variance 0 after the ReLU, the output is beta
        assert torch.equal(got[0][:, bn_ref.ALL_NEG], beta[bn_ref.ALL_NEG].expand(x.size(0)))


def columns(x, hard, plain, relu):
    """The all-negative column is an ordinary column without the ReLU."""
    return hard, (plain + [bn_ref.ALL_NEG] if (not relu and x.size(1) >= 5) else plain)


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_forward_training(shape, relu):
    x, hard, plain = bn_ref.probe_input(*shape)
    gamma, beta = params(shape[1])
    got = fwd_train(x.to(DEV), gamma, beta, relu)[:3]
    check_forward(got, x, gamma, beta, relu, *columns(x, hard, plain, relu))


@pytest.mark.parametrize("shape", [(777, 37), (3 * S + 5, 100)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_forward_training_on_a_column_slice(shape):
    n, f = shape
    x, hard, plain = bn_ref.probe_input(n, f)
    wide = torch.full((n, f + 3), float("nan"))
    wide[:, :f] = x
    xs = wide.to(DEV)[:, :f]  # ldx = F + 3
    assert xs.stride(0) == f + 3
    gamma, beta = params(f)
    check_forward(fwd_train(xs, gamma, beta, 1)[:3], x, gamma, beta, 1, hard, plain)


@pytest.mark.parametrize("p", [0.5, 0.25, 0.9])
@pytest.mark.parametrize("shape", [(777, 37), (3 * S + 5, 100)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_dropout_matches_the_replica_element_for_element(shape, p):
    x, hard, plain = bn_ref.probe_input(*shape)
    gamma, beta = params(shape[1])
    beta = beta.abs() + 0.1  # (no output is zero by itself: the zeros are the mask's)
    out = fwd_train(x.to(DEV), gamma, beta, 1, p=p, seed=SEED)[0]
    keep, scale = bn_ref.dropout_keep(SEED, *shape, p), bn_ref.dropout_scale(p)
    want = bn_ref.forward(x, gamma, beta, EPS, True, keep, scale)[0]
    assert torch.equal(out[~keep], torch.zeros(int((~keep).sum()))) and not torch.signbit(out[~keep]).any()
    assert 0 < int(keep.sum()) < keep.numel()
    cols = plain + [bn_ref.ALL_NEG]
    assert bool((out[:, cols] != 0).eq(keep[:, cols]).all())
    torch.testing.assert_close(out.double()[:, plain], want[:, plain], **OUT)
    # the hard columns: torch's fp32 output under the same mask is the yardstick
    base = torch.where(keep, torch_fp32(x, gamma, beta, True)[0].double() * scale, torch.zeros(shape).double())
    bar = bn_ref.column_bar(bn_ref.col_err(base, want))[hard]
    e = bn_ref.col_err(out, want)[hard]
    assert bool((e <= bar).all()), (e.tolist(), bar.tolist())


def test_dropout_of_everything_is_positive_zero():
    x, _, _ = bn_ref.probe_input(63, 37)
    out = fwd_train(x.to(DEV), *params(37), 1, p=1.0, seed=SEED)[0]
    assert torch.equal(out, torch.zeros(63, 37)) and not torch.signbit(out).any()


def make_bn(f, momentum=0.1, seed=1):
    bn = nn.BatchNorm1d(f, eps=EPS, momentum=momentum)
    gamma, beta = params(f, seed)
    with torch.no_grad():
        bn.weight.copy_(gamma)
        bn.bias.copy_(beta)
    return bn


def clone_bn(bn, to):
    other = nn.BatchNorm1d(bn.num_features, eps=bn.eps, momentum=bn.momentum)
    other.load_state_dict(bn.state_dict())
    return other.to(to).train(bn.training)


@pytest.mark.parametrize("momentum", [0.1, None])
def test_running_statistics_over_three_calls(momentum):
    n, f = 3 * S + 5, 37
    cpu32 = make_bn(f, momentum)
    dev, cpu64 = clone_bn(cpu32, DEV), clone_bn(cpu32, "cpu").double()
    hard = plain = None
    for call in range(3):
        x, hard, plain = bn_ref.probe_input(n, f, seed=10 + call)
        x = x * (1.0 + call)
        assert ops.batch_norm_act_supported(x.to(DEV), dev, True)
        ops.batch_norm_act(x.to(DEV), dev, relu=True)
        cpu32(x.relu())
        cpu64(x.double().relu())
    torch.cuda.synchronize()
    assert int(dev.num_batches_tracked) == 3 == int(cpu64.num_batches_tracked)
    cols = plain + [bn_ref.ALL_NEG]
    for name in ("running_mean", "running_var"):
        got, want, base = getattr(dev, name).cpu(), getattr(cpu64, name), getattr(cpu32, name)
        print(name, "max rel err", float(((got.double() - want).abs() / want.abs().clamp_min(1e-30))[cols].max()))
        torch.testing.assert_close(got.double()[cols], want[cols], rtol=1e-5, atol=1e-8)
        e, bar = bn_ref.col_err(got, want)[hard], bn_ref.column_bar(bn_ref.col_err(base, want))[hard]
        assert bool((e <= bar).all()), (name, e.tolist(), bar.tolist())


@pytest.mark.parametrize("shape", [(1, 8), (777, 37), (S + 1, 256)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_eval_mode(shape):
    n, f = shape
    g = torch.Generator().manual_seed(3)
    x = torch.randn(n, f, generator=g)
    bn = make_bn(f).eval()
    with torch.no_grad():
        bn.running_mean.copy_(torch.randn(f, generator=g))
        bn.running_var.copy_(torch.rand(f, generator=g) + 0.25)
        bn.num_batches_tracked.fill_(5)
    dev = clone_bn(bn, DEV)
    before = {k: v.clone() for k, v in dev.state_dict().items()}
    with torch.no_grad():
        assert ops.batch_norm_act_supported(x.to(DEV), dev, False)
        out = ops.batch_norm_act(x.to(DEV), dev, relu=True, p=0.5)  # eval: no dropout
        again = ops.batch_norm_act(x.to(DEV), dev, relu=True, p=0.5)
    want = clone_bn(bn, "cpu").double()(x.double().relu()).detach()
    torch.testing.assert_close(out.cpu().double(), want, **OUT)
    assert torch.equal(out, again)
    for k, v in dev.state_dict().items():
        assert torch.equal(v, before[k]), k


def run_op(x, bn, relu, p, seed, dout, need_dx=True):
    """forward + backward of the op on the device: (out, dx, dgamma, dbeta)."""
    xd = x.to(DEV).requires_grad_(need_dx)
    bn.zero_grad()
    out = ops.batch_norm_act(xd, bn, relu=relu, p=p, seed=seed)
    out.backward(dout.to(DEV))
    torch.cuda.synchronize()
    return out.detach().cpu(), (xd.grad.cpu() if need_dx else xd.grad), bn.weight.grad.cpu(), bn.bias.grad.cpu()


def torch_fp32_backward(x, gamma, beta, relu, keep, scale, dout):
    xr = x.clone().requires_grad_(True)
    ga, be = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    y = F.batch_norm(xr.relu() if relu else xr, None, None, ga, be, True, 0.1, EPS)
    (y * keep * scale).backward(dout)
    return xr.grad, ga.grad, be.grad


@pytest.mark.parametrize("p", [0.0, 0.5])
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("shape", [(777, 37), (3 * S + 5, 100)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_backward(shape, relu, p):
    n, f = shape
    x, hard, plain = bn_ref.probe_input(n, f)
    hard, plain = columns(x, hard, plain, relu)
    if relu:
        plain = plain + [bn_ref.ALL_NEG]  # (iv): dx and dgamma are exactly 0, dbeta an ordinary sum
    bn = make_bn(f).to(DEV)
    gamma, beta = params(f)
    dout = torch.randn(n, f, generator=torch.Generator().manual_seed(4))
    keep, scale = bn_ref.dropout_keep(SEED, n, f, p), (bn_ref.dropout_scale(p) if p else 1.0)
    got = run_op(x, bn, relu, p, SEED, dout)[1:]
    want = bn_ref.backward(dout, x, gamma, EPS, relu, keep, scale)
    base = torch_fp32_backward(x, gamma, beta, relu, keep, scale, dout)
    torch.testing.assert_close(got[0].double()[:, plain], want[0][:, plain], **GRAD)
    assert_wgrad(got[1][plain], want[1][plain], "dgamma")
    assert_wgrad(got[2][plain], want[2][plain], "dbeta")
    for what, g, w, b in zip(("dx", "dgamma", "dbeta"), got, want, base):
        e, bar = bn_ref.col_err(g, w)[hard], bn_ref.column_bar(bn_ref.col_err(b, w))[hard]
        print(what, "hard err", e.tolist(), "bar", bar.tolist())
        assert bool((e <= bar).all()), (what, e.tolist(), bar.tolist())
    # the dx-skipped form: an input that needs no gradient
    _, dx, dgamma, dbeta = run_op(x, bn, relu, p, SEED, dout, need_dx=False)
    assert dx is None
    assert torch.equal(dgamma, got[1]) and torch.equal(dbeta, got[2])


def test_a_nan_stays_in_its_column():
    n, f, col = 777, 37, 7
    x = torch.randn(n, f, generator=torch.Generator().manual_seed(5))
    x[5, col] = float("nan")
    dout = torch.randn(n, f, generator=torch.Generator().manual_seed(6))
    cpu = make_bn(f)
    dev = clone_bn(cpu, DEV)
    out, dx, dgamma, dbeta = run_op(x, dev, True, 0.0, 0, dout)
    xr = x.clone().requires_grad_(True)
    ref = cpu(xr.relu())
    ref.backward(dout)
    pairs = dict(out=(out, ref.detach()), dx=(dx, xr.grad), dgamma=(dgamma, cpu.weight.grad),
                 dbeta=(dbeta, cpu.bias.grad), running_mean=(dev.running_mean.cpu(), cpu.running_mean),
                 running_var=(dev.running_var.cpu(), cpu.running_var))
    for name, (g, w) in pairs.items():
        assert torch.equal(torch.isnan(g), torch.isnan(w)), name
    assert torch.isnan(out[:, col]).all() and torch.isnan(dev.running_mean[col])
    rest = [c for c in range(f) if c != col]
    gamma, beta = params(f)
    want = bn_ref.forward(x, gamma, beta, EPS, True)[0]
    wdx, wdg, wdb = bn_ref.backward(dout, x, gamma, EPS, True)
    torch.testing.assert_close(out.double()[:, rest], want[:, rest], **OUT)
    torch.testing.assert_close(dx.double()[:, rest], wdx[:, rest], **GRAD)
    assert_wgrad(dgamma[rest], wdg[rest], "dgamma")
    assert_wgrad(dbeta[rest], wdb[rest], "dbeta")


def test_two_runs_are_bitwise_equal():
    n, f = 3 * S + 5, 100
    x, _, _ = bn_ref.probe_input(n, f)
    dout = torch.randn(n, f, generator=torch.Generator().manual_seed(7))
    runs = []
    for _ in range(2):
        bn = make_bn(f).to(DEV)
        res = run_op(x, bn, True, 0.5, SEED, dout)
        stats = fwd_train(x.to(DEV), *params(f), 1, p=0.5, seed=SEED)[:3]
        runs.append(list(res) + list(stats) + [bn.running_mean.cpu(), bn.running_var.cpu(),
                                               bn.num_batches_tracked.cpu()])
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    assert torch.equal(runs[0][0], runs[0][4])  # the op and the bare entry agree


# ---- the models ----

def rand_edges(seed, n, e):
    ei = torch.randint(0, n, (2, e), generator=torch.Generator().manual_seed(seed))
    return ei[:, torch.argsort(ei[1], stable=True)]


def sage_pair():
    torch.manual_seed(0)
    ref = pyg_ref.SAGE(16, 32, 5, 2, dropout=0.0, use_bn=True)
    with torch.no_grad():  # non-trivial BatchNorm parameters
        for bn in (ref.bn1, ref.bn2):
            bn.weight.uniform_(0.5, 1.5)
            bn.bias.normal_()
    mine = ngnn.SAGE(16, 32, 5, 2, dropout=0.0, use_bn=True)
    mine.load_state_dict(ref.state_dict(), strict=True)
    return ref.double(), mine.to(DEV)


def raising(*a, **k):
    raise AssertionError("torch's batch_norm was called")


def test_sage_training_matches_the_oracle(monkeypatch):
    ref, mine = sage_pair()
    x = torch.randn(300, 16, generator=torch.Generator().manual_seed(1))
    ei = rand_edges(2, 300, 2000)
    G = torch.randn(300, 5, generator=torch.Generator().manual_seed(3))
    want = ref.train()(x.double(), ei)
    (want * G).sum().backward()
    with monkeypatch.context() as mp:  # route: forward and backward run without torch's batch norm
        mp.setattr(F, "batch_norm", raising)
        out = mine.train()(x.to(DEV), ei.to(DEV))
        (out * G.to(DEV)).sum().backward()
        torch.cuda.synchronize()
    torch.testing.assert_close(out.detach().cpu().double(), want.detach(), **OUT)
    got = dict(mine.named_parameters())
    for k, q in ref.named_parameters():
        assert got[k].grad is not None, k
        assert_wgrad(got[k].grad, q.grad, k)
    bufs = dict(mine.named_buffers())
    for k, b in ref.named_buffers():
        torch.testing.assert_close(bufs[k].cpu().double(), b.double(), rtol=1e-5, atol=1e-7, msg=lambda m: f"{k}: {m}")
    # eval mode on the moved buffers
    with torch.no_grad():
        want_ev = ref.eval()(x.double(), ei)
        with monkeypatch.context() as mp:
            mp.setattr(F, "batch_norm", raising)
            ev = mine.eval()(x.to(DEV), ei.to(DEV))
    torch.testing.assert_close(ev.cpu().double(), want_ev, **OUT)


def test_sage_dropout_draws_a_fresh_mask_per_step_from_torchs_seed():
    x = torch.randn(300, 16, generator=torch.Generator().manual_seed(1)).to(DEV)
    ei = rand_edges(2, 300, 2000).to(DEV)
    torch.manual_seed(0)
    m = ngnn.SAGE(16, 32, 5, 3, dropout=0.5, use_bn=True).to(DEV).train()
    torch.manual_seed(11)
    a, b = m(x, ei).detach().clone(), m(x, ei).detach().clone()
    torch.manual_seed(11)
    c = m(x, ei).detach()
    assert not torch.equal(a, b) and torch.equal(a, c)
    # the hidden activations are dropped at the hash RNG's rate
    h = ops.batch_norm_act(m.convs[0](ops.batch_norm_act(x, m.bn1), ngnn.get_block(ei, 300)), m.bn2, relu=True,
                           p=0.5, seed=int(torch.randint(0, 1 << 62, (1,)).item()))
    assert 0.4 < float((h == 0).float().mean()) < 0.6


def test_sagepl_matches_its_restatement(monkeypatch):
    torch.manual_seed(0)
    ref = sagepl_ref.SAGEPL(16, 32, 5, 2, nbr_nodes=300, dropout=0.0, use_bn=True).train()
    mine = ngnn.SAGEPL(16, 32, 5, 2, nbr_nodes=300, dropout=0.0, use_bn=True).train()
    mine.load_state_dict(ref.state_dict(), strict=True)
    ref, mine = ref.double(), mine.to(DEV)
    x = torch.randn(300, 16, generator=torch.Generator().manual_seed(1))
    ei = rand_edges(2, 300, 2000)
    n_id = torch.randperm(300, generator=torch.Generator().manual_seed(3))
    G1 = torch.randn(300, 32, generator=torch.Generator().manual_seed(4))
    G3 = torch.randn(300, 5, generator=torch.Generator().manual_seed(5))
    want = ref(x.double(), ei, noise_rate=0.1, n_id=n_id)
    ((want[3] * G1).sum() + (want[2] * G3).sum()).backward()
    monkeypatch.setattr(F, "batch_norm", raising)
    outs = mine(x.to(DEV), ei.to(DEV), noise_rate=0.1, n_id=n_id.to(DEV))
    assert outs[0].requires_grad  # h is a tensor with a gradient
    ((outs[3] * G1.to(DEV)).sum() + (outs[2] * G3.to(DEV)).sum()).backward()
    got = dict(mine.named_parameters())
    for k, q in ref.named_parameters():
        assert_wgrad(got[k].grad, q.grad, k)
    for name, o, w in zip(sagepl_ref.OUT_NAMES, outs, want):
        torch.testing.assert_close(o.detach().cpu().double(), w.detach(), **OUT, msg=lambda m: f"{name}: {m}")
    bufs = dict(mine.named_buffers())
    for k, b in ref.named_buffers():  # after the double update, pure pass first
        torch.testing.assert_close(bufs[k].cpu().double(), b.double(), rtol=1e-5, atol=1e-7, msg=lambda m: f"{k}: {m}")
    assert int(mine.bn1.num_batches_tracked) == 2 == int(mine.bn2.num_batches_tracked)


def test_routes(monkeypatch):
    x = torch.randn(300, 16, generator=torch.Generator().manual_seed(1)).to(DEV)
    ei = rand_edges(2, 300, 2000).to(DEV)
    # use_bn=False still takes the fused stack
    plain = ngnn.SAGE(16, 32, 5, 2, dropout=0.0).to(DEV).train()
    calls = []
    real = fused.sage_stack
    monkeypatch.setattr(fused, "sage_stack", lambda *a, **k: calls.append(1) or real(*a, **k))
    plain(x, ei).sum().backward()
    assert calls == [1]
    bnm = ngnn.SAGE(16, 32, 5, 2, dropout=0.0, use_bn=True).to(DEV).train()
    bnm(x, ei).sum().backward()
    assert calls == [1]  # (use_bn=True does not)
    # a bf16 input still reaches torch's batch norm
    seen = []
    real_bn = F.batch_norm
    monkeypatch.setattr(F, "batch_norm", lambda *a, **k: seen.append(a[0].dtype) or real_bn(*a, **k))
    bn = nn.BatchNorm1d(16).to(DEV).to(torch.bfloat16)
    xb = x.to(torch.bfloat16)
    assert not ops.batch_norm_act_supported(xb, bn, True)
    out = ops.batch_norm_act(xb, bn, relu=True, p=0.0)
    assert seen == [torch.bfloat16] and out.dtype == torch.bfloat16
    # one row has no batch statistics: a ValueError, as torch's
    with pytest.raises(ValueError):
        ops.batch_norm_act(x[:1], nn.BatchNorm1d(16).to(DEV))
