"""The fixed-order sums of the loss kernels, bit for bit against a numpy fp32
restatement of the order their comments state (csrc/ngnn_rows.h block_sum):
thread t of 256 adds its terms t, t + 256, ... in ascending order, then a
halving tree over the threads; the one-launch ngnn_seed_xent_fwd_grad first
adds each workgroup's four rows as ((w0 + w1) + w2) + w3 and then the
workgroup sums the same way; one division at the end.

The inputs make every row term exact in fp32, so the order of the additions
is the only freedom: logits (0, -d) with label 1 and d in [128, 256) give
expf(-d) = 0, lse = 0 and the row loss d itself (23 random mantissa bits);
fix_cr(name='l2') with C = 1 gets differences of 11 significant bits, whose
squares are exact."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SIZES = [1, 255, 256, 257, 1000]
IGNORE = -100
f32 = np.float32


def _block_sum(terms):
    """csrc/ngnn_rows.h block_sum<256> of fp32 terms, in fp32.  (A thread with
    fewer terms adds nothing for the missing ones; adding +0 changes no sum
    that started at +0.)"""
    terms = np.asarray(terms, dtype=f32)
    rows = np.zeros((-(-max(terms.size, 1) // 256)) * 256, dtype=f32)
    rows[:terms.size] = terms
    acc = np.zeros(256, dtype=f32)
    for chunk in rows.reshape(-1, 256):
        acc = acc + chunk
    h = 128
    while h:
        acc[:h] = acc[:h] + acc[h:2 * h]
        h //= 2
    return acc[0]


def _xent_case(B, ignored):
    rng = np.random.default_rng(1000 + B)
    d = (np.uint32(0x43000000) | rng.integers(0, 1 << 23, B).astype(np.uint32)).view(f32)  # [128, 256)
    assert d.min() >= 128 and d.max() < 256
    x = np.zeros((B, 2), dtype=f32)
    x[:, 1] = -d
    y = np.ones(B, dtype=np.int64)
    if ignored:
        y[2::5] = IGNORE
    valid = (y != IGNORE).astype(f32)
    return x, y, d * valid, valid


def _bits(v):
    return np.asarray(v, dtype=f32).view(np.int32)


def _call_xent(B, x, y, with_grad):
    from ngnn import _lib as L
    lib = L.load()
    xd, yd = torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV)
    loss = torch.full((), -1.0, device=DEV)
    count = torch.full((), -1.0, device=DEV)
    ws = torch.zeros(lib.ngnn_seed_xent_workspace_bytes(B), dtype=torch.uint8, device=DEV)
    st = L.stream_handle(DEV)
    if with_grad:
        dx = torch.zeros(B, 2, device=DEV)
        L.check(lib.ngnn_seed_xent_fwd_grad(L.ptr(xd), 2, B, 2, L.ptr(yd), IGNORE, L.ptr(loss), L.ptr(count),
                                            L.ptr(dx), 2, L.ptr(ws), ws.numel(), st), "ngnn_seed_xent_fwd_grad")
    else:
        L.check(lib.ngnn_seed_xent_fwd(L.ptr(xd), 2, B, 2, L.ptr(yd), IGNORE, L.ptr(loss), L.ptr(count),
                                       L.ptr(ws), ws.numel(), st), "ngnn_seed_xent_fwd")
    return loss.cpu().numpy(), count.cpu().numpy()


@pytest.mark.parametrize("ignored", [False, True])
@pytest.mark.parametrize("B", SIZES)
def test_seed_xent_fwd_sum_order(B, ignored):
    x, y, terms, valid = _xent_case(B, ignored)
    loss, count = _call_xent(B, x, y, with_grad=False)
    want_n = _block_sum(valid)
    want = f32(_block_sum(terms) / want_n)
    print(f"B={B} ignored={ignored}: loss {loss!r} want {want!r}; count {count!r} want {want_n!r}")
    assert _bits(count) == _bits(want_n) and want_n == valid.sum()
    assert _bits(loss) == _bits(want)


@pytest.mark.parametrize("ignored", [False, True])
@pytest.mark.parametrize("B", SIZES)
def test_seed_xent_fwd_grad_sum_order(B, ignored):
    x, y, terms, valid = _xent_case(B, ignored)
    loss, count = _call_xent(B, x, y, with_grad=True)
    want_n = _block_sum(valid)
    w = np.zeros(-(-B // 4) * 4, dtype=f32)
    w[:B] = terms  # (a wave past the last row adds 0)
    w = w.reshape(-1, 4)
    groups = ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]
    want = f32(_block_sum(groups) / want_n)
    print(f"B={B} ignored={ignored}: loss {loss!r} want {want!r}; count {count!r} want {want_n!r}")
    assert _bits(count) == _bits(want_n)
    assert _bits(loss) == _bits(want)


@pytest.mark.parametrize("B", SIZES)
def test_fix_cr_l2_sum_order(B):
    from ngnn.losses import fix_cr
    rng = np.random.default_rng(2000 + B)
    d = rng.integers(1024, 2048, B).astype(f32) * rng.choice(np.array([-1, 1], dtype=f32), B)  # 11 bits each
    yp = rng.integers(-8, 8, B).astype(f32)  # (small integers: yn - yp is exact)
    yn = yp + d
    assert np.array_equal(yn - yp, d)
    loss = fix_cr(torch.from_numpy(yp[:, None]).to(DEV), torch.from_numpy(yn[:, None]).to(DEV), batch_size=B,
                  name="l2").cpu().numpy()
    want = f32(_block_sum(d * d) / (f32(B) * f32(1)))
    print(f"B={B}: loss {loss!r} want {want!r}")
    assert _bits(loss) == _bits(want)
