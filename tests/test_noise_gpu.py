"""ngnn.ops.add_node_noise (ngnn_node_noise_fwd / _bwd) against the torch
composition x + [sign(x) *] F.normalize(noise[n_id]) * rate evaluated on the
CPU: forward, dx and the dense table gradient at the fp32 bar (rtol = atol =
1e-5; the clamped-norm rows' gradients, about 1e10, at 1e-5 of their own
maximum), rows not named by n_id exactly zero; the deterministic mode; the
bounds guard; stream capture."""
import pytest
import torch

import ngnn
from ngnn import _lib
from ngnn.ops import add_node_noise, node_noise_bad_ids

from sagepl_ref import noisy_input

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
RATE = 0.1
ZERO_ROW, TINY_ROW = 3, 7  # table rows on the clamped-norm branch


def make_table(n_nodes, F, seed):
    g = torch.Generator().manual_seed(seed)
    t = torch.randn(n_nodes, F, generator=g)
    if n_nodes > TINY_ROW:
        t[ZERO_ROW] = 0.0
        t[TINY_ROW] *= 1e-20
    return t


def check_table_grad(got, ref, ids, msg):
    """got / ref: dense [n_nodes, F] (CPU); ids: the rows named."""
    named = torch.zeros(ref.size(0), dtype=torch.bool)
    named[ids] = True
    assert (got[~named] == 0).all(), f"{msg}: a row outside n_id was written"
    assert torch.isfinite(got).all(), msg
    big = ref.abs().amax(dim=1) > 1e3  # the clamped rows: g * rate / 1e-12
    for r in torch.nonzero(big).flatten().tolist():
        m = float(ref[r].abs().max())
        assert float((got[r] - ref[r]).abs().max()) <= 1e-5 * m, f"{msg}: clamped row {r}"
    torch.testing.assert_close(got[~big], ref[~big], rtol=1e-5, atol=1e-5, msg=lambda s: f"{msg}: {s}")


def run_case(x, table, ids, sign, msg, x_dev=None):
    """One forward + backward on the GPU and on the CPU.  x_dev: the device
    x to use (a strided view), else x.to(DEV)."""
    g = torch.Generator().manual_seed(5)
    G = torch.randn(x.shape, generator=g)
    xr, tr = x.clone().requires_grad_(True), table.clone().requires_grad_(True)
    ref = noisy_input(xr, tr, RATE, None if sign else ids)
    (ref * G).sum().backward()
    xd = (x.to(DEV) if x_dev is None else x_dev).detach().requires_grad_(True)
    td = table.to(DEV).requires_grad_(True)
    out = add_node_noise(xd, td, None if sign else ids.to(DEV), rate=RATE, sign=sign)
    assert out.data_ptr() != xd.data_ptr() and out.is_contiguous()
    (out * G.to(DEV)).sum().backward()
    torch.testing.assert_close(out.detach().cpu(), ref.detach(), rtol=1e-5, atol=1e-5, msg=lambda s: f"{msg} out: {s}")
    torch.testing.assert_close(xd.grad.cpu(), xr.grad, rtol=1e-5, atol=1e-5, msg=lambda s: f"{msg} dx: {s}")
    named = torch.arange(table.size(0)) if sign else ids
    check_table_grad(td.grad.cpu(), tr.grad, named, msg + " dnoise")


def ids_for(n_rows, n_nodes, dup, seed):
    g = torch.Generator().manual_seed(seed)
    if dup:
        ids = torch.randint(0, max(2, n_rows // 3), (n_rows,), generator=g)
        if n_rows >= 5:
            ids[0] = ids[1] = ZERO_ROW
            ids[2] = ids[4] = TINY_ROW
        else:
            ids[0] = TINY_ROW
    else:
        ids = torch.randperm(n_nodes, generator=g)[:n_rows]
        ids = ids[(ids != ZERO_ROW) & (ids != TINY_ROW)]
        ids = torch.cat([torch.tensor([ZERO_ROW, TINY_ROW]), ids])[:n_rows]
    return ids


@pytest.mark.parametrize("F", [1, 3, 100, 128, 130, 767])
@pytest.mark.parametrize("n_rows", [1, 5, 67])
def test_forward_backward_grid(n_rows, F):
    table = make_table(200, F, seed=F)
    x = torch.randn(n_rows, F, generator=torch.Generator().manual_seed(n_rows))
    # unique ids; ids with duplicates (dnoise accumulates); both hold the clamped rows
    run_case(x, table, ids_for(n_rows, 200, False, 1), False, "unique")
    run_case(x, table, ids_for(n_rows, 200, True, 2), False, "duplicates")
    # x as a stride(0) > F view: addressed through ldx, no copy
    wide = torch.randn(n_rows, F + 4, generator=torch.Generator().manual_seed(9)).to(DEV)
    view = wide[:, :F]
    assert n_rows == 1 or view.stride(0) > F
    run_case(view.cpu().contiguous(), table, ids_for(n_rows, 200, False, 3), False, "strided x", x_dev=view)
    # the n_id=None branch: sign(x), sign(0) = 0, the table's rows in order
    xs = x.clone()
    xs[:, ::2] = 0.0
    if F > 1:
        xs[0, 1] = -0.0
    run_case(xs, make_table(n_rows, F, seed=F + 1), None, True, "sign")


def test_single_large_row_loop():
    F, n_rows = 8710, 5
    table = make_table(16, F, seed=11)
    x = torch.randn(n_rows, F, generator=torch.Generator().manual_seed(12))
    run_case(x, table, torch.tensor([ZERO_ROW, 9, TINY_ROW, 9, 0]), False, "F=8710")
    xs = x.clone()
    xs[:, ::5] = 0.0
    run_case(torch.cat([xs, xs, xs, xs[:1]]), table, None, True, "F=8710 sign")


def test_deterministic_mode_is_bitwise_reproducible():
    F, n_rows = 100, 67
    table = make_table(200, F, seed=21)
    ids = ids_for(n_rows, 200, True, 4)
    x = torch.randn(n_rows, F, generator=torch.Generator().manual_seed(22))
    G = torch.randn(n_rows, F, generator=torch.Generator().manual_seed(23))
    tr = table.clone().requires_grad_(True)
    (noisy_input(x, tr, RATE, ids) * G).sum().backward()
    grads = []
    was = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True)
    try:
        for _ in range(2):
            td = table.to(DEV).requires_grad_(True)
            (add_node_noise(x.to(DEV), td, ids.to(DEV), rate=RATE) * G.to(DEV)).sum().backward()
            grads.append(td.grad.clone())
    finally:
        torch.use_deterministic_algorithms(was)
    assert torch.equal(grads[0], grads[1])
    check_table_grad(grads[0].cpu(), tr.grad, ids, "deterministic dnoise")


def test_bounds_guard():
    """Ids outside the table: 200 (one past) and -1.  The table is rows
    8..207 of a 264-row buffer, so even an unguarded access would stay inside
    the allocation; the rows around the table hold a sentinel."""
    F, n_rows, SENT = 128, 9, 12345.0
    buf = torch.full((264, F), SENT)
    buf[8:208] = make_table(200, F, seed=31)
    buf_d = buf.to(DEV)
    table = buf_d[8:208]
    ids = torch.tensor([5, 200, 17, -1, 17, 0, 199, ZERO_ROW, 42])
    bad = (ids < 0) | (ids >= 200)
    x = torch.randn(n_rows, F, generator=torch.Generator().manual_seed(32))
    G = torch.randn(n_rows, F, generator=torch.Generator().manual_seed(33))
    xd, idd, Gd = x.to(DEV), ids.to(DEV), G.to(DEV)
    node_noise_bad_ids(DEV, reset=True)
    out = add_node_noise(xd, table, idd, rate=RATE)
    assert node_noise_bad_ids(DEV) == 2
    assert torch.equal(out[bad.to(DEV)], xd[bad.to(DEV)])
    good = ~bad
    ref = noisy_input(x[good], buf[8:208], RATE, ids[good])
    torch.testing.assert_close(out.cpu()[good], ref, rtol=1e-5, atol=1e-5)
    # backward into a caller-owned gradient buffer with sentinel rows around it
    dbuf = torch.full((264, F), SENT, device=DEV)
    dbuf[8:208] = 0.0
    dn = dbuf[8:208]
    cnt = torch.zeros(1, dtype=torch.int32, device=DEV)
    _lib.check(_lib.load().ngnn_node_noise_bwd(
        Gd.data_ptr(), F, None, F, table.data_ptr(), F, 200, idd.data_ptr(), 1, n_rows, F, RATE, 0,
        dn.data_ptr(), F, cnt.data_ptr(), _lib.stream_handle(DEV)))
    torch.cuda.synchronize()
    assert int(cnt.item()) == 2
    assert (dbuf[:8] == SENT).all() and (dbuf[208:] == SENT).all()
    assert torch.equal(buf_d.cpu(), buf)  # the table and its surroundings untouched
    tr = buf[8:208].clone().requires_grad_(True)
    (noisy_input(x[good], tr, RATE, ids[good]) * G[good]).sum().backward()
    check_table_grad(dn.cpu(), tr.grad, ids[good], "guarded scatter")
    # scatter = 0: the out-of-range rows store zeros
    rows = torch.full((n_rows, F), SENT, device=DEV)
    _lib.check(_lib.load().ngnn_node_noise_bwd(
        Gd.data_ptr(), F, None, F, table.data_ptr(), F, 200, idd.data_ptr(), 0, n_rows, F, RATE, 0,
        rows.data_ptr(), F, None, _lib.stream_handle(DEV)))
    assert (rows[bad.to(DEV)] == 0).all() and (rows[good.to(DEV)] != SENT).all()
    # and through autograd: nothing from those rows, in either mode
    for det in (False, True):
        was = torch.are_deterministic_algorithms_enabled()
        torch.use_deterministic_algorithms(det)
        try:
            td = table.detach().clone().requires_grad_(True)
            (add_node_noise(xd, td, idd, rate=RATE) * Gd).sum().backward()
        finally:
            torch.use_deterministic_algorithms(was)
        check_table_grad(td.grad.cpu(), tr.grad, ids[good], f"autograd det={det}")


def test_forward_under_stream_capture():
    F, n_rows = 100, 67
    table = make_table(200, F, seed=41).to(DEV)
    x = torch.randn(n_rows, F, generator=torch.Generator().manual_seed(42)).to(DEV)
    ids = ids_for(n_rows, 200, False, 5).to(DEV)
    with torch.no_grad():
        add_node_noise(x, table, ids, rate=RATE)  # warm-up (allocates the bad-id counter)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = add_node_noise(x, table, ids, rate=RATE)
        x.copy_(torch.randn(n_rows, F, generator=torch.Generator().manual_seed(43)))
        ids.copy_(ids_for(n_rows, 200, True, 6))
        graph.replay()
        torch.cuda.synchronize()
        eager = add_node_noise(x, table, ids, rate=RATE)
    assert torch.equal(out, eager)


def test_validation_raises():
    x = torch.randn(4, 8, device=DEV)
    t = torch.randn(10, 8, device=DEV)
    ids = torch.arange(4, device=DEV)
    bad_calls = [
        lambda: add_node_noise(x.cpu(), t, ids),
        lambda: add_node_noise(x, t.cpu(), ids),
        lambda: add_node_noise(x.bfloat16(), t, ids),
        lambda: add_node_noise(x, t.bfloat16(), ids),
        lambda: add_node_noise(x, t[:, :7], ids),
        lambda: add_node_noise(x[0], t, ids),
        lambda: add_node_noise(x, t, ids.int()),
        lambda: add_node_noise(x, t, ids[:3]),
        lambda: add_node_noise(x, t, ids.cpu()),
        lambda: add_node_noise(x, t, None),  # 4 rows against a 10-row table
    ]
    for i, call in enumerate(bad_calls):
        with pytest.raises((ValueError, ngnn._lib.NGNNError)):
            call()
            pytest.fail(f"call {i} did not raise")
