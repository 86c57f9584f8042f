"""The per-layer backward kernels at the C ABI against float64
(tests/layer_bwd_ref.py): ngnn_sage_wgrad, ngnn_sage_dgrad_fused,
ngnn_sage_dgrad_gather / _scatter, ngnn_row_extent, ngnn_block_prefix_stats,
called through ngnn._lib with raw pointers, explicit leading dimensions and
the bounds as a device int32 pair -- one case per host dispatch leaf
(DESIGN.md section 5c lists leaf, condition and case).

Bars, all the project's own: weight gradients and input gradients within
gradbar.assert_wgrad (1e-5 of the tensor's max), input gradients also within
GRAD (rtol 1e-4, atol 1e-5, as test_dgrad_lowdim_abi), bitwise where the
summation order is fixed.  tests/test_layer_bwd_cpu.py shows the inputs
themselves cost a plain fp32 evaluation less than a tenth of the bar.

Poison: NaN wherever the contract says nothing is read (rows >= R of dy, y,
plain h, agg, dagg, droot; rows >= R' of the max input; the saved aggregate of
edgeless rows; padding columns; the whole workspace before a call); outputs
are prefilled with 7.0.  Every poisoned place lies inside its allocation and
every index passed is in range.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

if __name__ == "__main__":  # the child of test_wgrad_exact_kernel_on_x3_shapes
    _root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for _p in (os.path.join(_root, "noise-gnn_amd"), _root):
        if _p not in sys.path:
            sys.path.insert(0, _p)

import layer_bwd_ref as lr
from gradbar import _log_fields, assert_wgrad
from ngnn import _lib
from ngnn.block import Block

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GRAD = dict(rtol=1e-4, atol=1e-5)
NAN = float("nan")
SENT = 7.0

N = lr.N_NODES
EI = lr.make_block()
E = EI.size(1)
ROWPTR = lr.rowptr_of(EI, N)
EDGELESS = (ROWPTR[1:] == ROWPTR[:-1]).nonzero().flatten()
TABLE = N + 100  # rows of the feature table under h_idx

_state = {}


def lib():
    return _lib.load()


def block():
    if "blk" not in _state:
        _state["blk"] = Block(EI.to(DEV), N)
    return _state["blk"]


def place(t, ld=None, off=0, fill=NAN):
    """(buffer, address): the rows of t at stride ld, starting off elements
    into a device buffer; padding (and the lead-in) hold `fill`."""
    n, c = t.shape
    ld = c if ld is None else ld
    buf = torch.full((n * ld + off,), fill, dtype=t.dtype)
    buf[off:].view(n, ld)[:, :c] = t
    d = buf.to(DEV)
    return d, d.data_ptr() + off * t.element_size()


def unplace(buf, n, c, ld=None, off=0):
    """(rows, padding) of an output buffer made by place()."""
    ld = c if ld is None else ld
    v = buf.cpu()[off:].view(n, ld)
    return v[:, :c].clone(), v[:, c:].clone()


def device_bounds(R, r_next0=0):
    """The device int32 pair [R', R] as the backward holds it, R' written by
    ngnn_block_prefix_stats itself (and checked against its restatement)."""
    blk = block()
    bnd = torch.tensor([r_next0, R], dtype=torch.int32, device=DEV)
    rc = lib().ngnn_block_prefix_stats(_lib.ptr(blk.rowptr), _lib.ptr(blk.col), bnd.data_ptr() + 4,
                                       None, bnd.data_ptr(), E, _lib.stream_handle(DEV))
    _lib.check(rc, "ngnn_block_prefix_stats")
    torch.cuda.synchronize()
    Rn = int(bnd[0])
    assert Rn == max(r_next0, lr.rnext_of(EI, R)) and int(bnd[1]) == R
    return bnd, Rn


# =========================================================== ngnn_sage_wgrad
def wgrad_ws(Fo, K):
    if _state.get("ws_shape") != (Fo, K):  # (one workspace alive at a time)
        nbytes = lib().ngnn_sage_wgrad_workspace_bytes(Fo, K)
        _state["ws"] = None
        _state["ws"] = torch.empty(nbytes // 4, dtype=torch.float32, device=DEV)
        _state["ws_shape"] = (Fo, K)
    return _state["ws"]


def wgrad_setup(Fo, K, R, mask, hform="f32", layout="plain"):
    """Device operands of one call (poisoned) and the float64 reference."""
    indexed = layout in ("h_idx", "h_idx_dev")
    d = lr.wgrad_inputs(Fo, K, EI, N, table_rows=TABLE if indexed else 0)
    yscale = 2.0 if mask != "none" else 1.0
    dy = lr.poison_rows(d["dy"], R)
    y = None if mask == "none" else lr.poison_rows(d["y"], R)
    if mask == "bf16":
        y = y.bfloat16()
    h, h_idx = d["h"], d["h_idx"]
    if indexed:  # table rows the layer input does not name are never read
        unread = torch.ones(TABLE, dtype=torch.bool)
        unread[h_idx[:R]] = False
        h = lr.poison_rows(h, TABLE, unread.nonzero().flatten())
    else:
        h = lr.poison_rows(h, R)
    if hform == "bf16":
        h = h.bfloat16()
    agg = lr.poison_rows(d["agg"], R, EDGELESS)
    want = lr.wgrad_ref(dy, y, yscale, h, agg, ROWPTR, R, h_idx)
    pad = dict(dy=0, y=0, h=0, agg=0)
    off = dict(dy=0, y=0, h=0, agg=0)
    if layout == "padded":       # rows stay 16-B aligned
        pad = dict(dy=8, y=12, h=4, agg=8)
    elif layout == "padded_odd":  # rows at 4-B alignment only
        pad = dict(dy=1, y=3, h=1, agg=3)
    elif layout == "off_dz":
        off.update(dy=1, y=1)
    elif layout == "off_h":
        off.update(h=1, agg=1)
    ops = dict(Fo=Fo, K=K, yscale=yscale, keep=[], want=want,
               flags=(_lib_flag("h") if hform == "bf16" else 0) | (_lib_flag("y") if mask == "bf16" else 0))
    for name, t, width in (("dy", dy, Fo), ("y", y, Fo), ("h", h, K), ("agg", agg, K)):
        if t is None:
            ops[name], ops["ld_" + name] = None, width
            continue
        buf, addr = place(t, width + pad[name], off[name])
        ops["keep"].append(buf)
        ops[name], ops["ld_" + name] = addr, width + pad[name]
    ops.update(h_dev=None, h_idx=None, h_idx_dev=None, h_rows=0)
    if indexed:
        idx = h_idx.to(DEV)
        ops["keep"].append(idx)
        ops["h_rows"] = TABLE
        if layout == "h_idx":
            ops["h_idx"] = idx.data_ptr()
        else:
            word = torch.tensor([idx.data_ptr()], dtype=torch.int64, device=DEV)
            ops["keep"].append(word)
            ops["h_idx_dev"] = word.data_ptr()
    if layout == "h_dev":  # the address is read from a device word; the argument is null
        word = torch.tensor([ops["h"]], dtype=torch.int64, device=DEV)
        ops["keep"].append(word)
        ops["h_dev"], ops["h"] = word.data_ptr(), None
    return ops


def _lib_flag(which):
    return {"h": 1, "y": 2}[which]  # include/ngnn.h NGNN_WG_H_BF16, NGNN_WG_Y_BF16


def wgrad_call(ops, R, ws=None, poison_ws=True, ws_bytes=None, **override):
    """One ngnn_sage_wgrad call; returns (rc, dwl, dwr, dbl) on the host."""
    Fo, K = ops["Fo"], ops["K"]
    ws = wgrad_ws(Fo, K) if ws is None else ws
    if poison_ws:
        ws.fill_(NAN)  # the header asks for no zero-fill
    a = dict(ops)
    a.update(override)
    r = torch.tensor([R], dtype=torch.int32, device=DEV)
    dwl = torch.full((Fo, K), SENT, device=DEV)
    dwr = torch.full((Fo, K), SENT, device=DEV)
    dbl = torch.full((Fo,), SENT, device=DEV)
    rc = lib().ngnn_sage_wgrad(
        a["dy"], a["ld_dy"], a["y"], a["ld_y"], a["yscale"], a["h"], a["h_dev"], a["h_idx"],
        a["h_idx_dev"], a["h_rows"], a["flags"], a["ld_h"], a["agg"], a["ld_agg"],
        _lib.ptr(block().rowptr), N, a.get("r_ptr", r.data_ptr()), Fo, K, _lib.ptr(dwl),
        _lib.ptr(dbl), _lib.ptr(dwr), ws.data_ptr(), ws.numel() * 4 if ws_bytes is None else ws_bytes,
        _lib.stream_handle(DEV))
    torch.cuda.synchronize()
    return rc, dwl.cpu(), dwr.cpu(), dbl.cpu()


def wgrad_check(got, want, R, tag):
    rc, dwl, dwr, dbl = got
    assert rc == _lib.OK, (tag, rc)
    for name, g, w in (("dwl", dwl, want[0]), ("dwr", dwr, want[1]), ("dbl", dbl, want[2])):
        assert torch.isfinite(g).all(), f"{tag} {name}: poison reached the output"
        assert not (g == SENT).any(), f"{tag} {name}: element not overwritten"
        if R == 0:
            assert not g.any(), f"{tag} {name}: R = 0 must give exact zeros"
        assert_wgrad(g, w, f"wgrad {tag} R={R} {name}")


def wgrad_run(Fo, K, Rs, mask, hform="f32", layout="plain"):
    for R in Rs:
        tag = f"Fo={Fo} K={K} mask={mask} h={hform} {layout}"
        ops = wgrad_setup(Fo, K, R, mask, hform, layout)
        a = wgrad_call(ops, R)
        wgrad_check(a, ops["want"], R, tag)
        b = wgrad_call(ops, R)  # fixed-order reduction: bitwise reproducible
        for x, z in zip(a[1:], b[1:]):
            assert torch.equal(x, z), f"{tag} R={R}: two calls differ"


WGRAD_FULL_R = {(47, 64), (64, 64), (68, 132)}


@pytest.mark.parametrize("mask", ["none", "f32", "bf16"])
@pytest.mark.parametrize("Fo,K", lr.WGRAD_CASES)
def test_wgrad_dispatch_leaves(Fo, K, mask):
    """Every (NT, vz, vh) leaf of the exact kernel and the X3 kernel's
    partial-tile forms, under every mask form."""
    wgrad_run(Fo, K, lr.R_ALL if (Fo, K) in WGRAD_FULL_R else lr.R_FEW, mask)


@pytest.mark.parametrize("mask", ["none", "f32", "bf16"])
@pytest.mark.parametrize("Fo,K", lr.WGRAD_BF16H_CASES)
def test_wgrad_bf16_h(Fo, K, mask):
    """bf16 layer input (NGNN_WG_H_BF16): X3 with one-part h ((64, 128),
    (128, 64)) and the exact kernel's 8-B staging ((48, 64), (16, 64))."""
    wgrad_run(Fo, K, lr.R_FEW, mask, hform="bf16")


@pytest.mark.parametrize("layout", ["padded", "padded_odd", "off_dz", "off_h", "h_idx", "h_idx_dev",
                                    "h_dev"])
@pytest.mark.parametrize("Fo,K", [(7, 24), (48, 256), (20, 33), (68, 132), (64, 131)])
def test_wgrad_layouts(Fo, K, layout):
    """Padded leading dimensions, operands one element into their buffers
    (scalar staging; for X3 shapes: off_dz falls to the exact kernel, off_h
    stays on X3 with 4-B aligned 16-B loads), h through h_idx / h_idx_dev /
    h_dev -- on exact ((7, 24), (48, 256), (20, 33)) and X3 ((68, 132),
    (64, 131)) shapes, with the fp32 mask."""
    wgrad_run(Fo, K, lr.R_FEW, "f32", layout=layout)


@pytest.mark.parametrize("layout", ["padded", "h_idx_dev"])
@pytest.mark.parametrize("Fo,K", [(128, 64), (48, 64)])
def test_wgrad_bf16_h_layouts(Fo, K, layout):
    wgrad_run(Fo, K, lr.R_FEW, "bf16", hform="bf16", layout=layout)


@pytest.mark.parametrize("Fo,K", [(48, 256), (129, 52), (68, 132), (256, 100)])
def test_wgrad_stale_slabs_are_not_reduced(Fo, K):
    """R = 65 straight after R = N on the same workspace: the slabs of the
    larger call's extra slices are still there and must not be summed."""
    big = wgrad_setup(Fo, K, N, "f32")
    wgrad_check(wgrad_call(big, N), big["want"], N, f"Fo={Fo} K={K} before")
    small = wgrad_setup(Fo, K, 65, "f32")
    got = wgrad_call(small, 65, poison_ws=False)
    wgrad_check(got, small["want"], 65, f"Fo={Fo} K={K} stale-slabs")


def test_wgrad_argument_checks():
    Fo, K = 64, 64
    ops = wgrad_setup(Fo, K, N, "f32")
    need = lib().ngnn_sage_wgrad_workspace_bytes(Fo, K)
    assert need == 4 * 256 * (2 * Fo * K + Fo)
    assert wgrad_call(ops, N, ws_bytes=need - 1)[0] == _lib.E_WORKSPACE
    assert wgrad_call(ops, N, ld_dy=Fo - 1)[0] == _lib.E_SHAPE
    assert wgrad_call(ops, N, r_ptr=None)[0] == _lib.E_ARG
    odd = wgrad_setup(48, 66, N, "none")  # K % 4 != 0 with the bf16-h flag: refused, nothing launched
    assert wgrad_call(odd, N, flags=_lib_flag("h"))[0] == _lib.E_SHAPE
    wgrad_check(wgrad_call(ops, N), ops["want"], N, "after refused calls")


X3_OFF_CASES = [(64, 64), (68, 132), (256, 100), (64, 131)]


def _child_main():
    for Fo, K in X3_OFF_CASES:
        for mask in ("none", "f32", "bf16"):
            wgrad_run(Fo, K, lr.R_FEW, mask)
    wgrad_run(128, 64, lr.R_FEW, "f32", hform="bf16")
    print("exact-kernel child ok")


def test_wgrad_exact_kernel_on_x3_shapes():
    """NGNN_WGRAD_X3=0 (read once per process) sends X3-eligible shapes to the
    exact fp32 kernel's 16-B staged NT 4 leaf, reachable in no other way: one
    fresh child process runs the same assertions on three of them (and on
    (64, 131): scalar h under 16-B dz; (128, 64) with bf16 h: 8-B h)."""
    env = dict(os.environ, NGNN_WGRAD_X3="0")
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, timeout=240,
                       capture_output=True, text=True)
    assert r.returncode == 0 and "exact-kernel child ok" in r.stdout, (
        f"child exit {r.returncode}\n" + r.stdout[-2000:] + r.stderr[-4000:])


# ===================================================== ngnn_sage_dgrad_fused
def grad_close(got, want, tag):
    """GRAD elementwise; the worst |err| / (atol + rtol |want|) is logged
    (NGNN_GRAD_LOG) and printed before it is asserted."""
    if want.numel():
        err = (got.double() - want).abs()
        worst = float((err / (GRAD["atol"] + GRAD["rtol"] * want.abs())).max())
        _log_fields(tensor=tag, grad_bar_ratio=worst, max_err=float(err.max()))
        print(f"{tag}: worst |err| / (atol + rtol |ref|) = {worst:.3f}")
    torch.testing.assert_close(got.double(), want, **GRAD)


def dgrad_tail_check(dh, pad, Rn, zero_tail, tag):
    assert torch.isfinite(dh).all(), f"{tag}: poison reached the output"
    tail = dh[Rn:]
    assert torch.all(tail == (0.0 if zero_tail else SENT)), f"{tag}: rows >= R' touched wrongly"
    assert torch.all(pad == SENT), f"{tag}: padding columns written"


def fused_run(Fo, K, reduce, R, masked, zero_tail, w_off=0, r_next0=0):
    d = lr.dgrad_inputs(Fo, K, EI, N, reduce)
    bnd, Rn = device_bounds(R, r_next0)
    yscale = 2.0 if masked else 1.0
    dy = lr.poison_rows(d["dy"], R)
    y = lr.poison_rows(d["y"], R) if masked else None
    h = agg = None
    if reduce == "max":
        h, agg = lr.poison_rows(d["h"], Rn), lr.poison_rows(d["agg"], R, EDGELESS)
    want = lr.dgrad_fused_ref(dy, y, yscale, d["wl"], d["wr"], EI, N, R, reduce, h, agg)
    keep = [place(dy), place(y) if masked else (None, None), place(d["wl"], off=w_off),
            place(d["wr"], off=w_off), place(h) if h is not None else (None, None),
            place(agg) if agg is not None else (None, None)]
    ldd = K + 4
    dh, p_dh = place(torch.full((N, K), SENT), ldd, fill=SENT)
    blk = block()
    rc = lib().ngnn_sage_dgrad_fused(
        keep[0][1], Fo, keep[1][1], Fo, yscale, keep[2][1], keep[3][1], Fo, K, _lib.ptr(blk.rowptr),
        _lib.ptr(blk.col), N, bnd.data_ptr() + 4, bnd.data_ptr(), _lib.REDUCE[reduce], keep[4][1], K,
        keep[5][1], K, p_dh, ldd, zero_tail, _lib.stream_handle(DEV))
    _lib.check(rc, "ngnn_sage_dgrad_fused")
    torch.cuda.synchronize()
    got, pad = unplace(dh, N, K, ldd)
    tag = f"dgrad_fused Fo={Fo} K={K} {reduce} R={R} masked={masked} zt={zero_tail} w_off={w_off}"
    dgrad_tail_check(got, pad, Rn, zero_tail, tag)
    assert_wgrad(got[:Rn], want[:Rn], tag)
    if R == 0:
        assert not got[:Rn].any(), f"{tag}: R = 0 must leave rows < R' zero"
    grad_close(got[:Rn], want[:Rn], tag)


FUSED_FULL_R = {(64, 64), (10, 48)}


@pytest.mark.parametrize("reduce", ["mean", "sum", "max"])
@pytest.mark.parametrize("Fo,K,w_off", [(Fo, K, 0) for Fo, K in lr.DGRAD_FUSED_CASES] + [(64, 64, 1)])
def test_dgrad_fused(Fo, K, w_off, reduce):
    """LDS-resident and L2-streaming variants (by Fo >= 32, (Fo K) % 4, the
    150 KiB budget, the alignment of wl / wr), with and without the mask,
    zero_tail 0 and 1; R = 0 runs with R' preset to 100.

    Measured on the MI355X (profiles/layer_bwd_grad_errors.jsonl): every
    case within 6e-7 of the tensor's max (bar 1e-5).  The elementwise GRAD
    tolerance is closest at (512, 40), sum, R = N: worst |err| / (atol + rtol
    |ref|) 0.53 .. 0.64 from run to run (the atomics' order), on an element
    of 0.04 in a tensor whose max is about 160.  With one chain of 512 dependent
    adds per output the kernel stood at 1.25 there and failed this test (a
    plain fp32 torch evaluation: 1.0); it keeps four partial sums now."""
    Rs = lr.R_ALL if (Fo, K) in FUSED_FULL_R and not w_off else lr.R_FEW
    for R in Rs:
        for masked in (False, True):
            for zt in (0, 1):
                fused_run(Fo, K, reduce, R, masked, zt, w_off, r_next0=100 if R == 0 else 0)


def test_dgrad_fused_shape_envelope():
    Fo, K = 513, 8
    bnd, _ = device_bounds(65)
    dy, w = torch.zeros(N, Fo, device=DEV), torch.zeros(Fo, K, device=DEV)
    dh = torch.full((N, K), SENT, device=DEV)
    blk = block()
    rc = lib().ngnn_sage_dgrad_fused(
        _lib.ptr(dy), Fo, None, Fo, 1.0, _lib.ptr(w), _lib.ptr(w), Fo, K, _lib.ptr(blk.rowptr),
        _lib.ptr(blk.col), N, bnd.data_ptr() + 4, bnd.data_ptr(), _lib.REDUCE["mean"], None, K, None,
        K, _lib.ptr(dh), K, 0, _lib.stream_handle(DEV))
    torch.cuda.synchronize()
    assert rc == _lib.E_SHAPE and torch.all(dh == SENT)


# ==================================== ngnn_sage_dgrad_gather / _dgrad_scatter
def gather_scatter_run(K, reduce, R, layout, zero_tail, cache):
    """One gather call (twice: bitwise equal) and one scatter call on the same
    operands.  layout: 'halves' -- dagg | droot as the column halves of one
    [N, 2K] buffer (the dgrad GEMM's output); 'separate'; 'offset' -- every
    float operand one element into its buffer (scalar forms)."""
    d = lr.gather_inputs(K, EI, N, reduce)
    bnd, Rn = device_bounds(R)
    dagg, droot = lr.poison_rows(d["dagg"], R), lr.poison_rows(d["droot"], R)
    h = agg = None
    if reduce == "max":
        h, agg = lr.poison_rows(d["h"], Rn), lr.poison_rows(d["agg"], R, EDGELESS)
    if ("ref", R) not in cache:
        cache["ref", R] = (lr.dgrad_ref(dagg, droot, EI, N, R, reduce, h, agg),
                           torch.from_numpy(lr.dgrad_gather_f32(dagg, droot, EI, N, R, reduce, h, agg)))
    want, want32 = cache["ref", R]
    off = 1 if layout == "offset" else 0
    if layout == "halves":
        both, p = place(torch.cat([dagg, droot], dim=1))
        p_dagg, p_droot, ld_g, keep = p, p + 4 * K, 2 * K, [both]
    else:
        b0, p_dagg = place(dagg, K + off, off)
        b1, p_droot = place(droot, K + off, off)
        ld_g, keep = K + off, [b0, b1]
    bh, p_h = place(h, K + off, off) if h is not None else (None, None)
    ba, p_agg = place(agg, K + off, off) if agg is not None else (None, None)
    ldd = K + (1 if off else 4)
    blk = block()
    t = blk.transposed()
    red = _lib.REDUCE[reduce]
    ws_bytes = lib().ngnn_sage_dgrad_workspace_bytes(N, K, red)
    assert ws_bytes == (4 * N * K if reduce == "max" else 0)
    ws = torch.full((ws_bytes // 4 + 1,), NAN, device=DEV)
    tag = f"K={K} {reduce} R={R} {layout} zt={zero_tail}"
    outs = []
    for _ in range(2):
        dh, p_dh = place(torch.full((N, K), SENT), ldd, off, fill=SENT)
        ws.fill_(NAN)
        rc = lib().ngnn_sage_dgrad_gather(
            p_dagg, ld_g, p_droot, ld_g, _lib.ptr(blk.rowptr), _lib.ptr(blk.col), _lib.ptr(t.rowptr),
            _lib.ptr(t.col), N, bnd.data_ptr() + 4, bnd.data_ptr(), K, red, p_h, K + off, p_agg,
            K + off, p_dh, ldd, zero_tail, ws.data_ptr(), ws_bytes, _lib.stream_handle(DEV))
        _lib.check(rc, "ngnn_sage_dgrad_gather")
        torch.cuda.synchronize()
        outs.append(unplace(dh, N, K, ldd, off))
    got, pad = outs[0]
    dgrad_tail_check(got, pad, Rn, zero_tail, "gather " + tag)
    assert torch.equal(got, outs[1][0]), f"gather {tag}: two calls differ"
    assert torch.equal(got[:Rn], want32[:Rn]), (
        f"gather {tag}: not the edge-order fp32 sum (max |diff| "
        f"{float((got[:Rn] - want32[:Rn]).abs().max()):.3e})")
    assert_wgrad(got[:Rn], want[:Rn], "dgrad_gather " + tag)

    dh, p_dh = place(torch.full((N, K), SENT), ldd, off, fill=SENT)
    rc = lib().ngnn_sage_dgrad_scatter(
        p_dagg, ld_g, p_droot, ld_g, _lib.ptr(blk.rowptr), _lib.ptr(blk.col), N, bnd.data_ptr() + 4,
        bnd.data_ptr(), K, red, p_h, K + off, p_agg, K + off, p_dh, ldd, zero_tail,
        _lib.stream_handle(DEV))
    _lib.check(rc, "ngnn_sage_dgrad_scatter")
    torch.cuda.synchronize()
    sc, pad = unplace(dh, N, K, ldd, off)
    dgrad_tail_check(sc, pad, Rn, zero_tail, "scatter " + tag)
    assert_wgrad(sc[:Rn], want[:Rn], "dgrad_scatter " + tag)
    grad_close(sc[:Rn], want[:Rn], "dgrad_scatter " + tag)
    torch.testing.assert_close(sc[:Rn], got[:Rn], **GRAD)


@pytest.mark.parametrize("reduce", ["mean", "sum", "max"])
@pytest.mark.parametrize("K", lr.GATHER_K)
def test_dgrad_gather_and_scatter(K, reduce):
    """The deterministic gather is the fp32 edge-order sum bit for bit (the
    kernel divides and adds in the oracle's order; contraction is off), for
    all three reductions; the atomic scatter is within GRAD of float64 and of
    the gather (measured: at most 0.33 .. 0.52 of that tolerance from run to
    run, K = 13, sum, R = N; both within 7e-7 of the tensor's max).  K walks the lanes-per-row widths 4..64, a second column
    chunk (260; scalar form: 100, 132, 260; K = 20, 7 and 13 are there for
    the 8-wide vector form and the 8- and 16-wide scalar forms, which the
    other sizes skip) and k_dh_init's three loops
    (64: K/4 divides 256; 132: it does not; 3: scalar)."""
    cache = {}
    for layout in ("halves", "separate", "offset"):
        for R in (lr.R_ALL if (K == 64 and layout == "halves") else lr.R_FEW):
            for zt in (0, 1):
                gather_scatter_run(K, reduce, R, layout, zt, cache)


def test_dgrad_gather_max_workspace_check():
    K = 8
    bnd, _ = device_bounds(65)
    z = torch.zeros(N, K, device=DEV)
    dh = torch.full((N, K), SENT, device=DEV)
    blk = block()
    t = blk.transposed()
    need = lib().ngnn_sage_dgrad_workspace_bytes(N, K, _lib.REDUCE["max"])
    ws = torch.zeros(need, dtype=torch.uint8, device=DEV)
    rc = lib().ngnn_sage_dgrad_gather(
        _lib.ptr(z), K, _lib.ptr(z), K, _lib.ptr(blk.rowptr), _lib.ptr(blk.col), _lib.ptr(t.rowptr),
        _lib.ptr(t.col), N, bnd.data_ptr() + 4, bnd.data_ptr(), K, _lib.REDUCE["max"], _lib.ptr(z), K,
        _lib.ptr(z), K, _lib.ptr(dh), K, 0, _lib.ptr(ws), need - 1, _lib.stream_handle(DEV))
    torch.cuda.synchronize()
    assert rc == _lib.E_WORKSPACE and torch.all(dh == SENT)


# ============================================================ ngnn_row_extent
def row_extent_call(g, ld, off, out0, pad_fill=3.0):
    n, F = g.shape
    buf, p = place(g, ld, off, fill=pad_fill)
    out = torch.tensor([out0], dtype=torch.int32, device=DEV)
    rc = lib().ngnn_row_extent(p, ld, n, F, out.data_ptr(), _lib.stream_handle(DEV))
    _lib.check(rc, "ngnn_row_extent")
    torch.cuda.synchronize()
    return int(out[0])


@pytest.mark.parametrize("layout", ["flat", "strided", "offset"])
@pytest.mark.parametrize("F", [1, 3, 4, 10, 47, 64])
def test_row_extent(F, layout):
    """The flat float4 sweep (ld == F at a 16-B aligned base; F = 3 and 47 put
    a float4 across two rows), the strided sweep (ld > F over nonzero padding)
    and a base one element into its buffer; a NaN counts, -0.0 does not."""
    n = 257
    ld, off = {"flat": (F, 0), "strided": (F + 3, 0), "offset": (F, 1)}[layout]
    total = n * F
    spots = {(0, F - 1), (n - 1, 0), (100, F // 2), (n - 1, F - 1)}
    spots |= {divmod(e, F) for e in range(total - total % 4, total)}  # the flat sweep's tail
    zero = torch.zeros(n, F)
    zero[::2] = -0.0
    for out0 in (0, 5):
        assert row_extent_call(zero, ld, off, out0) == out0  # all zero: out as given
    for r, c in sorted(spots):
        for val in (1.5, NAN, -1e-30):
            g = zero.clone()
            g[r, c] = val
            want = lr.row_extent_ref(g.numpy())
            assert want == r + 1
            assert row_extent_call(g, ld, off, 0) == want, (F, layout, r, c, val)
        assert row_extent_call(g, ld, off, n + 7) == n + 7  # a larger preset stays
        assert row_extent_call(g, ld, off, max(r, 1)) == max(r + 1, 1)
    g = torch.randn(n, F)
    g[200:] = 0
    assert row_extent_call(g, ld, off, 3) == lr.row_extent_ref(g.numpy(), 3) == 200


# ==================================================== ngnn_block_prefix_stats
@pytest.mark.parametrize("R", [0, 1, 65, N])
def test_block_prefix_stats(R):
    """*r_next = max(*r_next, R, 1 + max col[0 .. rowptr[R])), *nnz_out =
    rowptr[R] (nullable): r_next preset to 0, between R and the answer, and
    above it.  The block's CSR is the stable target grouping."""
    blk = block()
    rowptr, col = lr.target_grouped(EI, N)
    assert torch.equal(blk.rowptr.cpu().long(), rowptr) and torch.equal(blk.col.cpu().long(), col)
    ans, nnz = lr.prefix_stats_ref(rowptr.numpy(), col.numpy(), R)
    for preset in (0, (R + ans) // 2, ans + 9):
        for with_nnz in (False, True):
            bnd = torch.tensor([preset, R, -1], dtype=torch.int32, device=DEV)
            rc = lib().ngnn_block_prefix_stats(
                _lib.ptr(blk.rowptr), _lib.ptr(blk.col), bnd.data_ptr() + 4,
                bnd.data_ptr() + 8 if with_nnz else None, bnd.data_ptr(), E, _lib.stream_handle(DEV))
            _lib.check(rc, "ngnn_block_prefix_stats")
            torch.cuda.synchronize()
            want = lr.prefix_stats_ref(rowptr.numpy(), col.numpy(), R, preset)
            assert bnd.tolist() == [want[0], R, want[1] if with_nnz else -1], (R, preset, with_nnz)


@pytest.mark.parametrize("R", [0, 65])
def test_block_prefix_stats_without_edges(R):
    rowptr = torch.zeros(N + 1, dtype=torch.int32, device=DEV)
    for preset in (0, R + 4):
        bnd = torch.tensor([preset, R, -1], dtype=torch.int32, device=DEV)
        rc = lib().ngnn_block_prefix_stats(_lib.ptr(rowptr), None, bnd.data_ptr() + 4,
                                           bnd.data_ptr() + 8, bnd.data_ptr(), 0,
                                           _lib.stream_handle(DEV))
        _lib.check(rc, "ngnn_block_prefix_stats")
        torch.cuda.synchronize()
        assert bnd.tolist() == [max(preset, R), R, 0]


if __name__ == "__main__":
    _child_main()
