"""The argument checks of ngnn_sage2_fwd and ngnn_sage2_bwd at the C ABI (no
GPU: every call here fails a check or returns early, before any launch).

The entries promise a code per fault AND, for a call with several faults,
the code of the first check in their fixed order (csrc/ngnn_fwd2.hip
sage2_fwd_check, csrc/ngnn_bwd2.hip sage2_bwd_check; include/ngnn.h).  Both
rules are restated below in Python, check by check.  From one valid argument
set per entry the test applies every single perturbation the checks name and
every pair of them, and compares the library's answer with the rule's.  A
call the rule lets through would go on to launch and is left out (the valid
set itself, a NULL wr0 alone, a well-formed head alone, ...).
"""
import ctypes
import itertools
import math

from ngnn import _lib

A = 4096            # an aligned placeholder address: nothing is dereferenced on the host
LIM = 0xF0000000 - 4096   # kRangeMax (csrc/ngnn_internal.h): largest whole-buffer range
MEAN, SUM, MAX = _lib.REDUCE["mean"], _lib.REDUCE["sum"], _lib.REDUCE["max"]
BIG_LD = 1 << 24    # 64 rows x 2^24 floats x 4 B = 2^32 > LIM
FWD_ORDER = ["x", "x_dev", "xrow", "xrow_dev", "x_rows", "ldx", "K0", "n_rows", "n_rows_dev", "n_edge_rows",
             "n_edge_rows_dev", "rowptr", "col", "col_x", "reduce", "wl0", "bl0", "wr0", "ldw0", "H", "wl1", "bl1",
             "wr1", "ldw1", "F1", "p_drop", "seed", "seed_dev", "h", "ldh", "h_rows", "h_rows_dev", "agg0", "ld_agg",
             "out", "ldo", "head", "stages", "ws", "ws_bytes", "stream"]
BWD_ORDER = ["dy", "ldy", "F1", "wl1", "wr1", "ldw1", "h", "ldh", "yscale", "x", "x_dev", "xrow", "xrow_dev", "x_rows",
             "ldx", "K0", "agg0", "ld_agg", "rowptr", "col", "n_rows", "r_ptr", "rnext_ptr", "reduce", "dwl1", "dbl1",
             "dwr1", "dwl0", "dbl0", "dwr0", "g_pre", "adam", "ws", "ws_bytes", "stream"]
HEAD_ORDER = ["y", "B", "ignore_index", "loss", "count", "dy", "ldd", "g", "g_rows", "g_rows_dev", "ws", "ws_bytes",
              "src_count"]


def _al(p, a):
    return p is None or p % a == 0


def _a256(n):
    return (n + 255) & ~255


def fwd_ws_need(F1, n_rows):
    rows16 = -(-max(n_rows, 1) // 16) * 16
    return _a256(rows16 * 256 * 4) + _a256(rows16 * -(-F1 // 16) * 16 * 4)


def bwd_ws_need(n_rows, K0, F1):
    return _a256(64 * (512 * K0 + 256 + 512 * F1 + F1) * 4) + max(n_rows, 1) * ((F1 + 3) & ~3) * 4


def fwd_valid():
    return dict(x=A, x_dev=None, xrow=None, xrow_dev=None, x_rows=0, ldx=100, K0=100, n_rows=64, n_rows_dev=None,
                n_edge_rows=64, n_edge_rows_dev=None, rowptr=A, col=A, col_x=None, reduce=MEAN, wl0=A, bl0=A, wr0=A,
                ldw0=100, H=256, wl1=A, bl1=A, wr1=A, ldw1=256, F1=47, p_drop=0.5, seed=7, seed_dev=None, h=A,
                ldh=256, h_rows=64, h_rows_dev=None, agg0=A, ld_agg=100, out=A, ldo=47, head=None,
                stages=_lib.SAGE2_ALL, ws=A, ws_bytes=fwd_ws_need(47, 64), stream=None)


def head_valid():
    return dict(y=A, B=16, ignore_index=-100, loss=A, count=A, dy=A, ldd=47, g=None, g_rows=0, g_rows_dev=None,
                ws=A, ws_bytes=256 + 4 * (32 + 16), src_count=None)


def fwd_rule(a):
    """sage2_fwd_check's answer, or None when the call would go on to launch."""
    K0, H, F1, n = a["K0"], a["H"], a["F1"], a["n_rows"]
    if not (96 < K0 <= 128 and K0 % 4 == 0 and H == 256 and 32 < F1 <= 48 and a["reduce"] in (MEAN, SUM)):
        return _lib.E_SHAPE
    if n < 0 or a["n_edge_rows"] < 0 or a["h_rows"] < 0:
        return _lib.E_ARG
    if a["p_drop"] < 0.0 or not (a["p_drop"] <= 1.0):
        return _lib.E_ARG
    if a["stages"] <= 0 or a["stages"] > _lib.SAGE2_ALL:
        return _lib.E_ARG
    if (a["ldx"] < K0 or a["ldx"] % 4 or a["ldw0"] < K0 or a["ldw0"] % 4 or a["ldw1"] < H or a["ldw1"] % 4
            or a["ldh"] < H or a["ldh"] % 4 or a["ld_agg"] < K0 or a["ld_agg"] % 4 or a["ldo"] != F1):
        return _lib.E_SHAPE
    if n > 2**31 - 1:
        return _lib.E_RANGE
    indexed = bool(a["xrow"] or a["xrow_dev"])
    if indexed and (a["x_rows"] <= 0 or not a["col_x"]):
        return _lib.E_ARG
    if n == 0:
        return _lib.OK
    if not a["wr0"] and indexed:
        return _lib.E_ARG
    if ((not a["x"] and not a["x_dev"]) or not a["rowptr"] or (not a["col"] and a["n_edge_rows"] > 0)
            or not all(a[k] for k in ("wl0", "bl0", "wl1", "bl1", "wr1", "h", "agg0", "out", "ws"))):
        return _lib.E_ARG
    if (not all(_al(a[k], 16) for k in ("x", "h", "out", "agg0", "bl0", "wr0", "wl0", "wr1", "wl1"))
            or not _al(a["ws"], 256)):
        return _lib.E_ALIGN
    if (max(n, a["x_rows"] if indexed else 0) * a["ldx"] * 4 > LIM or n * a["ldh"] * 4 > LIM
            or n * a["ld_agg"] * 4 > LIM or n * a["ldo"] * 4 > LIM or n * 256 * 4 > LIM):
        return _lib.E_RANGE
    if a["ws_bytes"] < fwd_ws_need(F1, n):
        return _lib.E_WORKSPACE
    hd = a["head"]
    if hd is not None:
        if not all(hd[k] for k in ("y", "loss", "count", "dy", "ws")):
            return _lib.E_ARG
        if hd["B"] <= 0 or hd["B"] > n or hd["ldd"] < F1:
            return _lib.E_ARG
        if hd["g"] and (hd["g_rows"] < 0 or hd["g_rows"] > n):
            return _lib.E_ARG
        if hd["ws_bytes"] < 256 + 4 * (32 + hd["B"]):
            return _lib.E_WORKSPACE
        if not _al(hd["ws"], 16) or not _al(hd["g"], 16):
            return _lib.E_ALIGN
        if hd["g"] and hd["g_rows"] * ((F1 + 3) & ~3) * 4 > LIM:
            return _lib.E_RANGE
    return None


def bwd_valid():
    return dict(dy=A, ldy=47, F1=47, wl1=A, wr1=A, ldw1=256, h=A, ldh=256, yscale=2.0, x=A, x_dev=None, xrow=None,
                xrow_dev=None, x_rows=0, ldx=100, K0=100, agg0=A, ld_agg=100, rowptr=A, col=A, n_rows=64, r_ptr=A,
                rnext_ptr=A, reduce=MEAN, dwl1=A, dbl1=A, dwr1=A, dwl0=A, dbl0=A, dwr0=A, g_pre=None, adam=None,
                ws=A, ws_bytes=bwd_ws_need(64, 100, 47), stream=None)


def fold_valid():
    return dict(param=[A] * 6, exp_avg=[A] * 6, exp_avg_sq=[A] * 6, step=A)


def bwd_rule(a):
    """sage2_bwd_check's answer, or None when the call would go on to launch."""
    F1, K0, n = a["F1"], a["K0"], a["n_rows"]
    if a["reduce"] not in (MEAN, SUM):
        return _lib.E_ARG
    if F1 <= 0 or F1 > 48 or K0 <= 0 or K0 > 128 or K0 % 4:
        return _lib.E_SHAPE
    if n < 0 or n > 2**31 - 1:
        return _lib.E_RANGE
    root = bool(a["dwr0"] or a["dwr1"])
    indexed = bool(a["xrow"] or a["xrow_dev"])
    if (not all(a[k] for k in ("dy", "wl1", "wr1", "h", "agg0", "rowptr", "col", "r_ptr", "rnext_ptr", "dwl1", "dbl1",
                               "dwl0", "dbl0", "ws"))
            or (root and not a["x"] and not a["x_dev"]) or (root and (not a["dwr1"] or not a["dwr0"]))):
        return _lib.E_ARG
    if not root and indexed:
        return _lib.E_ARG
    if (a["ldy"] < F1 or a["ldw1"] < 256 or a["ldh"] < 256 or a["ldh"] % 4 or a["ldx"] < K0 or a["ldx"] % 4
            or a["ld_agg"] < K0 or a["ld_agg"] % 4):
        return _lib.E_SHAPE
    if not all(_al(a[k], 16) for k in ("x", "h", "agg0", "g_pre")) or not _al(a["ws"], 256):
        return _lib.E_ALIGN
    if indexed and a["x_rows"] <= 0:
        return _lib.E_ARG
    if (n * a["ldh"] * 4 > LIM or n * a["ld_agg"] * 4 > LIM or n * a["ldy"] * 4 > LIM
            or max(n, a["x_rows"] if indexed else 0) * a["ldx"] * 4 > LIM or n * ((F1 + 3) & ~3) * 4 > LIM):
        return _lib.E_RANGE
    ad = a["adam"]
    if ad is not None:
        if not ad["step"]:
            return _lib.E_ARG
        if not all(ad[f][k] for k in range(6) for f in ("param", "exp_avg", "exp_avg_sq")):
            return _lib.E_ARG
    if a["ws_bytes"] < bwd_ws_need(n, K0, F1):
        return _lib.E_WORKSPACE
    return None


def _set(**kw):
    return lambda a: a.update(kw)


def _head(**kw):
    def f(a):
        a["head"] = dict(a["head"] or head_valid(), **kw)
    return f


def _fold(field=None, k=None):
    def f(a):
        ad = a["adam"] or fold_valid()
        ad = dict(ad, param=list(ad["param"]), exp_avg=list(ad["exp_avg"]), exp_avg_sq=list(ad["exp_avg_sq"]))
        if field == "step":
            ad["step"] = None
        elif field:
            ad[field][k] = None
        a["adam"] = ad
    return f


def _common(ptrs, strides, al16, rows):
    P = {f"{k}=NULL": _set(**{k: None}) for k in ptrs}
    for k, lo in strides.items():
        P[f"{k} short by one"] = _set(**{k: lo - 1})
        P[f"{k} not a multiple of 4"] = _set(**{k: lo + 1})
        P[f"{k} past the range"] = _set(**{k: BIG_LD})
    P.update({f"{k} misaligned": _set(**{k: A + 4}) for k in al16})
    P["ws misaligned"] = _set(ws=A + 16)
    P.update({f"{k} negative": _set(**{k: -1}) for k in rows})
    P["n_rows above int32"] = _set(n_rows=2**31)
    P["n_rows past the range"] = _set(n_rows=30_000_000)
    P["indexed (xrow)"] = _set(xrow=A, x_rows=50, col_x=A)
    P["indexed (xrow_dev)"] = _set(xrow_dev=A, x_rows=50, col_x=A)
    P["indexed, x_rows 0"] = _set(xrow=A, x_rows=0, col_x=A)
    P["indexed, table past the range"] = _set(xrow=A, x_rows=1 << 26, col_x=A)
    return P


def fwd_perturbations():
    P = _common(["x", "rowptr", "col", "wl0", "bl0", "wr0", "wl1", "bl1", "wr1", "h", "agg0", "out", "ws"],
                dict(ldx=100, ldw0=100, ldw1=256, ldh=256, ld_agg=100),
                ["x", "h", "out", "agg0", "bl0", "wr0", "wl0", "wr1", "wl1"], ["n_rows", "n_edge_rows", "h_rows"])
    P.update({"ldo short by one": _set(ldo=46), "ldo padded": _set(ldo=48), "x by x_dev": _set(x=None, x_dev=A),
              "indexed, col_x NULL": _set(xrow=A, x_rows=50, col_x=None),
              "n_rows 0": _set(n_rows=0), "no edge rows": _set(n_edge_rows=0),
              "stages 0": _set(stages=0), "stages above ALL": _set(stages=_lib.SAGE2_ALL + 1),
              "stages MAIN": _set(stages=_lib.SAGE2_MAIN),
              "p_drop < 0": _set(p_drop=-0.1), "p_drop > 1": _set(p_drop=1.5), "p_drop NaN": _set(p_drop=math.nan),
              "ws short by one byte": _set(ws_bytes=fwd_ws_need(47, 64) - 1),
              "K0 96": _set(K0=96), "K0 132": _set(K0=132), "K0 102": _set(K0=102), "H 128": _set(H=128),
              "F1 32": _set(F1=32, ldo=32), "F1 49": _set(F1=49, ldo=49), "reduce max": _set(reduce=MAX),
              "reduce sum": _set(reduce=SUM), "head": _head(), "head g": _head(g=A, g_rows=64),
              "head B 0": _head(B=0), "head B above n_rows": _head(B=65, ws_bytes=1 << 20),
              "head ldd short": _head(ldd=46), "head g_rows negative": _head(g=A, g_rows=-1),
              "head g_rows above n_rows": _head(g=A, g_rows=65), "head g past the range": _head(g=A, g_rows=25_000_000),
              "head ws short by one byte": _head(ws_bytes=256 + 4 * (32 + 16) - 1),
              "head ws misaligned": _head(ws=A + 4), "head g misaligned": _head(g=A + 4, g_rows=64)})
    P.update({f"head {k}=NULL": _head(**{k: None}) for k in ("y", "loss", "count", "dy", "ws")})
    return P


def bwd_perturbations():
    P = _common(["dy", "wl1", "wr1", "h", "x", "agg0", "rowptr", "col", "r_ptr", "rnext_ptr", "dwl1", "dbl1", "dwr1",
                 "dwl0", "dbl0", "dwr0", "ws"],
                dict(ldy=47, ldw1=256, ldh=256, ldx=100, ld_agg=100), ["x", "h", "agg0"], ["n_rows"])
    P.update({"root-free": _set(dwr0=None, dwr1=None), "root-free, x NULL": _set(dwr0=None, dwr1=None, x=None),
              "x by x_dev": _set(x=None, x_dev=A), "g_pre": _set(g_pre=A), "g_pre misaligned": _set(g_pre=A + 4),
              "reduce max": _set(reduce=MAX), "reduce sum": _set(reduce=SUM), "F1 0": _set(F1=0), "F1 49": _set(F1=49),
              "K0 0": _set(K0=0), "K0 132": _set(K0=132), "K0 102": _set(K0=102), "n_rows 0": _set(n_rows=0),
              "ws short by one byte": _set(ws_bytes=bwd_ws_need(64, 100, 47) - 1),
              "fold": _fold(), "fold step=NULL": _fold("step")})
    P.update({f"fold {f}[{k}]=NULL": _fold(f, k) for f in ("param", "exp_avg", "exp_avg_sq") for k in range(6)})
    return P


def _call_fwd(lib, a):
    hd = a["head"]
    keep = _lib.XentHead(*[hd[k] for k in HEAD_ORDER]) if hd is not None else None
    args = [(None if keep is None else ctypes.byref(keep)) if k == "head" else a[k] for k in FWD_ORDER]
    return lib.ngnn_sage2_fwd(*args)


def _call_bwd(lib, a):
    ad, keep = a["adam"], None
    if ad is not None:
        arr = [(ctypes.c_void_p * 6)(*ad[f]) for f in ("param", "exp_avg", "exp_avg_sq")]
        keep = _lib.AdamFold(*arr, ad["step"], 1e-3, 0.9, 0.999, 1e-8, 0.0)
    args = [(None if keep is None else ctypes.byref(keep)) if k == "adam" else a[k] for k in BWD_ORDER]
    return lib.ngnn_sage2_bwd(*args)


def _sweep(valid, perturbations, rule, call):
    assert rule(valid()) is None, "the starting set must pass every check"
    lib = _lib.load()
    names = list(perturbations)
    cases = [(n,) for n in names] + list(itertools.combinations(names, 2))
    ran, wrong = 0, []
    for case in cases:
        a = valid()
        for n in case:
            perturbations[n](a)
        want = rule(a)
        if want is None:
            continue  # (would launch)
        ran += 1
        got = call(lib, a)
        if got != want:
            wrong.append((case, got, want))
    assert not wrong, f"{len(wrong)} of {ran} cases, first: {wrong[:5]}"
    return ran, len(names)


def test_sage2_fwd_argument_checks():
    ran, n = _sweep(fwd_valid, fwd_perturbations(), fwd_rule, _call_fwd)
    print(f"ngnn_sage2_fwd: {ran} failing or early-return cases from {n} perturbations")
    assert n >= 70 and ran >= 2500


def test_sage2_bwd_argument_checks():
    ran, n = _sweep(bwd_valid, bwd_perturbations(), bwd_rule, _call_bwd)
    print(f"ngnn_sage2_bwd: {ran} failing cases from {n} perturbations")
    assert n >= 70 and ran >= 2400


def test_every_code_and_the_early_return_are_reached():
    """The sweep is not vacuous: each code the checks can give is the rule's
    answer for some case, as is the forward's n_rows == 0 early NGNN_OK."""
    def codes(valid, P, rule):
        out = set()
        for case in [(n,) for n in P] + list(itertools.combinations(P, 2)):
            a = valid()
            for n in case:
                P[n](a)
            out.add(rule(a))
        return out
    every = {_lib.E_ARG, _lib.E_SHAPE, _lib.E_ALIGN, _lib.E_RANGE, _lib.E_WORKSPACE, None}
    assert codes(fwd_valid, fwd_perturbations(), fwd_rule) == every | {_lib.OK}
    assert codes(bwd_valid, bwd_perturbations(), bwd_rule) == every
