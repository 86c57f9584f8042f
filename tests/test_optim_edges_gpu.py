"""ngnn_adam_step's edge paths against a float64 restatement (tests/adam_ref.py).

Teacher-forced, one step at a time: the kernel's (p, m, v) are read before a
step, the step runs, and (p', m', v') are compared with adam_ref applied to
that same start state and the known step number t -- errors do not accumulate
and a wrong t still shows.

The bar is measured (gradbar.assert_measured_bar): from the same start state
one step of torch.optim.Adam(capturable=True) on the device gives e_torch =
max|q_torch - q_ref64| per tensor and quantity q in (p, m, v); ours must hold
e_ours <= 4 * max(e_torch, 2^-24 * max|q_ref64|).  (4: another, equally valid
operation order and powf.  A wrong rule -- eps inside the root, the second
bias correction without its root, decay after the update, t off by one --
misses by orders of magnitude.)

bf16 parameters: m', v' as above (torch run on the widened values); p' must
be the round-to-nearest-even bf16 of the float64 p' element for element,
except where that lies within 4 * 2^-24 * |value| of a rounding tie (either
neighbour then); at most 1 % of a test's elements may use the exception.

With weight_decay 0, an element whose gradient and moments are exactly zero
keeps its p bit for bit.

Paths: the scalar path of views not aligned for 4-element accesses, ragged
bf16 tails, more than 16 tensors (several launches + the increment launch),
zero-element tensors, the prefetching grid-stride loop crossing tensors,
non-default hyper-parameters, large t, two groups, the gate words, a state
reload on the device, a late first gradient.
"""
import copy
import ctypes
import math

import pytest
import torch

import adam_ref
from gradbar import _log_fields, assert_measured_bar

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
F32, BF16 = torch.float32, torch.bfloat16

HYPERS = [
    dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0),
    dict(lr=1e-2, betas=(0.5, 0.9), eps=1e-3, weight_decay=5e-4),
    dict(lr=1e-3, betas=(0.0, 0.99), eps=1e-8, weight_decay=0.0),
]
SHAPES = [(1,), (3,), (4,), (5,), (1023,), (1024,), (1025,), (47, 33)]
SENT = -7.0  # (exact in bf16 and fp32)
PAD = 9      # sentinel elements after a view (one before it)


def _values(shape, dtype, gen):
    """Parameter values: normal; for bf16 pushed to |p| >= 0.25.  The bf16 rule
    is relative to the RESULT p', while the kernel's fp32 p - update carries
    an absolute error of ~2^-24 |p|: where the two cancel (|p| ~ lr) that is
    no longer small against p', for any fp32 implementation -- the rule
    speaks of parameters away from that cancellation (the fp32 tensors keep
    |p| ~ 0: their bar is absolute)."""
    x = torch.randn(shape, generator=gen)
    if dtype == BF16:
        x = x + torch.where(x < 0, -0.25, 0.25)
    return x.to(dtype)


class _T:
    """One parameter of a case: aligned (its own allocation) or a contiguous
    view at element offset 1 of a sentinel-filled buffer, gradient alike."""

    def __init__(self, shape, dtype, gen, view=False):
        self.shape, self.dtype, self.view = tuple(shape), dtype, view
        self.n = n = math.prod(shape)
        vals = _values(shape, dtype, gen)
        if view:
            assert len(shape) == 1
            self.buf = torch.full((n + 1 + PAD,), SENT, dtype=dtype, device=DEV)
            self.gbuf = torch.full((n + 1 + PAD,), SENT, dtype=dtype, device=DEV)
            self.buf[1:1 + n] = vals.to(DEV)
            self.p = torch.nn.Parameter(self.buf[1:1 + n])
            assert n == 0 or self.p.data_ptr() == self.buf.data_ptr() + self.buf.element_size()
        else:
            self.p = torch.nn.Parameter(vals.to(DEV))
        # ~5 % exact-zero gradients, the same elements at every step (their
        # moments stay zero), one for sure from 4 elements on
        self.zero = torch.rand(shape, generator=gen) < 0.05
        if n >= 4:
            self.zero.view(-1)[n // 2] = True

    def set_grad(self, gen, scale=1.0):
        g = (torch.randn(self.shape, generator=gen) * scale).to(self.dtype)
        g[self.zero] = 0
        if self.view:
            self.gbuf[1:1 + self.n] = g.to(DEV)
            self.p.grad = self.gbuf[1:1 + self.n]
        else:
            self.p.grad = g.to(DEV)

    def check_sentinels(self):
        if not self.view:
            return
        for b in (self.buf, self.gbuf):
            out = torch.cat([b[:1], b[1 + self.n:]]).cpu()
            assert out.numel() == 1 + PAD and bool((out == SENT).all()), "write outside the view"


class _Ties:
    """A test's tally.  Per quantity the comparison nearest its bar (logged
    once per test, with the largest raw e_ours / e_torch and the number of
    comparisons); of the bf16 elements, how many lay near a rounding tie and
    how many took the other neighbour there."""

    def __init__(self):
        self.total = self.near = self.used = 0
        self.worst = {}

    def bar(self, q, ours, base, want, name):
        e_ours, e_base, floor = assert_measured_bar(ours, base, want, msg=f"{name}:{q}")
        w = self.worst.setdefault(q, dict(n=0, to_bar=-1.0, raw=0.0))
        w["n"] += 1
        if e_base > 0:
            w["raw"] = max(w["raw"], e_ours / e_base)
        if e_ours / max(e_base, floor, 1e-300) > w["to_bar"]:
            w.update(to_bar=e_ours / max(e_base, floor, 1e-300), name=name, e_ours=e_ours, e_torch=e_base,
                     floor=floor)

    def finish(self, label):
        for q, w in sorted(self.worst.items()):
            _log_fields(tensor=f"{w['name']}:{q}", e_ours=w["e_ours"], e_torch=w["e_torch"], floor=w["floor"],
                        ratio_to_bar=w["to_bar"], comparisons=w["n"], largest_e_ours_over_e_torch=w["raw"])
        if not self.total:
            return
        _log_fields(tensor=f"{label}:bf16_ties", elements=self.total, near_tie=self.near,
                    exception_used=self.used)
        assert self.used <= 0.01 * self.total, (self.used, self.total)


def _check_bf16_rounding(got, ref64, ties, label):
    """got (bf16) == RNE_bf16(ref64) element for element; within 4 * 2^-24 *
    |value| of a tie, the other neighbour too."""
    x = ref64.reshape(-1)
    got = got.detach().cpu().reshape(-1).double()
    ax = x.abs()
    b = ax.float().view(torch.int32) & -65536  # (the fp32 rounding of |x|, its low half cut)
    b = torch.where(b.view(torch.float32).double() > ax, b - 65536, b)
    lo = b.view(torch.float32).double()           # largest bf16 <= |x|
    hi = (b + 65536).view(torch.float32).double()  # the next one
    assert bool(((lo <= ax) & (ax < hi)).all())
    mid = (lo + hi) / 2  # (exact in float64)
    even = torch.where(((b >> 16) & 1) == 0, lo, hi)
    want = torch.where(ax > mid, hi, torch.where(ax < mid, lo, even))
    sgn = torch.where(x < 0, -1.0, 1.0).double()
    near = (ax - mid).abs() <= 4 * 2.0 ** -24 * ax
    exact = got == sgn * want
    other = near & ((got == sgn * lo) | (got == sgn * hi))
    bad = ~(exact | other)
    assert not bool(bad.any()), (
        f"{label}: {int(bad.sum())} of {x.numel()} elements are not the nearest bf16; first: "
        f"ref {float(x[bad][0])!r} got {float(got[bad][0])!r} want {float((sgn * want)[bad][0])!r}")
    ties.total += x.numel()
    ties.near += int(near.sum())
    ties.used += int((other & ~exact).sum())


def _torch_step(before, t, h):
    """One step of torch.optim.Adam(capturable=True) on the device from fp32
    copies of `before` = [(p0, g, m0, v0)] (bf16 widened) with step t - 1."""
    qs = []
    for p0, g, _, _ in before:
        q = p0.float().clone().requires_grad_(True)
        q.grad = g.float().clone()
        qs.append(q)
    live = [(q, b) for q, b in zip(qs, before) if q.numel()]
    if live:
        opt = torch.optim.Adam([q for q, _ in live], capturable=True, **h)
        for q, (_, _, m0, v0) in live:
            opt.state[q] = dict(step=torch.tensor(float(t - 1), dtype=F32, device=DEV),
                                exp_avg=m0.clone().reshape(q.shape), exp_avg_sq=v0.clone().reshape(q.shape))
        opt.step()
        for q, _ in live:
            assert float(opt.state[q]["step"]) == t
        st = {id(q): opt.state[q] for q, _ in live}
    return [(q.detach(), st[id(q)]["exp_avg"], st[id(q)]["exp_avg_sq"]) if q.numel() else (q.detach(), None, None)
            for q in qs]


def _compare(label, t, h, before, after, ties):
    """after = [(p', m', v')] of ours from before = [(p0, g, m0, v0)], step t."""
    base = _torch_step(before, t, h)
    for k, ((p0, g, m0, v0), (p1, m1, v1), (pt, mt, vt)) in enumerate(zip(before, after, base)):
        if p0.numel() == 0:
            continue
        bf = p0.dtype == BF16
        name = f"{label}:t{t}:{k}:{'bf16' if bf else 'f32'}[{p0.numel()}]"
        c = [x.detach().cpu() for x in (p0, g, m0, v0)]
        step = adam_ref.adam_step_bf16 if bf else adam_ref.adam_step
        args = (c[0], c[1]) if bf else (c[0].double(), c[1].double())
        pr, mr, vr = step(*args, c[2].double().reshape(c[0].shape), c[3].double().reshape(c[0].shape), t,
                          h["lr"], h["betas"], h["eps"], h["weight_decay"])
        assert m1.dtype == F32 and v1.dtype == F32 and p1.dtype == p0.dtype
        ties.bar("m", m1, mt, mr, name)
        ties.bar("v", v1, vt, vr, name)
        if bf:
            _check_bf16_rounding(p1, pr, ties, name + ":p")
        else:
            ties.bar("p", p1, pt, pr, name)
        if h["weight_decay"] == 0:
            still = ((c[1] == 0) & (c[2].reshape(c[0].shape) == 0) & (c[3].reshape(c[0].shape) == 0)).reshape(-1)
            iv = torch.int16 if bf else torch.int32
            a = p1.detach().cpu().reshape(-1).view(iv)[still]
            assert torch.equal(a, c[0].reshape(-1).view(iv)[still]), name + ": a zero gradient moved p"


def _snapshot(opt, ts):
    out = []
    for T in ts:
        st = opt.state.get(T.p, {})
        m0 = st["exp_avg"].clone() if "exp_avg" in st else torch.zeros(T.shape, dtype=F32, device=DEV)
        v0 = st["exp_avg_sq"].clone() if "exp_avg_sq" in st else torch.zeros(T.shape, dtype=F32, device=DEV)
        out.append((T.p.detach().clone(), T.p.grad.clone(), m0, v0))
    return out


def _tickets_zero(opt):
    return all(int(tk.count_nonzero()) == 0 for tk in opt._tickets.values())


def _run(label, groups, gen, steps=3, pre=None, t_of=lambda it: it + 1, ties=None):
    """groups: [(tensors, hyper)] -> the optimizer after `steps` teacher-forced
    steps.  pre(opt, it): called before step `it` (after the gradients)."""
    from ngnn.optim import Adam
    own = ties is None
    ties = _Ties() if own else ties
    opt = Adam([dict(params=[T.p for T in ts], **h) for ts, h in groups])
    for it in range(steps):
        for ts, _ in groups:
            for T in ts:
                T.set_grad(gen, scale=float(it + 1))
        if pre is not None:
            pre(opt, it)
        before = [_snapshot(opt, ts) for ts, _ in groups]
        opt.step()
        torch.cuda.synchronize()
        assert _tickets_zero(opt)
        for gi, ((ts, h), bef) in enumerate(zip(groups, before)):
            sts = [opt.state[T.p] for T in ts]
            assert float(sts[0]["step"]) == t_of(it)
            assert all(st["step"] is sts[0]["step"] for st in sts)
            after = [(T.p.detach(), st["exp_avg"], st["exp_avg_sq"]) for T, st in zip(ts, sts)]
            _compare(f"{label}:g{gi}", t_of(it), h, bef, after, ties)
            for T in ts:
                T.check_sentinels()
    if own:
        ties.finish(label)
    return opt


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("hi", range(len(HYPERS)))
def test_hyper_parameters_and_shapes(hi, dtype):
    """Each shape alone (a grid of one workgroup up to two, vector body and
    ragged tail), then all in one call."""
    gen = torch.Generator().manual_seed(100 + hi)
    ties = _Ties()
    zeros = 0
    for shape in SHAPES:
        T = _T(shape, dtype, gen)
        zeros += int(T.zero.sum())
        _run(f"hyper{hi}:{shape}", [([T], HYPERS[hi])], gen, ties=ties)
    assert zeros >= 5  # (the zero-gradient rule was exercised)
    _run(f"hyper{hi}:all", [([_T(s, dtype, gen) for s in SHAPES], HYPERS[hi])], gen, ties=ties)
    ties.finish(f"hyper{hi}")


def test_unaligned_views_take_the_scalar_path_inside_their_bounds():
    """Parameters and gradients that are contiguous views at element offset 1
    (the data-parallel bucket's gradient views are such): vec[k] == 0, the
    per-element path for the whole tensor, mixed with aligned tensors in one
    launch; nothing outside the views is written."""
    gen = torch.Generator().manual_seed(7)
    ts = [_T((47, 33), F32, gen), _T((7,), F32, gen, view=True), _T((7,), BF16, gen, view=True),
          _T((1025,), BF16, gen), _T((2050,), F32, gen, view=True), _T((2050,), BF16, gen, view=True),
          _T((5,), F32, gen)]
    assert ts[1].p.data_ptr() % 16 == 4 and ts[2].p.data_ptr() % 8 == 2
    _run("views", [(ts, HYPERS[1])], gen)
    gen = torch.Generator().manual_seed(8)
    ts = [_T((2050,), BF16, gen, view=True), _T((4,), BF16, gen), _T((7,), F32, gen, view=True)]
    _run("views_nowd", [(ts, HYPERS[0])], gen)


def _ptrs(ts):
    return (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


def _raw_step(items, step, ticket, h, gate=None, gate_gen=None):
    """ngnn_adam_step through the C ABI: items = [(p, g, m, v)] device tensors."""
    from ngnn import _lib
    n = len(items)
    N = (ctypes.c_int64 * n)(*[it[0].numel() for it in items])
    D = (ctypes.c_int32 * n)(*[_lib.BF16 if it[0].dtype == BF16 else _lib.F32 for it in items])
    rc = _lib.load().ngnn_adam_step(
        n, _ptrs([it[0] for it in items]), _ptrs([it[1] for it in items]), _ptrs([it[2] for it in items]),
        _ptrs([it[3] for it in items]), N, D, step.data_ptr(), _lib.ptr(ticket),
        h["lr"], h["betas"][0], h["betas"][1], h["eps"], h["weight_decay"],
        _lib.ptr(gate), _lib.ptr(gate_gen), _lib.stream_handle(DEV))
    torch.cuda.synchronize()
    return rc


def _raw_items(sizes, gen, odd_moments=False):
    """[(p, g, m, v)] with non-trivial moments; odd_moments: every one of the
    four a view at element offset 1 of a sentinel-filled buffer."""
    items, bufs = [], []
    for n, dtype in sizes:
        vals = [_values((n,), dtype, gen), torch.randn(n, generator=gen).to(dtype),
                torch.randn(n, generator=gen) * 0.1, torch.rand(n, generator=gen) * 0.01]
        if odd_moments:
            row = []
            for x in vals:
                b = torch.full((n + 1 + PAD,), SENT, dtype=x.dtype, device=DEV)
                b[1:1 + n] = x.to(DEV)
                bufs.append((b, n))
                row.append(b[1:1 + n])
            items.append(tuple(row))
        else:
            items.append(tuple(x.to(DEV) for x in vals))
    return items, bufs


def test_raw_abi_odd_offset_moments():
    """exp_avg / exp_avg_sq as odd-offset views too (4-B aligned only): the
    scalar path for every operand, inside the views' bounds."""
    gen = torch.Generator().manual_seed(21)
    items, bufs = _raw_items([(7, F32), (2050, F32), (7, BF16), (2050, BF16), (1024, F32)], gen,
                             odd_moments=True)
    aligned, _ = _raw_items([(1025, F32)], gen)
    items = items[:2] + aligned + items[2:]
    step = torch.full((), 4.0, device=DEV)
    ticket = torch.zeros(1024, dtype=torch.int32, device=DEV)
    before = [tuple(x.clone() for x in it) for it in items]
    assert _raw_step(items, step, ticket, HYPERS[1], None, None) == 0
    assert float(step) == 5.0 and int(ticket.count_nonzero()) == 0
    ties = _Ties()
    _compare("raw_odd", 5, HYPERS[1], before, [(it[0], it[2], it[3]) for it in items], ties)
    ties.finish("raw_odd")
    assert len(bufs) == 20
    for b, n in bufs:
        out = torch.cat([b[:1], b[1 + n:]]).cpu()
        assert bool((out == SENT).all()), "write outside a view"
    for it, bef in zip(items, before):  # (the gradients are read only)
        assert torch.equal(it[1], bef[1])


@pytest.mark.parametrize("n_tensors", [17, 33])
def test_more_than_16_tensors(n_tensors):
    """The ticket-less path: launches of 16 tensors each reading *step, then
    the increment launch; the count advances once per step() and the ticket
    (not used) stays zero."""
    gen = torch.Generator().manual_seed(n_tensors)
    sizes = [0, 1, 3, 4, 5, 1023, 1024, 1025]
    ts = [_T((sizes[k % 8],), BF16 if k % 3 == 1 else F32, gen) for k in range(n_tensors)]
    _run(f"many{n_tensors}", [(ts, HYPERS[1])], gen)


@pytest.mark.parametrize("where", ["first", "middle", "last", "all"])
def test_zero_element_tensors(where):
    """Empty tensors are skipped by the workgroup -> tensor search wherever
    they stand; a list of only empty tensors still advances the count by one,
    as torch's Adam does."""
    gen = torch.Generator().manual_seed(31)
    full = [(1025,), (3,), (4,), (1023,), (5,)]
    empty = {"first": {0}, "middle": {2}, "last": {4}, "all": {0, 1, 2, 3, 4}}[where]
    ts = [_T((0,) if k in empty else full[k], BF16 if k == 3 else F32, gen) for k in range(5)]
    opt = _run(f"empty_{where}", [(ts, HYPERS[0])], gen)
    # torch: an empty parameter's step advances with every step() as well
    q = torch.zeros(0, device=DEV, requires_grad=True)
    to = torch.optim.Adam([q], capturable=True)
    for _ in range(3):
        q.grad = torch.zeros(0, device=DEV)
        to.step()
    assert float(to.state[q]["step"]) == float(opt.state[ts[0].p]["step"]) == 3.0


@pytest.mark.parametrize("big", [F32, BF16], ids=["f32", "bf16"])
def test_prefetch_loop_crosses_tensor_boundaries(big):
    """More virtual workgroups than the grid cap (2 per CU): workgroups whose
    second trip leaves the large aligned tensor for its ragged tail, an
    odd-offset view, (an empty tensor,) and a 1-element tensor -- the
    operands prefetched for one kind while the other is applied."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    gen = torch.Generator().manual_seed(41)
    ts = [_T(((2 * cus + 40) * 1024 + 3,), big, gen), _T((1500,), F32, gen, view=True),
          _T((0,), F32, gen), _T((1,), BF16, gen)]
    _run("prefetch", [(ts, HYPERS[1])], gen)


def test_large_step_counts():
    """t = 1000 and t = 100000 (the device count set by fill_): powf at large
    exponents inside the same measured bar."""
    gen = torch.Generator().manual_seed(51)
    ts = [_T((1025,), F32, gen), _T((47, 33), BF16, gen), _T((5,), F32, gen)]
    t_of = {0: 1, 1: 1000, 2: 100000}

    def pre(opt, it):
        if it:
            opt.state[ts[0].p]["step"].fill_(t_of[it] - 1)

    _run("large_t", [(ts, HYPERS[0])], gen, pre=pre, t_of=t_of.get)


def test_two_parameter_groups():
    """Two groups, two learning rates and decays: two counters, two tickets,
    each group by its own hyper-parameters."""
    gen = torch.Generator().manual_seed(61)
    a = [_T((1025,), F32, gen), _T((7,), BF16, gen)]
    b = [_T((47, 33), F32, gen), _T((3,), F32, gen), _T((1024,), BF16, gen)]
    opt = _run("groups", [(a, HYPERS[0]), (b, HYPERS[1])], gen)
    s0, s1 = opt.state[a[0].p]["step"], opt.state[b[0].p]["step"]
    assert s0.data_ptr() != s1.data_ptr() and len(opt._tickets) == 2
    assert opt._tickets[s0.data_ptr()].data_ptr() != opt._tickets[s1.data_ptr()].data_ptr()
    # the second group stepping alone advances its counter only
    for T in a:
        T.p.grad = None
    for T in b:
        T.set_grad(gen)
    opt.step()
    torch.cuda.synchronize()
    assert float(s0) == 3.0 and float(s1) == 4.0 and _tickets_zero(opt)


@pytest.mark.parametrize("n_tensors", [3, 17], ids=["ticketed", "over16"])
def test_gate_words(n_tensors):
    """gate = (generation << 32 | bad bits), gate_gen's high half the current
    generation (csrc/ngnn_internal.h slot_gated).  Bad bits set in the current
    generation: p, m, v and the count bitwise untouched, every ticket word
    zero.  A stale generation, or no bad bits: the normal update."""
    gen = torch.Generator().manual_seed(71)
    sizes = [(1025, F32), (7, BF16), (1024, BF16), (3, F32)]
    items, _ = _raw_items([sizes[k % 4] for k in range(n_tensors)], gen)
    step = torch.full((), 2.0, device=DEV)
    ticket = torch.zeros(1024, dtype=torch.int32, device=DEV)
    word = lambda hi, lo: torch.tensor([(hi << 32) | lo], dtype=torch.int64, device=DEV)  # noqa: E731
    before = [tuple(x.clone() for x in it) for it in items]
    assert _raw_step(items, step, ticket, HYPERS[1], word(5, 1), word(5, 77)) == 0
    assert float(step) == 2.0 and int(ticket.count_nonzero()) == 0
    for it, bef in zip(items, before):
        for x, y in zip(it, bef):
            iv = torch.int16 if x.dtype == BF16 else torch.int32
            assert torch.equal(x.view(iv), y.view(iv)), "a gated step wrote"
    t = 2
    for gate in (word(4, 1), word(5, 0)):  # stale generation; current one, no bad bits
        before = [tuple(x.clone() for x in it) for it in items]
        assert _raw_step(items, step, ticket, HYPERS[1], gate, word(5, 77)) == 0
        t += 1
        assert float(step) == t and int(ticket.count_nonzero()) == 0
        ties = _Ties()
        _compare(f"gate{n_tensors}", t, HYPERS[1], before, [(it[0], it[2], it[3]) for it in items], ties)
        ties.finish(f"gate{n_tensors}")


def _cpu_state(sd):
    sd = copy.deepcopy(sd)
    for st in sd["state"].values():
        for k, v in st.items():
            if isinstance(v, torch.Tensor):
                st[k] = v.cpu()
    return sd


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_reload_on_the_device(dtype):
    """Three steps, state_dict() -> a deep copy on the CPU -> a fresh Adam over
    cloned parameters, two more steps: bit for bit the optimizer that never
    reloaded (a bf16 model's fp32 moments come back as saved), fp32 moments,
    one shared step, and the Adam fold still available to the fp32 SAGE."""
    import ngnn
    from ngnn import fused
    from ngnn.optim import Adam
    torch.manual_seed(81)
    gen = torch.Generator().manual_seed(82)
    m1 = ngnn.SAGE(100, 256, 47, 2, dropout=0.5).to(DEV).to(dtype)
    o1 = Adam(m1.parameters(), lr=1e-2, weight_decay=5e-4)

    def grads(models):
        for ps in zip(*[m.parameters() for m in models]):
            g = torch.randn(ps[0].shape, generator=gen).to(dtype).to(DEV)
            for p in ps:
                p.grad = g.clone()

    for _ in range(3):
        grads([m1])
        o1.step()
    m2 = copy.deepcopy(m1)
    o2 = Adam(m2.parameters(), lr=1e-2, weight_decay=5e-4)
    o2.load_state_dict(_cpu_state(o1.state_dict()))
    p2 = list(m2.parameters())
    step2 = o2.state[p2[0]]["step"]
    assert step2.is_cuda and step2.dtype == F32 and float(step2) == 3.0
    assert step2.data_ptr() != o1.state[next(m1.parameters())]["step"].data_ptr()
    for q in p2:
        st = o2.state[q]
        assert st["step"] is step2
        for k in ("exp_avg", "exp_avg_sq"):
            assert st[k].dtype == F32 and st[k].is_cuda and st[k].shape == q.shape and st[k].is_contiguous()
    if dtype == F32:
        assert fused.AdamFoldSpec.make(o2, m2) is not None
    for _ in range(2):
        grads([m1, m2])
        o1.step()
        o2.step()
    torch.cuda.synchronize()
    assert float(step2) == 5.0 == float(o1.state[next(m1.parameters())]["step"])
    iv = torch.int16 if dtype == BF16 else torch.int32
    for a, b in zip(m1.parameters(), p2):
        assert torch.equal(a.detach().view(iv), b.detach().view(iv))
        for k in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(o1.state[a][k].view(torch.int32), o2.state[b][k].view(torch.int32))
    assert _tickets_zero(o1) and _tickets_zero(o2)


def test_step_refuses_a_bf16_moment_before_any_launch():
    """The state torch's own load_state_dict leaves for a bf16 model (moments
    of half the bytes the kernel writes): step() raises, nothing is touched."""
    from ngnn.optim import Adam
    p = torch.nn.Parameter(torch.randn(1024).to(BF16).to(DEV))
    opt = Adam([p])
    opt.state[p] = dict(step=torch.zeros((), device=DEV), exp_avg=torch.zeros(1024, dtype=BF16, device=DEV),
                        exp_avg_sq=torch.zeros(1024, dtype=BF16, device=DEV))
    p.grad = torch.ones_like(p)
    p0 = p.detach().clone()
    with pytest.raises(RuntimeError, match="not float32"):
        opt.step()
    torch.cuda.synchronize()
    assert torch.equal(p.detach().view(torch.int16), p0.view(torch.int16))
    assert float(opt.state[p]["step"]) == 0.0


@pytest.mark.parametrize("late_first", [True, False], ids=["late_is_first", "late_is_second"])
def test_late_first_gradient_raises(late_first):
    """One step count per group: a parameter whose first gradient arrives after
    the group's state was made raises before any state is touched (it used to
    zero the other's moments and count, or die of a KeyError)."""
    from ngnn.optim import Adam
    gen = torch.Generator().manual_seed(91)
    a = torch.nn.Parameter(torch.randn(1025, generator=gen).to(DEV))
    b = torch.nn.Parameter(torch.randn(47, 33, generator=gen).to(DEV))
    opt = Adam([a, b] if late_first else [b, a], lr=1e-2)
    b.grad = torch.randn(b.shape, generator=gen).to(DEV)
    opt.step()
    torch.cuda.synchronize()
    st = opt.state[b]
    keep = (b.detach().clone(), st["exp_avg"].clone(), st["exp_avg_sq"].clone(), a.detach().clone())
    assert float(st["step"]) == 1.0 and float(st["exp_avg"].abs().max()) > 0
    a.grad = torch.randn(a.shape, generator=gen).to(DEV)
    b.grad = torch.randn(b.shape, generator=gen).to(DEV)
    with pytest.raises(RuntimeError, match="one step count per group"):
        opt.step()
    torch.cuda.synchronize()
    assert opt.state[b] is st and float(st["step"]) == 1.0 and "step" not in opt.state.get(a, {})
    for x, y in zip((b.detach(), st["exp_avg"], st["exp_avg_sq"], a.detach()), keep):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    # a gradient that becomes None later: that parameter is left out, as before
    a.grad = None
    opt.step()
    torch.cuda.synchronize()
    assert float(st["step"]) == 2.0 and torch.equal(a.detach(), keep[3])
