"""ngnn.optim.Adam's state after a reload (no kernel launches: state made by
hand, as tests/test_step_fusions_cpu.py::_with_state does).

torch.optim.Optimizer.load_state_dict casts every floating-point state tensor
to its parameter's dtype: for a bf16 model the moments come back bf16, in
buffers of half the bytes ngnn_adam_step reads and writes per element.
Adam.load_state_dict restores what the kernel needs -- per group one shared
fp32 step tensor, per parameter contiguous fp32 moments of its shape -- and
step()'s check (optim.check_moment) refuses anything else before a launch.
"""
import io

import pytest
import torch

from ngnn import optim
from ngnn.optim import Adam


def _params(dtype, seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(s, generator=g).to(dtype)) for s in [(5, 3), (7,), (1,), (2, 3, 4)]]


def _with_state(opt, counts, seed=1):
    """fp32 moments and one shared step tensor per group (what a first step
    makes), with values that bf16 cannot hold exactly."""
    g = torch.Generator().manual_seed(seed)
    for group, c in zip(opt.param_groups, counts):
        step = torch.tensor(float(c))
        for p in group["params"]:
            opt.state[p] = dict(step=step, exp_avg=torch.randn(p.shape, generator=g),
                                exp_avg_sq=torch.rand(p.shape, generator=g) + 2.0 ** -12)


def _roundtrip(sd, how):
    if how == "direct":
        return sd
    buf = io.BytesIO()
    torch.save(sd, buf)
    buf.seek(0)
    return torch.load(buf)


def _check_layout(opt, counts):
    steps = []
    for group, c in zip(opt.param_groups, counts):
        step = opt.state[group["params"][0]]["step"]
        assert step.dtype == torch.float32 and step.numel() == 1 and float(step) == float(c)
        assert step.device == group["params"][0].device
        for p in group["params"]:
            st = opt.state[p]
            assert st["step"] is step  # ONE counter per group: the kernel advances one address
            for k in ("exp_avg", "exp_avg_sq"):
                m = st[k]
                assert m.dtype == torch.float32 and m.shape == p.shape and m.is_contiguous()
                assert m.device == p.device
                optim.check_moment(p, m, k)
            optim.check_step(p, step)
        steps.append(step)
    return steps


@pytest.mark.parametrize("how", ["direct", "save_load"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_reload_keeps_fp32_moments_and_one_step_per_group(dtype, how):
    ps = _params(dtype)
    src = Adam([{"params": ps[:2]}, {"params": ps[2:], "lr": 1e-2}])
    _with_state(src, counts=(3, 7))
    sd = _roundtrip(src.state_dict(), how)
    qs = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    dst = Adam([{"params": qs[:2]}, {"params": qs[2:], "lr": 1e-2}])
    dst.load_state_dict(sd)
    s0, s1 = _check_layout(dst, counts=(3, 7))
    assert s0 is not s1 and s0.data_ptr() != s1.data_ptr()  # two groups keep two counters
    assert s0 is not src.state[ps[0]]["step"]  # and none shared with the optimizer saved from
    for p, q in zip(ps, qs):
        for k in ("exp_avg", "exp_avg_sq"):
            # exactly the saved fp32 values, also under a bf16 parameter
            # (torch's rounding of them to the parameter's dtype is dropped)
            assert torch.equal(dst.state[q][k], src.state[p][k])
            assert dst.state[q][k].data_ptr() != src.state[p][k].data_ptr()
    # a second trip through the same optimizer changes nothing
    dst.load_state_dict(_roundtrip(dst.state_dict(), how))
    _check_layout(dst, counts=(3, 7))


def test_bf16_moments_in_a_saved_state_are_widened():
    """A checkpoint written around Adam.load_state_dict (the moments already
    bf16): the loaded moments are fp32 with exactly those values."""
    ps = _params(torch.bfloat16)
    opt = Adam(ps)
    _with_state(opt, counts=(4,))
    sd = opt.state_dict()
    for st in sd["state"].values():
        st["exp_avg"] = st["exp_avg"].to(torch.bfloat16)
        st["exp_avg_sq"] = st["exp_avg_sq"].to(torch.bfloat16)
    want = {k: (st["exp_avg"].float(), st["exp_avg_sq"].float()) for k, st in sd["state"].items()}
    opt.load_state_dict(sd)
    _check_layout(opt, counts=(4,))
    for k, p in enumerate(ps):
        assert torch.equal(opt.state[p]["exp_avg"], want[k][0])
        assert torch.equal(opt.state[p]["exp_avg_sq"], want[k][1])


def test_per_parameter_step_copies_are_merged():
    """torch's per-parameter .to() across devices leaves every parameter its
    own copy of step (equal values): one shared tensor again after the load."""
    ps = _params(torch.float32)
    opt = Adam(ps)
    _with_state(opt, counts=(5,))
    sd = opt.state_dict()
    for st in sd["state"].values():
        st["step"] = st["step"].clone()
    opt.load_state_dict(sd)
    _check_layout(opt, counts=(5,))


def test_differing_step_counts_in_a_group_raise_and_load_nothing():
    ps = _params(torch.float32)
    opt = Adam([{"params": ps[:2]}, {"params": ps[2:]}])
    _with_state(opt, counts=(3, 3))
    sd = opt.state_dict()
    sd["state"][3]["step"] = torch.tensor(9.0)  # group 1: counts 3 and 9
    before = {p: dict(opt.state[p]) for p in ps}
    with pytest.raises(RuntimeError, match="one step count per group"):
        opt.load_state_dict(sd)
    for p in ps:  # nothing was loaded
        assert all(opt.state[p][k] is before[p][k] for k in before[p])
    # different counts in DIFFERENT groups are what two counters are for
    sd["state"][2]["step"] = torch.tensor(9.0)
    opt.load_state_dict(sd)
    _check_layout(opt, counts=(3, 9))


def test_a_moment_of_another_size_is_refused_at_load():
    ps = _params(torch.float32)
    opt = Adam(ps)
    _with_state(opt, counts=(1,))
    sd = opt.state_dict()
    sd["state"][1]["exp_avg_sq"] = torch.zeros(6)
    with pytest.raises(RuntimeError, match="6 elements"):
        opt.load_state_dict(sd)


def test_check_moment():
    """The check step() makes before a launch whenever the state's tensors
    changed: fp32, the parameter's device and numel, contiguous."""
    p = torch.nn.Parameter(torch.zeros(4, 6, dtype=torch.bfloat16))
    optim.check_moment(p, torch.zeros(4, 6), "exp_avg")
    optim.check_moment(p, torch.zeros(24), "exp_avg")  # (addresses only: the shape is not the kernel's concern)
    with pytest.raises(RuntimeError, match="bfloat16"):  # what torch's load leaves for a bf16 model
        optim.check_moment(p, torch.zeros(4, 6, dtype=torch.bfloat16), "exp_avg")
    with pytest.raises(RuntimeError, match="23 elements"):
        optim.check_moment(p, torch.zeros(23), "exp_avg_sq")
    with pytest.raises(RuntimeError, match="not contiguous"):
        optim.check_moment(p, torch.zeros(6, 4).t(), "exp_avg")
    with pytest.raises(RuntimeError, match="not a tensor"):
        optim.check_moment(p, None, "exp_avg")
    with pytest.raises(RuntimeError, match="meta"):
        optim.check_moment(p, torch.zeros(4, 6, device="meta"), "exp_avg")
    optim.check_step(p, torch.zeros(()))
    for bad in (torch.zeros((), dtype=torch.float64), torch.zeros(2), 3.0, torch.zeros((), device="meta")):
        with pytest.raises(RuntimeError, match="step"):
            optim.check_step(p, bad)


def test_torchs_own_load_is_what_the_override_repairs():
    """The premise (torch 2.x): Optimizer.load_state_dict alone hands a bf16
    model bf16 moments -- which check_moment refuses."""
    ps = _params(torch.bfloat16)
    opt = Adam(ps)
    _with_state(opt, counts=(2,))
    torch.optim.Optimizer.load_state_dict(opt, opt.state_dict())
    m = opt.state[ps[0]]["exp_avg"]
    assert m.dtype == torch.bfloat16
    with pytest.raises(RuntimeError, match="not float32"):
        optim.check_moment(ps[0], m, "exp_avg")
