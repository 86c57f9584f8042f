"""Adam on the device in one launch (ngnn_adam_step): the update over every
parameter tensor; its last workgroup advances the step count.

Same rule and hyper-parameters as ``torch.optim.Adam`` (the reference's
optimiser, model.py:66-69; amsgrad / maximize / foreach variants not
offered); the step count is a device tensor, so the step is capturable in a
HIP graph (``ngnn.graphs.GraphedTrainStep``).  State keys follow torch:
``step``, ``exp_avg``, ``exp_avg_sq``.

What the state is, whatever made it (the first step or ``load_state_dict``):
per group ONE fp32 ``step`` tensor on the parameters' device, shared by every
parameter of the group (the kernel advances one counter), and per parameter
contiguous fp32 moments of its shape on its device -- also for a bf16
parameter.  ``torch.optim.Optimizer.load_state_dict`` alone casts the moments
to the parameter's dtype (bf16 buffers of half the bytes the kernel writes)
and copies ``step`` per parameter; ``Adam.load_state_dict`` restores the
layout (the moments from the saved tensors, so fp32 ones exactly), and
``step()`` checks it before a launch whenever the tensors changed.
One counter per group: loaded counts that differ within a group, and a
parameter whose first gradient arrives after the group's state was made,
raise (torch keeps a count per parameter there).
"""
from __future__ import annotations

import ctypes

import torch

from . import _lib


# (gate word, generation word) of the graph slot whose step is being
# captured (ngnn.graphs sets it around a one-rank capture): the captured
# Adam launch skips the update of a block that broke the slot's contract
# (ABI 20; include/ngnn.h ngnn_adam_step)
_slot_gate = None


def check_moment(p: torch.Tensor, t, name: str) -> None:
    """The kernel reads and writes p.numel() fp32 values at t's address:
    anything else (a bf16 moment of a reloaded bf16 model, a tensor of
    another size, device or layout) is an error before the launch."""
    if not isinstance(t, torch.Tensor):
        raise RuntimeError(f"ngnn.optim.Adam: state[{name!r}] is not a tensor")
    if t.dtype != torch.float32:
        raise RuntimeError(f"ngnn.optim.Adam: state[{name!r}] is {t.dtype}, not float32 (a state "
                           "loaded around Adam.load_state_dict?)")
    if t.device != p.device:
        raise RuntimeError(f"ngnn.optim.Adam: state[{name!r}] is on {t.device}, its parameter on {p.device}")
    if t.numel() != p.numel():
        raise RuntimeError(f"ngnn.optim.Adam: state[{name!r}] has {t.numel()} elements, its parameter "
                           f"{p.numel()}")
    if not t.is_contiguous():
        raise RuntimeError(f"ngnn.optim.Adam: state[{name!r}] is not contiguous")


def check_step(p: torch.Tensor, step) -> None:
    """The group's one device counter: a single fp32 value on p's device."""
    if not isinstance(step, torch.Tensor) or step.dtype != torch.float32 or step.numel() != 1 \
            or step.device != p.device:
        raise RuntimeError("ngnn.optim.Adam: state['step'] must be one float32 value on the "
                           "parameters' device")


class Adam(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
        if lr < 0 or eps < 0 or weight_decay < 0 or not (0 <= betas[0] < 1 and 0 <= betas[1] < 1):
            raise ValueError("invalid Adam hyper-parameters")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay,
                                      capturable=True))
        self._tickets: dict = {}  # step tensor address -> device ticket
        # per group: (parameter addresses, the launch's pointer arrays) -- the
        # eager step is host-bound, and only the gradient addresses change
        # from step to step
        self._arrays: dict = {}

    def load_state_dict(self, state_dict):
        """torch's load, then the layout this optimizer keeps (module
        docstring); moments saved as bf16 are widened, their values kept.
        Step counts that differ within a group, and a moment of another size
        than its parameter, raise before anything is loaded."""
        counts = []
        for g in state_dict["param_groups"]:
            vals = {float(state_dict["state"][k]["step"]) for k in g["params"]
                    if "step" in state_dict["state"].get(k, {})}
            if len(vals) > 1:
                raise RuntimeError("ngnn.optim.Adam: the loaded step counts differ within a parameter "
                                   f"group ({sorted(vals)}); one step count per group")
            counts.append(vals.pop() if vals else None)
            for k in g["params"]:
                for name in ("exp_avg", "exp_avg_sq"):
                    t = state_dict["state"].get(k, {}).get(name)
                    if isinstance(t, torch.Tensor) and not t.is_floating_point():
                        raise RuntimeError(f"ngnn.optim.Adam: loaded state[{name!r}] is {t.dtype}")
        if len(state_dict["param_groups"]) == len(self.param_groups):  # (else: torch's error below)
            for g, sg in zip(self.param_groups, state_dict["param_groups"]):
                for p, k in zip(g["params"], sg["params"]):
                    for name in ("exp_avg", "exp_avg_sq"):
                        t = state_dict["state"].get(k, {}).get(name)
                        if isinstance(t, torch.Tensor) and t.numel() != p.numel():
                            raise RuntimeError(f"ngnn.optim.Adam: loaded state[{name!r}] has {t.numel()} "
                                               f"elements, its parameter {p.numel()}")
        super().load_state_dict(state_dict)
        self._arrays.clear()
        self._tickets.clear()
        for group, sg, count in zip(self.param_groups, state_dict["param_groups"], counts):
            live = [(p, k) for p, k in zip(group["params"], sg["params"]) if "step" in self.state.get(p, {})]
            if not live:
                continue
            step = torch.full((), count, dtype=torch.float32, device=live[0][0].device)
            for p, k in live:
                st = self.state[p]
                st["step"] = step
                for name in ("exp_avg", "exp_avg_sq"):
                    # from the tensor that was SAVED, not torch's cast of it to
                    # the parameter's dtype: a bf16 model's fp32 moments come
                    # back as they were (a copy: never the saved tensor itself)
                    t = state_dict["state"][k][name]
                    st[name] = t.to(device=p.device, dtype=torch.float32, copy=True) \
                        .reshape(p.shape).contiguous()

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        lib = _lib.load()
        for gi, group in enumerate(self.param_groups):
            ps = [p for p in group["params"] if p.grad is not None]
            if not ps:
                continue
            # (address, numel, dtype, contiguity) per parameter: a parameter
            # replaced by one of another size or dtype that the caching
            # allocator placed at the same address re-runs the checks and
            # rebuilds the arrays
            pkey = tuple((p.data_ptr(), p.numel(), p.dtype, p.is_contiguous()) for p in ps)
            cached = self._arrays.get(gi)
            if cached is None or cached[0][0] != pkey:
                cached = None
                for p in ps:  # (the parameters' own checks: once per parameter set)
                    if not p.is_cuda or p.dtype not in (torch.float32, torch.bfloat16) \
                            or not p.is_contiguous():
                        raise RuntimeError("ngnn.optim.Adam: contiguous float32 / bfloat16 GPU "
                                           "parameters only")
            for p in ps:
                g = p.grad
                if g.dtype != p.dtype:
                    raise RuntimeError("ngnn.optim.Adam: gradient dtype differs from the parameter")
                if g.is_sparse:
                    raise RuntimeError("ngnn.optim.Adam: dense gradients only")
            sts = [self.state.get(p) or {} for p in ps]
            if not all("step" in st for st in sts):
                # the first step makes the group's state -- for a group that
                # has it, a parameter without (its first gradient arrived
                # late) would need a step count of its own
                if any("step" in self.state.get(p, {}) for p in group["params"]):
                    raise RuntimeError(
                        "ngnn.optim.Adam: a parameter received its first gradient after its "
                        "group's state was made; the device keeps one step count per group "
                        "(give every parameter of the group a gradient at the first step, or "
                        "put the late one in a group of its own)")
                step = torch.zeros((), dtype=torch.float32, device=ps[0].device)
                for p in ps:
                    st = self.state[p]
                    st["step"] = step  # one device counter per group
                    st["exp_avg"] = torch.zeros_like(p, dtype=torch.float32,
                                                     memory_format=torch.contiguous_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, dtype=torch.float32,
                                                        memory_format=torch.contiguous_format)
                sts = [self.state[p] for p in ps]
            step = sts[0]["step"]
            grads = [p.grad if p.grad.is_contiguous() else p.grad.contiguous() for p in ps]
            n = len(ps)
            G = (ctypes.c_void_p * n)(*[g.data_ptr() for g in grads])
            # (the moments' and the count's addresses belong to the key: a
            # state reload -- load_state_dict -- makes new tensors)
            key = (pkey, tuple(st["exp_avg"].data_ptr() for st in sts),
                   tuple(st["exp_avg_sq"].data_ptr() for st in sts),
                   tuple(st["step"].data_ptr() for st in sts))
            if cached is None or cached[0] != key:
                # the state's own checks, once per parameter set or reload:
                # the kernel takes addresses only
                check_step(ps[0], step)
                for p, st in zip(ps, sts):
                    if st["step"] is not step:
                        raise RuntimeError("ngnn.optim.Adam: the parameters of a group must share "
                                           "one step tensor (one step count per group)")
                    check_moment(p, st["exp_avg"], "exp_avg")
                    check_moment(p, st["exp_avg_sq"], "exp_avg_sq")
                cached = (key, (ctypes.c_void_p * n)(*[k[0] for k in pkey]),
                          (ctypes.c_void_p * n)(*key[1]), (ctypes.c_void_p * n)(*key[2]),
                          (ctypes.c_int64 * n)(*[p.numel() for p in ps]),
                          (ctypes.c_int32 * n)(*[_lib.BF16 if p.dtype == torch.bfloat16 else _lib.F32
                                                 for p in ps]))
                self._arrays[gi] = cached
            ticket = self._tickets.get(step.data_ptr())
            if ticket is None:  # zero once; the kernel re-zeroes it after every use
                ticket = torch.zeros(1024, dtype=torch.int32, device=step.device)  # (ABI 21: two levels, a line per group)
                self._tickets[step.data_ptr()] = ticket
            _, P, M, V, N, D = cached
            b1, b2 = group["betas"]
            _lib.check(lib.ngnn_adam_step(n, P, G, M, V, N, D, step.data_ptr(), ticket.data_ptr(),
                                          float(group["lr"]),
                                          float(b1), float(b2), float(group["eps"]),
                                          float(group["weight_decay"]),
                                          *(_slot_gate if _slot_gate is not None else (None, None)),
                                          _lib.stream_handle(ps[0].device)), "ngnn_adam_step")
        return loss
