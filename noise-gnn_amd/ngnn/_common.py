"""Two helpers every op module shares: the per-device "bad entry" counters and
the row layout of a 2-D operand."""
from __future__ import annotations

import torch

_counters: dict = {}  # (name, device index) -> int32[1] on that device


def device_counter(name: str, device, op: str) -> torch.Tensor:
    """The int32[1] counter `name` of `device`, zero-filled at its first use.
    That first use must not be inside a stream capture: the counter would
    live in the graph's pool and every replay would zero it again."""
    device = torch.device(device)
    idx = device.index if device.index is not None else torch.cuda.current_device()
    c = _counters.get((name, idx))
    if c is None:
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError(f"{op}: call it once eagerly on this device before capturing "
                               f"(its {name} counter is allocated at the first call)")
        c = _counters[name, idx] = torch.zeros(1, dtype=torch.int32, device=torch.device("cuda", idx))
    return c


def read_counter(name: str, device, op: str, reset: bool) -> int:
    """The counter's value (a device-to-host copy: it synchronises), zeroed
    afterwards with `reset`."""
    c = device_counter(name, "cuda" if device is None else device, op)
    n = int(c.item())
    if reset:
        c.zero_()
    return n


def rows_ld(t: torch.Tensor) -> tuple[torch.Tensor, int]:
    """``(t', ld)``: the 2-D `t` as rows of `ld` elements with dense columns.
    A row-sliced, column-sliced or padded view passes as it is, through its
    leading dimension; anything else is made contiguous.  A single row's
    stride is arbitrary, so its ld is the row's width."""
    if (t.size(1) > 1 and t.stride(1) != 1) or (t.size(0) > 1 and t.stride(0) < t.size(1)):
        t = t.contiguous()
    return t, (t.stride(0) if t.size(0) > 1 else t.size(1))
