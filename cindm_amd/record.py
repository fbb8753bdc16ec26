"""``return_trajectory_every=``: every k-th state of a sampling chain.

A chain runs n steps, i = 0 .. n-1 in execution order (DDPM: n = t_start - t_end + 1, DDIM: n = n_steps; a guided step with
relaxation iterations is one step).  With ``every = k`` the state after step i is recorded iff (i + 1) % k == 0 or i == n - 1:
ceil(n / k) records, the last one is the result the call returns.  Two streams: ``x`` (the state the step leaves behind) and ``x0``
(the x_start that step predicted, clamped as its update used it).

The library chains record inside the captured step (``cindm_ddpm1d_set_recorder``: one more kernel per step copies the state into a
caller tensor allocated before the chain); the routes that loop in Python clone per step with the same indexing, so what a caller
gets does not depend on which route its ``design_fn`` selects.
"""
import ctypes as C

import torch

from . import _ffi

STREAM_BITS = {"x": 1, "x0": 2}


def record_schedule(n, every):
    """The 1-based step counts after which a chain of ``n`` steps records with ``every``: the multiples of ``every`` up to n,
    and n itself."""
    n, every = int(n), int(every)
    if n < 1:
        raise ValueError(f"a chain has at least one step, got n = {n}")
    if every < 1:
        raise ValueError(f"return_trajectory_every must be >= 1, got {every}")
    steps = list(range(every, n + 1, every))
    if not steps or steps[-1] != n:
        steps.append(n)
    return steps


def record_times(steps, *, t_start=None, times=None):
    """The timestep of every recorded step: ``t_start - i`` for a DDPM chain, ``times[i]`` for a DDIM chain (i = step - 1)."""
    if (t_start is None) == (times is None):
        raise ValueError("give t_start (DDPM) or times (DDIM)")
    if times is not None:
        return [int(times[s - 1]) for s in steps]
    return [int(t_start) - (s - 1) for s in steps]


def stream_mask(trajectory):
    names = (trajectory,) if isinstance(trajectory, str) else tuple(trajectory)
    if not names:
        raise ValueError("trajectory must name at least one stream ('x', 'x0')")
    mask = 0
    for nm in names:
        if nm not in STREAM_BITS:
            raise ValueError(f"unknown trajectory stream {nm!r} (one of 'x', 'x0')")
        mask |= STREAM_BITS[nm]
    return mask


class ChainRecord:
    """What ``return_trajectory_every=`` hands back next to the designs: ``step`` (1-based step counts), ``t`` (their timesteps),
    ``x`` [n_records, *design shape] or None, ``x0`` likewise."""

    def __init__(self, step, t, x, x0):
        self.step, self.t, self.x, self.x0 = list(step), list(t), x, x0

    def __len__(self):
        return len(self.step)

    def __repr__(self):
        shape = None if self.x is None else tuple(self.x.shape)
        return f"ChainRecord(step={self.step}, t={self.t}, x={shape}, x0={'None' if self.x0 is None else tuple(self.x0.shape)})"


class DeviceRecorder:
    """The record buffer of one library chain: allocated before the chain, armed on the schedule handle right before every issue of
    the chain call (the call consumes it), unpacked after it.  Layout (include/cindm_hip.h): [records][streams][floats per record]
    in the library's state layout, then one staging record when ``x0`` is on."""

    def __init__(self, n, every, trajectory, floats_per_record, device, *, t_start=None, times=None):
        self.mask = stream_mask(trajectory)
        self.steps = record_schedule(n, every)
        self.t = record_times(self.steps, t_start=t_start, times=times)
        self.n, self.every, self.fpr = int(n), int(every), int(floats_per_record)
        self.ns = bin(self.mask).count("1")
        total = (len(self.steps) * self.ns + (1 if self.mask & 2 else 0)) * self.fpr
        self.buf = torch.empty(total, dtype=torch.float32, device=device)

    def arm(self, h):
        _ffi.check(_ffi.lib().cindm_ddpm1d_set_recorder(h, _ffi.ptr(self.buf), self.buf.numel(), self.every, self.mask))

    def collect(self, h, unpack):
        """``unpack``: [n_records * anything, floats per record] rows in the library's layout -> the caller's layout per row."""
        info = (C.c_int32 * 4)()
        _ffi.check(_ffi.lib().cindm_ddpm1d_recorder_info(h, info))
        if (info[0], info[1], info[2], info[3]) != (len(self.steps), self.fpr, self.n, self.mask):
            raise _ffi.CindmError(f"the chain recorded {tuple(info)} (records, floats per record, steps, streams), expected "
                                  f"{(len(self.steps), self.fpr, self.n, self.mask)}")
        rows = self.buf[:len(self.steps) * self.ns * self.fpr].view(len(self.steps), self.ns, self.fpr)
        x = unpack(rows[:, 0]) if self.mask & 1 else None
        x0 = unpack(rows[:, self.ns - 1]) if self.mask & 2 else None
        return ChainRecord(self.steps, self.t, x, x0)


class LoopRecorder:
    """The same record for the routes that loop in Python: ``after(i, x, x0)`` after step i clones what the schedule asks for."""

    def __init__(self, n, every, trajectory, *, t_start=None, times=None):
        self.mask = stream_mask(trajectory)
        self.steps = record_schedule(n, every)
        self.t = record_times(self.steps, t_start=t_start, times=times)
        self.reset()

    def reset(self):
        self._x, self._x0, self._k = [], [], 0

    def after(self, i, x, x0=None):
        if self._k == len(self.steps) or self.steps[self._k] != i + 1:
            return
        self._k += 1
        if self.mask & 1:
            self._x.append(x.detach().clone())
        if self.mask & 2:
            if x0 is None:
                raise NotImplementedError("this route has no x0 to record")
            self._x0.append(x0.detach().clone())

    def result(self, shape=None):
        f = lambda lst: None if not lst else (torch.stack(lst) if shape is None else torch.stack(lst).reshape((len(lst),) + tuple(shape)))
        return ChainRecord(self.steps, self.t, f(self._x), f(self._x0))
