"""What GaussianDiffusion1D and GaussianDiffusion share besides the schedule tables: the library's diffusion handle
(``cindm_ddpm1d_*``, one for both paths), built from the 13 registered buffers."""
import ctypes as C

import torch

from . import _ffi
from .schedule import check_solver, ddim_schedule, multistep_kappa


class DiffusionHandle:
    """Mixin of the two diffusion modules.  The class registers the buffers named in ``_ffi.SCHED_NAMES`` and sets
    ``num_timesteps``, ``sampling_timesteps``, ``ddim_sampling_eta`` and ``_h = _tab_sig = None``."""

    @staticmethod
    def _check_model_timesteps(model, timesteps):
        # the model's time path is a table with model.timesteps rows (the reference evaluates its time MLP per call)
        mt = getattr(model, "timesteps", None)
        if mt is not None and int(mt) < int(timesteps):
            raise ValueError(f"model was built with timesteps={mt} < diffusion timesteps={timesteps}: pass timesteps={timesteps} to the model")

    def __del__(self):
        h = self.__dict__.get("_h")
        if h is not None and h.value:
            try:
                _ffi.lib().cindm_ddpm1d_destroy(h)
            except Exception:
                pass
            self.__dict__["_h"] = None

    def _handle(self):
        sig = tuple((getattr(self, n).data_ptr(), getattr(self, n)._version) for n in _ffi.SCHED_NAMES)
        if self._h is not None and sig == self._tab_sig:
            return self._h
        L = _ffi.lib()
        if self._h is not None:
            L.cindm_ddpm1d_destroy(self._h)
        dev = self.betas.device
        if dev.type != "cuda":
            raise _ffi.CindmError(f"{type(self).__name__} is on the CPU: move it to a ROCm device (.to('cuda')); "
                                  "there is no CPU execution path")
        d = _ffi.SchedDesc()
        d.timesteps = self.num_timesteps
        keep = []
        for n in _ffi.SCHED_NAMES:
            t = getattr(self, n).detach().to("cpu", torch.float32).contiguous()
            keep.append(t)
            setattr(d, n, t.data_ptr())
        h = C.c_void_p()
        with torch.cuda.device(dev):
            _ffi.check(L.cindm_ddpm1d_create(C.byref(d), C.byref(h)))
        self._h, self._tab_sig = h, sig
        return h

    @staticmethod
    def _t_int(t):
        return int(t.reshape(-1)[0]) if torch.is_tensor(t) else int(t)

    def ddim_schedule(self):
        """(times [S+1] descending to -1, coefs [S,3] = (sqrt(alpha_next), c, sigma)) of ddim_sample (model/diffusion_1d.py:1743-1777,
        the same recurrence in model/diffusion_2d.py), in the reference's fp32 tensor arithmetic (schedule.ddim_schedule)."""
        return ddim_schedule(self)

    def multistep_kappa(self):
        """fp32 [S]: the per-step factor of ``solver="dpmpp-2m"`` on the ``ddim_schedule()`` grid (schedule.multistep_kappa)."""
        return multistep_kappa(self)

    def _check_solver(self, solver, step_range, history):
        """What a DDIM call refuses of ``solver=`` / ``history=``, before any device work (schedule.check_solver, and the segment
        form's history: X of step i0 - 1, required when i0 > 0, refused otherwise).  True for the multistep solver."""
        on = check_solver(self, solver)
        i0 = 0 if step_range is None else int(step_range[0])
        if history is not None and not on:
            raise ValueError("history= belongs to solver='dpmpp-2m'")
        if on and i0 > 0 and history is None:
            raise ValueError(f"solver='dpmpp-2m' from step {i0}: pass history= (the x_start of step {i0 - 1}, as a segment call returns it)")
        if on and i0 == 0 and history is not None:
            raise ValueError("history= with a chain that starts at step 0: the first step has no previous x_start")
        return on

    def _multistep(self, on, i0, i1, history, state, pack=None):
        """The multistep solver of a DDIM call over steps i0 .. i1-1 (``on``: _check_solver's answer), or None: (kappa fp32
        [i1 - i0] on the host, the history buffer shaped like ``state``, the caller's history in that shape or None; ``pack``
        brings it into the state's layout).  Without a history the buffer is left uninitialised: kappa[0] == 0 does not read it."""
        if not on:
            return None
        kappa = multistep_kappa(self)[i0:i1].clone()
        hist0 = None
        if history is not None:
            hist0 = (pack(history) if pack is not None else history).to(state.device, torch.float32).contiguous()
            if tuple(hist0.shape) != tuple(state.shape):
                raise ValueError(f"history has shape {tuple(history.shape)}: it must be shaped like the state")
        return kappa.contiguous(), torch.empty_like(state), hist0

    @staticmethod
    def _arm_multistep(ms, h):
        """First thing a DDIM chain's call does after the recorder: the chain call consumes the solver, so every issue arms it
        again -- and puts the caller's history back, which the previous issue has overwritten."""
        if ms is None:
            return
        kappa, hist, hist0 = ms
        if hist0 is not None:
            hist.copy_(hist0)
        _ffi.check(_ffi.lib().cindm_ddpm1d_set_multistep(h, C.c_void_p(kappa.data_ptr()), kappa.numel(), _ffi.ptr(hist), hist.numel()))
