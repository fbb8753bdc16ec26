"""What GaussianDiffusion1D and GaussianDiffusion share besides the schedule tables: the library's diffusion handle
(``cindm_ddpm1d_*``, one for both paths), built from the 13 registered buffers."""
import ctypes as C

import torch

from . import _ffi
from .schedule import ddim_schedule


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
