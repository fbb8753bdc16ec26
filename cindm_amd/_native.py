"""What the three native model classes (``TemporalUnet1D``, ``Unet``, ``ForceUnet``) share: the library handle, the parameters
under the reference's state-dict names, the weight synchronisation, the kernel-path options and the workspace cache
(``_NativeModel``), and the recovery from a timed-out in-kernel exchange (``_ExchangeRecovery``).

The handle's C entry points are ``cindm_<prefix>_*`` (include/cindm_hip.h).  Which options keep the packed weights valid is
known to the library alone: ``set_option`` only marks the model "needs sync", and ``sync_weights`` finalizes the handle when
the handle reports that it is not finalized (``*_workspace_bytes`` answers 0 then)."""
import ctypes as C
import math

import torch
from torch import nn

from . import _ffi


class _Node(nn.Module):
    """Anonymous container used to rebuild the reference's dotted key hierarchy."""


def _attach(root, dotted, param):
    parts = dotted.split(".")
    mod = root
    for p in parts[:-1]:
        if p not in mod._modules:
            mod.add_module(p, _Node())
        mod = mod._modules[p]
    mod.register_parameter(parts[-1], param)


class _NativeModel(nn.Module):
    """Base of the model classes.  A subclass sets ``_PREFIX`` (the C prefix), ``_CPU_TEXT`` (the error for parameters that
    are not on a ROCm device) and ``_WS_PROBE`` (arguments of ``*_workspace_bytes`` after the handle that ask for the smallest
    workspace); it calls ``_create`` with its descriptor and may override ``_fill`` (initial value of a parameter),
    ``_sinusoid_table`` and ``_param_tensor``."""
    _PREFIX = None
    _CPU_TEXT = None
    _WS_PROBE = (1,)

    def _c(self, name):
        return getattr(_ffi.lib(), f"cindm_{self._PREFIX}_{name}")

    def _create(self, desc):
        """Creates the handle and registers the parameters of its manifest, PyTorch-default initialisation."""
        h = C.c_void_p()
        _ffi.check(self._c("create")(C.byref(desc), C.byref(h)))
        self._h = h
        self._sig = None                 # parameter signature of the last upload
        self._dirty = True               # an option changed since the last sync_weights
        self._range_checked = False      # the range guard has checked a result of the current pack (TemporalUnet1D)
        self._py_recovered = 0           # exchange-free re-runs driven from Python (_ExchangeRecovery)
        self._ws = None
        name = C.create_string_buffer(256)
        shape = (C.c_int64 * 4)()
        nd = C.c_int()
        manifest = []
        for i in range(self._c("num_params")(h)):
            _ffi.check(self._c("param_info")(h, i, name, 256, C.byref(shape), C.byref(nd)))
            manifest.append((name.value.decode(), tuple(int(shape[j]) for j in range(nd.value))))
        fan = {k[:-7]: math.prod(s[1:]) for k, s in manifest if k.endswith(".weight") and len(s) >= 2}
        for k, s in manifest:
            t = torch.empty(s)
            v = self._fill(k)
            if v is not None:
                t.fill_(v)
            else:
                bound = 1.0 / math.sqrt(fan[k.rsplit(".", 1)[0]])
                t.uniform_(-bound, bound)
            _attach(self, k, nn.Parameter(t))
        self._manifest = manifest

    @staticmethod
    def _fill(key):
        """Constant initial value of a parameter (GroupNorm / LayerNorm gains 1, biases 0); None: uniform in +-1/sqrt(fan_in)."""
        if key.endswith(".g") or key.endswith(".norm.weight"):
            return 1.0
        if key.endswith(".norm.bias"):
            return 0.0
        return None

    def _sinusoid_table(self):
        return None

    def _param_tensor(self, key, p):
        if p.dtype != torch.float32:
            raise TypeError(f"{key}: fp32 parameters required, got {p.dtype}")
        return p.detach().contiguous()

    def __del__(self):
        h = self.__dict__.get("_h")
        if h is not None and h.value:
            try:
                self._c("destroy")(h)
            except Exception:
                pass
            self.__dict__["_h"] = None

    # ------------------------------------------------------------------ weights -> library
    def _signature(self):
        return tuple((p.data_ptr(), p._version) for p in self.parameters())

    def _finalized(self):
        return self._c("workspace_bytes")(self._h, *self._WS_PROBE) != 0

    def sync_weights(self, force=False):
        """Copies the parameter values into the library handle when they changed (or ``force``), and re-runs the handle's
        finalisation (weight repack, per-timestep tables, range rule) when the handle needs it."""
        sig = self._signature()
        if not force and not self._dirty and sig == self._sig:
            return
        upload = force or sig != self._sig
        dev = None
        for k, p in self.named_parameters():
            if p.is_cuda:
                dev = p.device
            if upload:
                t = self._param_tensor(k, p)
                _ffi.check(self._c("set_param")(self._h, k.encode(), _ffi.ptr(t), t.numel(), int(t.is_cuda)))
        if dev is None:
            raise _ffi.CindmError(self._CPU_TEXT)
        tab = self._sinusoid_table() if upload else None
        if tab is not None:
            _ffi.check(self._c("set_sinusoid_table")(self._h, _ffi.ptr(tab), tab.numel()))
        if not self._finalized():
            with torch.cuda.device(dev):
                _ffi.check(self._c("finalize")(self._h, _ffi.current_stream(dev)))
            self._range_checked = False
            self._ws = None
        self._sig, self._dirty = sig, False

    def _option(self, key):
        v = C.c_int32()
        _ffi.check(self._c("get_option")(self._h, key.encode(), C.byref(v)))
        return int(v.value)

    def set_option(self, key, value):
        """Selects a kernel path of this model (``cindm_<model>_set_option``; keys in include/cindm_hip.h).  Every path computes
        the same function; takes effect at the next call."""
        _ffi.check(self._c("set_option")(self._h, key.encode(), int(value)))
        self._dirty = True
        self._ws = None
        return self

    def get_option(self, key):
        """Current value of a kernel-path option after the weights were synchronised; ``get_option("range_fallback")`` is
        non-zero when the range rule selected the exact fp32 kernels."""
        self.sync_weights()
        return self._option(key)

    def workspace(self, n, device):
        """The cached workspace for ``n`` rows / images (reallocated when it holds fewer bytes than ``n`` needs, or on another device)."""
        need = self._c("workspace_bytes")(self._h, n)      # not monotonic in n: fewer rows can select a plan with larger staging
        if self._ws is None or self._ws.numel() < need or self._ws.device != device:
            self._ws = torch.empty(need, dtype=torch.uint8, device=device)
        return self._ws


class _ExchangeRecovery:
    """Recovery from a timed-out in-kernel exchange between workgroups (foreign load on the device kept a partner workgroup from
    becoming resident): the work is re-run once on the exchange-free kernels (run-time option ``no_exchange``), or the time-out
    is raised when the handle's run-time option ``recover`` is 0.  A subclass sets ``_POLL`` (the C entry point that reads and
    clears the handle's exchange flag), ``TIMEOUT_TEXT`` and ``RERUN_TIMEOUT_TEXT``."""
    _POLL = None

    @property
    def recover_exchange_timeouts(self):
        return bool(self._option("recover"))

    @recover_exchange_timeouts.setter
    def recover_exchange_timeouts(self, on):
        """The handle's run-time option ``recover``: also its chain entry points (sample / ddim_sample / the built-in guided loops)
        return an error instead of re-running a timed-out chain."""
        _ffi.check(self._c("set_option")(self._h, b"recover", int(bool(on))))

    def poll_raw(self, device):
        """True when an exchange of the work issued so far timed out (the flag is cleared); synchronises; never raises for a
        time-out."""
        with torch.cuda.device(device):
            rc = self._c(self._POLL)(self._h, _ffi.current_stream(device))
        if rc < 0:
            _ffi.check(rc)
        return rc == 1

    def exchange_free(self, on):
        """Run-time switch (option ``no_exchange``; does not touch the packed weights or the workspace): only kernels without an
        in-launch exchange between workgroups."""
        _ffi.check(self._c("set_option")(self._h, b"no_exchange", int(bool(on))))

    def rerun_exchange_free(self, fn, device):
        """``fn()`` once more with this model on the exchange-free kernels (after a time-out); a second time-out cannot happen
        there and raises."""
        self.exchange_free(True)
        try:
            out = fn()
            if self.poll_raw(device):
                raise _ffi.CindmError(self.RERUN_TIMEOUT_TEXT)
        finally:
            self.exchange_free(False)
        self.note_recovered()
        return out

    def _checked(self, call, device, check=True):
        """``call()``, handed back only after the exchange flag was read (``check``): a time-out re-runs ``call`` exchange-free,
        or raises with ``recover`` = 0."""
        out = call()
        if check and self.poll_raw(device):
            if not self.recover_exchange_timeouts:
                raise _ffi.CindmError(self.TIMEOUT_TEXT)
            out = self.rerun_exchange_free(call, device)
        return out

    def note_recovered(self):
        """Counts one exchange-free re-run driven from Python (GaussianDiffusion1D's steps re-run their models together)."""
        self._py_recovered += 1

    @property
    def recovered(self):
        """Calls / chains of this model that were re-run on the exchange-free kernels after a time-out; 0 in normal operation."""
        return int(self._c("recovered")(self._h)) + self._py_recovered
