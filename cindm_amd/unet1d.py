"""TemporalUnet1D on MI355X: the reference's constructor / state_dict / forward surface
(model/diffusion_1d.py:517-646 of AI4Science-WestlakeU/cindm) over the HIP library.

The module owns ordinary ``nn.Parameter`` tensors under the reference's state-dict key names
(SURVEY.md Appendix A.3), so reference checkpoints load with ``load_state_dict(strict=True)``
and ``.to(device)`` / ``.eval()`` / ``.parameters()`` behave as callers expect.  ``forward``
hands raw device pointers to ``libcindm_hip.so``; there is no PyTorch compute path.
"""
import ctypes as C
import math

import torch

from . import _ffi
from ._native import _ExchangeRecovery, _NativeModel


def sinusoid_table(timesteps, dim):
    """Row t = SinusoidalPosEmb(dim)(t) (model/diffusion_1d.py:151-158): fp32 frequencies
    ``exp(arange(half) * -(ln 1e4 / (half-1)))``, fp32 product with the integer timestep, fp32
    sin/cos -- evaluated once on the host for t = 0..timesteps-1."""
    half = dim // 2
    emb = math.log(10000) / (half - 1)
    freq = torch.exp(torch.arange(half) * -emb)
    arg = torch.arange(timesteps)[:, None] * freq[None, :]
    return torch.cat((arg.sin(), arg.cos()), dim=-1).contiguous()


class TemporalUnet1D(_ExchangeRecovery, _NativeModel):
    """Drop-in for ``TemporalUnet1D(horizon, transition_dim, cond_dim, dim=64,
    dim_mults=(1, 2, 4, 8), attention=False)`` (model/diffusion_1d.py:519-527).

    ``dim``: a power of two >= 32, or 96 (the reference's ``--Unet_dim 96`` checkpoint); ``dim_mults``: powers of
    two.  dim 64 runs the fused level / deep-block / attention-site kernels; every other width, 96 included, runs
    the generic convolution and attention kernels (more launches per forward, the same results contract).

    Extra keyword ``timesteps`` (default 1000) sizes the per-timestep bias table that replaces
    the time-embedding MLP at run time."""

    def __init__(self, horizon, transition_dim, cond_dim, dim=64, dim_mults=(1, 2, 4, 8), attention=False,
                 *, timesteps=1000):
        super().__init__()
        self.horizon = horizon
        self.transition_dim = transition_dim
        self.channels = transition_dim
        self.cond_dim = cond_dim
        self.dim = dim
        self.dim_mults = tuple(dim_mults)
        self.attention = bool(attention)
        self.timesteps = int(timesteps)
        d = _ffi.UnetDesc()
        d.horizon, d.transition_dim, d.dim, d.n_mults = horizon, transition_dim, dim, len(self.dim_mults)
        for i, m in enumerate(self.dim_mults):
            d.dim_mults[i] = m
        d.attention, d.timesteps = int(self.attention), self.timesteps
        self._create(d)

    _PREFIX = "unet1d"
    _CPU_TEXT = ("TemporalUnet1D parameters are on the CPU: move the module to a ROCm device (.to('cuda')); "
                 "there is no CPU execution path")

    @staticmethod
    def _fill(key):
        if key.endswith(".norm.g") or (".block.2." in key and key.endswith(".weight")):
            return 1.0
        return 0.0 if ".block.2." in key else None

    def _sinusoid_table(self):
        return sinusoid_table(self.timesteps, self.dim)

    @property
    def launches_per_forward(self):
        return _ffi.lib().cindm_unet1d_launches_per_forward(self._h)

    # ------------------------------------------------------------------ forward
    @torch.no_grad()
    def forward(self, x, time, cond=None, *, check=None):
        """x [B, horizon, transition_dim] fp32 on a ROCm device, time [B] (all equal) -> eps [B, horizon, F]
        (model/diffusion_1d.py:610-646).  ``cond`` is ignored, as in the reference.

        ``check`` (build-only keyword): read the handle's exchange flag before returning -- a device-to-host copy and a
        stream synchronise -- and recover from a timed-out exchange (``recover_exchange_timeouts``).  Default: on, except
        while the current stream is being captured (a synchronise would invalidate the capture).  Callers that pass
        ``check=False`` (asynchronous pipelines, graph captures) must call ``check_status()`` / ``poll_status()`` themselves
        before they trust the results."""
        if not x.is_cuda:
            raise _ffi.CindmError("TemporalUnet1D.forward needs a ROCm device tensor; there is no CPU execution path")
        if x.dim() != 3 or x.shape[1] != self.horizon or x.shape[2] != self.transition_dim:
            raise ValueError(f"expected x of shape [B, {self.horizon}, {self.transition_dim}], got {tuple(x.shape)}")
        if torch.is_tensor(time):
            lo, hi = torch.aminmax(time)
            lo, hi = int(lo), int(hi)
            if lo != hi:
                raise NotImplementedError("per-row timesteps are not supported on the sampling path (all rows share t)")
            t = lo
        else:
            t = int(time)
        self.sync_weights()
        x = x.contiguous().float()
        out = torch.empty_like(x)
        if check is None:
            check = not torch.cuda.is_current_stream_capturing()

        def launch():
            ws = self.workspace(x.shape[0], x.device)          # (inside: a range escalation re-runs on a plan of its own size)
            with torch.cuda.device(x.device):
                _ffi.check(_ffi.lib().cindm_unet1d_forward(self._h, _ffi.ptr(x), t, None, _ffi.ptr(out), x.shape[0],
                                                           _ffi.ptr(ws), ws.numel(), _ffi.current_stream(x.device)))

        self._checked(launch, x.device, check)
        if check and self.range_guard_pending():
            # the range rule on the caller's own data: the FIRST checked forward after a weight synchronisation
            self.range_guard(lambda: out, launch, x.device)
        return out

    # ------------------------------------------------------------------ range rule on the caller's data (round 6)
    def range_guard_pending(self):
        """True until the first result after the last weight synchronisation has been checked -- and only where the check can
        change anything: the handle runs the split-fp16 kernels with ``auto_range`` on.  Every finalize of the handle (new weights,
        a change of an option that selects what is packed) makes it pending again; a run-time option does not."""
        if self._range_checked:
            return False
        return bool(self.get_option("auto_range")) and not self.get_option("mfma_f32") and not self.get_option("range_fallback")

    def range_guard(self, result, rerun, device):
        """``result()`` is what the split-fp16 kernels just produced for the caller's own inputs.  Finite: nothing to do (one
        reduction and one synchronise, once per weight synchronisation).  inf / nan: the un-normalised residual stream of this
        checkpoint left fp16's exponent range on real data although the synthetic calibration batch passed -- the handle is repacked
        for the exact fp32-MFMA kernels (``get_option("range_fallback")`` reads 3), ``rerun()`` repeats the work; if that is not
        finite either the cause was not the range (non-finite inputs / weights) and the split-fp16 pack is restored.
        Returns True when the handle was escalated."""
        self._range_checked = True
        if bool(torch.isfinite(result()).all()):
            return False
        import warnings
        with torch.cuda.device(device):
            _ffi.check(_ffi.lib().cindm_unet1d_range_escalate(self._h, 1, _ffi.current_stream(device)))
        self._ws = None           # (the fp32 plan has its own workspace size)
        rerun()
        if bool(torch.isfinite(result()).all()):
            warnings.warn("cindm_amd: the first result after loading these weights was not finite on the split-fp16 kernels (an activation left "
                          "fp16's exponent range on the caller's data); the model now runs on the exact fp32-MFMA kernels, about 3x slower "
                          "(get_option('range_fallback') == 3)", RuntimeWarning)
            return True
        with torch.cuda.device(device):
            _ffi.check(_ffi.lib().cindm_unet1d_range_escalate(self._h, 0, _ffi.current_stream(device)))
        self._ws = None
        return False

    TIMEOUT_TEXT = ("an in-kernel exchange between workgroups timed out (GroupNorm pair / attention head exchange): "
                    "the results of that forward are invalid")
    RERUN_TIMEOUT_TEXT = TIMEOUT_TEXT
    _POLL = "poll"

    def check_status(self, device):
        """Raises CindmError when an in-kernel exchange between workgroups of a forward issued so far timed out (its
        results are invalid); synchronises the current stream."""
        with torch.cuda.device(device):
            _ffi.check(_ffi.lib().cindm_unet1d_status(self._h, _ffi.current_stream(device)))

    def poll_status(self, device):
        """True when an exchange of a forward issued so far timed out (the flag is cleared); synchronises the current
        stream.  With ``recover_exchange_timeouts = False`` a time-out raises CindmError here instead."""
        hit = self.poll_raw(device)
        if hit and not self.recover_exchange_timeouts:
            raise _ffi.CindmError(self.TIMEOUT_TEXT)
        return hit

    # kind 4 = the k=5 convolutions: conv_gemm_h3_kernel<5,48,*> (split-fp16 MFMA; default) or
    # conv_gemm_kernel<5,32,48,*> (fp32 MFMA; CINDM_MFMA=f32)
    KERNEL_KINDS = ("conv_gemm_kernel<0>", "conv_gemm_kernel<1>", "conv_gemm_kernel<3>", "conv_gemm_kernel<4>",
                    "conv5_gemm", "attention_and_level_kernels")

    @torch.no_grad()
    def profile(self, x, t):
        """One forward with every launch bracketed by HIP events on the current stream.
        Returns {kernel kind: (launches, total ms, total algorithmic FLOPs)}."""
        self.sync_weights()
        x = x.contiguous().float()
        out = torch.empty_like(x)
        ws = self.workspace(x.shape[0], x.device)
        cnt, ms, fl = (C.c_int32 * 6)(), (C.c_float * 6)(), (C.c_double * 6)()
        with torch.cuda.device(x.device):
            _ffi.check(_ffi.lib().cindm_unet1d_profile(self._h, _ffi.ptr(x), int(t), _ffi.ptr(out), x.shape[0], _ffi.ptr(ws),
                                                       ws.numel(), _ffi.current_stream(x.device), C.byref(cnt), C.byref(ms),
                                                       C.byref(fl)))
        return {k: (cnt[i], ms[i], fl[i]) for i, k in enumerate(self.KERNEL_KINDS)}

    @torch.no_grad()
    def profile_detail(self, x, t, cap=256):
        """Per-launch records of one instrumented forward: [(kind, ms, flops, grid_x, grid_y, stages)]."""
        self.sync_weights()
        x = x.contiguous().float()
        out = torch.empty_like(x)
        ws = self.workspace(x.shape[0], x.device)
        n = C.c_int32()
        kind, ms, fl, g = (C.c_int32 * cap)(), (C.c_float * cap)(), (C.c_double * cap)(), (C.c_int32 * (3 * cap))()
        with torch.cuda.device(x.device):
            _ffi.check(_ffi.lib().cindm_unet1d_profile_detail(self._h, _ffi.ptr(x), int(t), _ffi.ptr(out), x.shape[0], _ffi.ptr(ws),
                                                              ws.numel(), _ffi.current_stream(x.device), cap, C.byref(n), kind, ms, fl, g))
        return [(self.KERNEL_KINDS[kind[i]], ms[i], fl[i], g[3 * i], g[3 * i + 1], g[3 * i + 2]) for i in range(n.value)]

    def tap(self, name, rows):
        """Intermediate activation of the last forward as [rows, C, L] (the reference's layout)."""
        shape = (C.c_int64 * 3)()
        ws = self._ws
        dst = torch.empty(rows * 1536 * 8, dtype=torch.float32, device=ws.device)
        with torch.cuda.device(ws.device):
            _ffi.check(_ffi.lib().cindm_unet1d_tap(self._h, name.encode(), rows, _ffi.ptr(ws), _ffi.ptr(dst),
                                                   dst.numel(), C.byref(shape), _ffi.current_stream(ws.device)))
        n = shape[0] * shape[1] * shape[2]
        return dst[:n].view(shape[0], shape[1], shape[2]).transpose(1, 2).contiguous()
