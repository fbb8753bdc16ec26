"""ForceUnet and the airfoil design objective on MI355X.

``ForceUnet`` keeps the reference's constructor and state-dict surface (model/diffusion_2d.py:411-486) so its
checkpoints load strictly; ``ForceObjective`` is the ``design_fn`` of inference/inverse_design_2d.py:208-214 -- the
gradient of (summed lift / drag surrogate forces + lambda * boundary overlap) with respect to the diffusion state --
evaluated by libcindm_hip.so (forward AND input-gradient kernels) instead of ``torch.autograd.grad``.  It plugs into
``GaussianDiffusion.sample(design_fn=..., design_guidance="standard-alpha")`` unchanged: the 2-D convention is that
``design_fn(x)`` returns the gradient tensor (model/diffusion_2d.py:813)."""
import ctypes as C
import math

import torch

from . import _ffi
from ._native import _ExchangeRecovery, _NativeModel
from .unet2d import from_device_layout, to_device_layout


class ForceUnet(_ExchangeRecovery, _NativeModel):
    """Drop-in for ``ForceUnet(dim, dim_mults=(1, 2, 4, 8), channels=4)``.  ``forward(x[N, 4, H, W]) -> [N, 2]``;
    ``input_grad(x, lambda_force)`` returns d(sum lambda |out[:, 0]| + out[:, 1]) / dx as well."""

    def __init__(self, dim, init_dim=None, out_dim=None, dim_mults=(1, 2, 4, 8), channels=3, self_condition=False,
                 resnet_block_groups=8, learned_variance=False, *, image_size=64):
        super().__init__()
        if self_condition or learned_variance or resnet_block_groups != 8 or (init_dim not in (None, dim)):
            raise NotImplementedError("ForceUnet: only the configuration of inference/inverse_design_2d.py:157-161 is built")
        self.channels, self.dim, self.dim_mults, self.image_size = channels, dim, tuple(dim_mults), int(image_size)
        d = _ffi.ForceUnetDesc()
        d.dim, d.n_mults, d.channels, d.image_size = dim, len(self.dim_mults), channels, self.image_size
        for i, m in enumerate(self.dim_mults):
            d.dim_mults[i] = m
        self._create(d)

    _PREFIX = "forceunet"
    _CPU_TEXT = "ForceUnet parameters are on the CPU: move the module to a ROCm device; there is no CPU execution path"
    _WS_PROBE = (1, 0)
    _POLL = "status"
    TIMEOUT_TEXT = "an in-kernel exchange of the surrogate's GroupNorm derivative timed out (foreign load on the device)"
    RERUN_TIMEOUT_TEXT = "an exchange timed out during the exchange-free re-run (internal error)"

    def _param_tensor(self, key, p):
        return p.detach().to(torch.float32).contiguous()

    # True (default): every gradient call reads the handle's exchange flag before its result is handed back -- a stream synchronise
    # and a 4-byte device-to-host copy per call, which serialises a Python-driven guided loop on the host.  False: asynchronous calls
    # (as TemporalUnet1D.forward(check=False)); the caller reads ``cindm_forceunet_status`` / ``poll_status()`` before trusting results.
    check_exchange = True

    def poll_status(self, device=None):
        """Reads and clears the exchange flag (synchronises the current stream): 0 = clean, 1 = an exchange timed out since the last
        read (the gradients computed since then contain NaN)."""
        dev = device if device is not None else next(self.parameters()).device
        with torch.cuda.device(dev):
            return int(_ffi.lib().cindm_forceunet_status(self._h, _ffi.current_stream(dev)))

    def _grad_call(self, call, device):
        """Runs ``call()`` (one library gradient call on the current stream) and hands its result back only after the handle's
        exchange flag has been read: a timed-out exchange (NaN gradients) is re-run once with ``no_exchange`` = 1 -- or raised,
        with ``recover`` = 0.  Skipped under stream capture (a capture cannot synchronise; the chain entry points check)."""
        return self._checked(call, device, self.check_exchange and not torch.cuda.is_current_stream_capturing())

    def _workspace(self, nbytes, device):
        if self._ws is None or self._ws.numel() < nbytes or self._ws.device != device:
            self._ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
        return self._ws

    def _run(self, x, lambda_force=None, dout=None):
        if not x.is_cuda:
            raise _ffi.CindmError("ForceUnet needs a ROCm device tensor; there is no CPU execution path")
        n, c, hh, ww = x.shape
        if c != self.channels or hh != self.image_size or ww != self.image_size:
            raise ValueError(f"expected [N, {self.channels}, {self.image_size}, {self.image_size}], got {tuple(x.shape)}")
        self.sync_weights()
        L = _ffi.lib()
        xd = x.detach().float().permute(0, 2, 3, 1).reshape(n, hh * ww, c).contiguous()
        out = torch.empty((n, 2), dtype=torch.float32, device=x.device)
        with_grad = lambda_force is not None or dout is not None
        ws = self._workspace(L.cindm_forceunet_workspace_bytes(self._h, n, int(with_grad)), x.device)
        with torch.cuda.device(x.device):
            if not with_grad:
                _ffi.check(L.cindm_forceunet_forward(self._h, _ffi.ptr(xd), _ffi.ptr(out), n, _ffi.ptr(ws), ws.numel(),
                                                     _ffi.current_stream(x.device)))
                return out, None
            dx = torch.empty_like(xd)
            if dout is not None:
                do = dout.detach().to(device=x.device, dtype=torch.float32).reshape(n, 2).contiguous()
                self._grad_call(lambda: _ffi.check(L.cindm_forceunet_vjp(self._h, _ffi.ptr(xd), _ffi.ptr(do), _ffi.ptr(out), _ffi.ptr(dx), n,
                                                                       _ffi.ptr(ws), ws.numel(), _ffi.current_stream(x.device))), x.device)
            else:
                self._grad_call(lambda: _ffi.check(L.cindm_forceunet_grad(self._h, _ffi.ptr(xd), float(lambda_force), _ffi.ptr(out), _ffi.ptr(dx), n,
                                                                        _ffi.ptr(ws), ws.numel(), _ffi.current_stream(x.device))), x.device)
        return out, dx.reshape(n, hh, ww, c).permute(0, 3, 1, 2).contiguous()

    def forward(self, x, x_self_cond=None):
        """``[N, channels, H, W] -> [N, 2]`` (lift, drag).  Differentiable with respect to ``x`` under torch.autograd (the
        reference's ``force_fn`` takes ``autograd.grad`` of a function of this output, inverse_design_2d.py:113-117): the
        backward is the library's input-gradient pass (``cindm_forceunet_vjp``; the forward is recomputed there -- the
        kernels keep no state between calls).  Weights are frozen: no parameter gradients exist."""
        if x.requires_grad and torch.is_grad_enabled():
            return _ForceUnetFn.apply(x, self)
        with torch.no_grad():
            return self._run(x)[0]

    @torch.no_grad()
    def input_grad(self, x, lambda_force=1.0):
        """(out [N, 2], d(sum_n lambda_force * |out[n, 0]| + out[n, 1]) / dx [N, C, H, W])."""
        return self._run(x, lambda_force)

    def tap(self, name, images, grad=False):
        """Test hook, option ``taps`` = 1: the block output ``name`` of the last ``forward`` / ``input_grad`` call (or, ``grad``, the
        gradient of that call's objective with respect to it) as [images, C, H, W].  Names as the reference's modules: ``init_conv``,
        ``downs.i.0`` .. ``downs.i.3``, ``mid_block1``, ``mid_attn``, ``mid_block2``."""
        ws = self._ws
        if ws is None:
            raise _ffi.CindmError("tap: no forward / input_grad call has run on this model")
        L, shape = _ffi.lib(), (C.c_int64 * 3)()
        with torch.cuda.device(ws.device):
            args = (self._h, name.encode(), int(bool(grad)), images, _ffi.ptr(ws))
            _ffi.check(L.cindm_forceunet_tap(*args, None, 0, C.byref(shape), _ffi.current_stream(ws.device)))
            n, hw, c = shape[0], shape[1], shape[2]
            dst = torch.empty(n * hw * c, dtype=torch.float32, device=ws.device)
            _ffi.check(L.cindm_forceunet_tap(*args, _ffi.ptr(dst), dst.numel(), C.byref(shape), _ffi.current_stream(ws.device)))
        s = int(round(math.sqrt(hw)))
        return dst.view(n, s, s, c).permute(0, 3, 1, 2).contiguous()


class _ForceUnetFn(torch.autograd.Function):
    """ForceUnet.forward under autograd: input gradients only (frozen weights), computed by the HIP backward pass."""

    @staticmethod
    def forward(ctx, x, model):
        ctx.model = model
        ctx.save_for_backward(x)
        return model._run(x)[0]

    @staticmethod
    def backward(ctx, dout):
        (x,) = ctx.saved_tensors
        with torch.no_grad():
            _, dx = ctx.model._run(x, dout=dout)
        return dx.to(x.dtype), None


class ForceObjective:
    """``design_fn`` of the airfoil inverse design (inference/inverse_design_2d.py:208-214; ``sum_boundary`` as force_fn's):
    ``g = grad_force + lambda_overlap * grad_overlap`` for a state ``x [B * nb, 3 * frames + 3, 64, 64]``."""

    def __init__(self, force_model, batch_size, num_boundaries, frames, p_min, p_max, lambda_force=1.0, lambda_overlap=1.0,
                 downsampling_factor=4, frames_per_pass=None, sum_boundary=True):
        self.model, self.B, self.nb, self.frames = force_model, int(batch_size), int(num_boundaries), int(frames)
        # all frames of a design as ONE surrogate batch by default (frames * B * nb images per pass; workspace scales with it)
        self.frames_per_pass = int(frames_per_pass or frames)
        if self.frames % self.frames_per_pass:
            raise ValueError("frames_per_pass must divide frames")
        self.p_min, self.p_max = float(p_min), float(p_max)
        self.lambda_force, self.lambda_overlap, self.factor = float(lambda_force), float(lambda_overlap), int(downsampling_factor)
        self.sum_boundary = bool(sum_boundary)          # force_fn's branch (:98-132); the script's default is True
        self._ws = None

    @torch.no_grad()
    def __call__(self, x):
        if not x.is_cuda:
            raise _ffi.CindmError("ForceObjective needs a ROCm device tensor; there is no CPU execution path")
        n, c, hh, ww = x.shape
        if n != self.B * self.nb or c != 3 * self.frames + 3:
            raise ValueError(f"expected [{self.B * self.nb}, {3 * self.frames + 3}, H, W], got {tuple(x.shape)}")
        m = self.model
        m.sync_weights()
        L = _ffi.lib()
        cp = (c + 3) // 4 * 4
        xd = to_device_layout(x.detach().float(), cp)
        g = torch.empty_like(xd)
        nbytes = L.cindm_airfoil_design_workspace_bytes(m._h, self.B, self.nb, self.frames_per_pass)
        if self._ws is None or self._ws.numel() < nbytes or self._ws.device != x.device:
            self._ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
        with torch.cuda.device(x.device):
            m._grad_call(lambda: _ffi.check(L.cindm_airfoil_design_grad(m._h, _ffi.ptr(xd), self.B, self.nb, self.frames, cp, self.p_min, self.p_max,
                                                                      self.lambda_force, self.lambda_overlap, self.factor, int(self.sum_boundary),
                                                                      _ffi.ptr(g), _ffi.ptr(self._ws), self._ws.numel(),
                                                                      _ffi.current_stream(x.device))), x.device)
        return from_device_layout(g, c, hh, ww)
