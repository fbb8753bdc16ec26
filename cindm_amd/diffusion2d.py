"""GaussianDiffusion (2-D airfoil design, sampling half) on MI355X: the reference's constructor / buffers /
``sample`` surface (model/diffusion_2d.py:551-963 of AI4Science-WestlakeU/cindm) over the HIP library.

What runs where
  * the Unet on all ``batch * num_boundaries`` images, the boundary sharing of the predicted noise, x0, clamp,
    posterior mean and the (boundary-shared) noise add run in ``libcindm_hip.so``;
  * with ``design_fn=None`` the whole reverse loop is ONE call (``cindm_ddpm2d_sample``: one captured HIP graph
    step replayed per timestep), the state staying in the library's channel-last layout for the whole chain;
  * ``design_fn`` is a user Python callable returning a gradient tensor (:813); it is evaluated between library
    calls, exactly where the reference evaluates it.
  * DDIM (``sampling_timesteps < timesteps``, ``ddim_sample``) without ``design_fn`` is ONE call too
    (``cindm_ddpm2d_sample_ddim``: U-Net + one element-wise DDIM update per captured step, t and the step index
    advanced on the device).  The reference's own 2-D DDIM cannot run; the semantics are defined in ``ddim_sample``.
  * DDIM with ``design_fn=ForceObjective`` under ``"standard-alpha"`` is ONE call as well (``cindm_ddpm2d_sample_ddim_force``:
    surrogate gradient + U-Net + one update that carries the guidance shift, per captured step).
  * Replacement conditioning (``known=`` / ``known_mask=`` / ``cond=`` of the sampling calls): a known region of the state rides
    the forward-diffusion trajectory of its clean values inside the captured step of all four library chains (known2d_kernel,
    ``cindm_ddpm1d_set_known2d``) and comes back exactly; the reference's 2-D sampler takes no condition, the semantics are
    defined in ``p_sample_loop`` / ``ddim_sample``.
Training, self-conditioning, DDIM with any other ``design_fn`` / guidance, DDIM with share_noise=False and
return_all_timesteps are outside this build's scope and raise NotImplementedError.
"""
import ctypes as C
from collections import namedtuple

import torch
from torch import nn

from . import _ffi
from .diffusion_base import DiffusionHandle
from .record import DeviceRecorder, LoopRecorder, stream_mask
from .schedule import check_solver, make_schedule
from .unet2d import from_device_layout, to_device_layout


ModelPrediction = namedtuple("ModelPrediction", ["pred_noise", "pred_x_start"])      # model/diffusion_2d.py:43


class NoiseTape2D:
    """Explicit noise for parity runs, replacing the reference's ``sample_noise`` draws (:775-785):
    ``init`` = (state [B,1,C-3,H,W], boundary [B,nb,3,H,W]) for x_T (:895);
    ``step_state`` [T,B,1,C-3,H,W] / ``step_boundary`` [T,B,nb,3,H,W] indexed by timestep (:807).
    ``known_init`` / ``known_state`` / ``known_boundary`` (all three or none): the draws of the known region's forward
    diffusion (``known=`` / ``cond=`` of the sampling calls), shaped and indexed like ``init`` and the step rows -- by t for
    DDPM, by the DDIM step index for DDIM."""

    def __init__(self, init, step_state, step_boundary, known_init=None, known_state=None, known_boundary=None):
        self.init, self.step_state, self.step_boundary = init, step_state, step_boundary
        self.known_init, self.known_state, self.known_boundary = known_init, known_state, known_boundary


# the seed word of the known region's counter-based draws (known2d_kernel's kKnown2dSeed): distinct from the step draws'
KNOWN_SEED = 0x6b6e6f776e326421


def _state_cl(s):
    """[..., B, 1, Cs, H, W] -> channel-last [..., B, H*W, Cs]"""
    *lead, b, one, cs, h, w = s.shape
    return s.reshape(*lead, b, cs, h * w).transpose(-1, -2).contiguous()


def _boundary_cl(s):
    """[..., B, nb, 3, H, W] -> channel-last [..., B*nb, H*W, 3]"""
    *lead, b, nb, c, h, w = s.shape
    return s.reshape(*lead, b * nb, c, h * w).transpose(-1, -2).contiguous()


class GaussianDiffusion(DiffusionHandle, nn.Module):
    """Drop-in for the reference's 2-D ``GaussianDiffusion`` (constructor :552-676)."""

    def __init__(self, model, *, image_size, frames=6, cond_frames=4, timesteps=1000, sampling_timesteps=None,
                 loss_type="l1", objective="pred_noise", beta_schedule="sigmoid", schedule_fn_kwargs=dict(),
                 ddim_sampling_eta=0., auto_normalize=True, min_snr_loss_weight=False, min_snr_gamma=5,
                 diffuse_cond=True, backward_steps=5, backward_lr=0.01, standard_fixed_ratio=0.01,
                 forward_fixed_ratio=0.01, coeff_ratio=0.1, share_noise=True, use_average_share=True):
        super().__init__()
        assert model.channels == model.out_dim
        assert not model.random_or_learned_sinusoidal_cond
        if objective not in _ffi.OBJECTIVES:
            raise ValueError("objective must be either pred_noise (predict noise) or pred_x0 (predict image start) or pred_v (predict v)")
        if schedule_fn_kwargs or min_snr_loss_weight:
            raise NotImplementedError("schedule_fn_kwargs / min_snr_loss_weight only matter for training")
        self.model = model
        self.channels = model.channels
        self.self_condition = False
        self.frames, self.cond_frames = frames, cond_frames
        self.image_size = image_size
        self.objective = objective
        self.diffuse_cond = diffuse_cond
        self.backward_steps, self.backward_lr = backward_steps, backward_lr
        self.standard_fixed_ratio, self.forward_fixed_ratio = standard_fixed_ratio, forward_fixed_ratio
        self.coeff_ratio = coeff_ratio
        self.share_noise, self.use_average_share = share_noise, use_average_share
        assert self.channels == frames * 3 + 3, "channels must be frames * 3 + 3 (states + boundary mask/offsets)"
        assert image_size == model.image_size, "image_size must match the Unet's launch plan"
        tables = make_schedule(beta_schedule, timesteps, objective)
        self.num_timesteps = int(timesteps)
        self._check_model_timesteps(model, timesteps)
        self.loss_type = loss_type
        self.sampling_timesteps = sampling_timesteps if sampling_timesteps is not None else timesteps
        assert self.sampling_timesteps <= timesteps
        self.is_ddim_sampling = self.sampling_timesteps < timesteps
        self.ddim_sampling_eta = ddim_sampling_eta
        for name in _ffi.SCHED_NAMES:               # same buffer names as the reference (:626-674)
            self.register_buffer(name, tables[name])
        self._h = None
        self._tab_sig = None
        self._ws = None
        self._ddim_tab = None

    def _share_mode(self):
        """The library's ``use_average_share`` word: bit 0 = mean (1) / sum (0) over the boundary copies of a design, bit 1 =
        share_noise False -- the clamped x_start and the posterior mean are shared instead of the prediction (:757-773); bits 4-5 =
        the objective (pred_noise / pred_x0 / pred_v, :743-753)."""
        return int(bool(self.use_average_share)) | (0 if self.share_noise else 2) | (_ffi.OBJECTIVES[self.objective] << 4)

    # ------------------------------------------------------------------ library handle
    def _prepare(self, images, device):
        self.model.sync_weights()
        h = self._handle()
        nbytes = _ffi.lib().cindm_ddpm2d_workspace_bytes(self.model._h, images)
        if self._ws is None or self._ws.numel() < nbytes or self._ws.device != device:
            self._ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
        return h, self._ws

    # ------------------------------------------------------------------ reference-named helpers (plumbing)
    def predict_start_from_noise(self, x_t, t, noise):
        return self.sqrt_recip_alphas_cumprod[t].view(-1, 1, 1, 1) * x_t - self.sqrt_recipm1_alphas_cumprod[t].view(-1, 1, 1, 1) * noise

    def q_posterior(self, x_start, x_t, t):
        mean = self.posterior_mean_coef1[t].view(-1, 1, 1, 1) * x_start + self.posterior_mean_coef2[t].view(-1, 1, 1, 1) * x_t
        return mean, self.posterior_variance[t].view(-1, 1, 1, 1), self.posterior_log_variance_clipped[t].view(-1, 1, 1, 1)

    def q_sample(self, x_start, t, noise=None):
        if noise is None:
            noise = torch.randn_like(x_start)
        return self.sqrt_alphas_cumprod[t].view(-1, 1, 1, 1) * x_start + self.sqrt_one_minus_alphas_cumprod[t].view(-1, 1, 1, 1) * noise

    def share_states_over_boundaries(self, shape, x, use_average_share=True):
        """:712-725 (torch; the library does this inside its update kernel -- this is for callers' own tensors)."""
        s = x[:, :-3].reshape(shape[0], shape[1], shape[2] - 3, shape[3], shape[4])
        s = s.mean(dim=1, keepdim=True) if use_average_share else s.sum(dim=1, keepdim=True)
        x[:, :-3] = s.expand(-1, shape[1], -1, -1, -1).reshape(shape[0] * shape[1], shape[2] - 3, shape[3], shape[4])
        return x

    def sample_noise(self, shape, device):
        """:775-785."""
        state = torch.randn((shape[0], 1, shape[2] - 3, shape[3], shape[4]), device=device)
        boundary = torch.randn((shape[0], shape[1], 3, shape[3], shape[4]), device=device)
        return torch.cat([state.expand(-1, shape[1], -1, -1, -1), boundary], dim=2)

    # ------------------------------------------------------------------ replacement conditioning (known region)
    def _known_region(self, shape, known, known_mask, cond, noise=None, rows=0):
        """The known region of a sampling call as (values [B, nb, C, H, W] fp32, mask bool of that shape), or None.  Host checks
        only (ValueError), made before any device work: shapes, ``cond=`` against ``known=``, the state channels of values and
        mask identical over the boundary copies of a design, and the tape's known rows (``rows`` of them at least)."""
        if known is None and cond is None:
            if known_mask is not None:
                raise ValueError("known_mask without known")
            return None
        B, nb, Cc, H, W = shape
        k = torch.zeros(tuple(shape), dtype=torch.float32, device=(known if known is not None else cond).device)
        m = torch.zeros(tuple(shape), dtype=torch.bool, device=k.device)
        if known is not None:
            if known_mask is None:
                raise ValueError("known needs known_mask (bool, broadcastable to [B, nb, C, H, W])")
            if tuple(known.shape) != tuple(shape):
                raise ValueError(f"known must have the shape of the state {tuple(shape)}, got {tuple(known.shape)}")
            if known_mask.dtype != torch.bool:
                raise ValueError("known_mask must be a bool tensor")
            try:
                m = torch.broadcast_to(known_mask.to(k.device), tuple(shape)).clone()
            except RuntimeError as e:
                raise ValueError(f"known_mask {tuple(known_mask.shape)} does not broadcast to {tuple(shape)}") from e
            if known_mask.dim() > len(shape):
                raise ValueError(f"known_mask {tuple(known_mask.shape)} does not broadcast to {tuple(shape)}")
            k = known.to(torch.float32).clone()
        if cond is not None:
            nc = 3 * self.cond_frames
            if tuple(cond.shape) != (B, nc, H, W):
                raise ValueError(f"cond must be [B, 3 * cond_frames, H, W] = {(B, nc, H, W)}, got {tuple(cond.shape)}")
            if bool(m[:, :, :nc].any()):
                raise ValueError("cond= and known= name the same channels (the first 3 * cond_frames): give one of them there")
            k[:, :, :nc] = cond.to(k.device, torch.float32)[:, None]
            m[:, :, :nc] = True
        ms, ks = m[:, :, :-3], torch.where(m[:, :, :-3], k[:, :, :-3], torch.zeros((), device=k.device))
        if not (bool((ms == ms[:, :1]).all()) and bool((ks == ks[:, :1]).all())):
            raise ValueError("the state channels of known / known_mask must be identical over the boundary copies of a design "
                             "(the chains share those channels over the boundary axis)")
        if noise is not None:
            parts = (noise.known_init, noise.known_state, noise.known_boundary)
            if any(q is None for q in parts):
                raise ValueError("a noise tape used with a known region needs known_init, known_state and known_boundary")
            ki, kst, kb = parts
            if (len(ki) != 2 or tuple(ki[0].shape) != (B, 1, Cc - 3, H, W) or tuple(ki[1].shape) != (B, nb, 3, H, W)
                    or kst.dim() != 6 or kb.dim() != 6 or kst.shape[0] < rows or kb.shape[0] < rows
                    or tuple(kst.shape[1:]) != (B, 1, Cc - 3, H, W) or tuple(kb.shape[1:]) != (B, nb, 3, H, W)):
                raise ValueError(f"the noise tape needs known_init ([{B}, 1, {Cc - 3}, {H}, {W}], [{B}, {nb}, 3, {H}, {W}]), known_state "
                                 f"[>= {rows}, {B}, 1, {Cc - 3}, {H}, {W}] and known_boundary [>= {rows}, {B}, {nb}, 3, {H}, {W}]")
        return k, m

    def known_replace(self, shape, x, known, known_mask, t, z=None):
        """The definition of the known region in torch (what the library's known2d_kernel does inside the captured
        step, and what the routes that loop in Python call): ``x[m] = q(k, t, z)`` for ``t >= 0``, ``x[m] = k`` for ``t < 0``,
        with ``q = sqrt_alphas_cumprod[t] * k + sqrt_one_minus_alphas_cumprod[t] * z``.  x [B*nb, C, H, W] (or [B, nb, C, H, W]);
        ``z``: a (state [B, 1, C-3, H, W], boundary [B, nb, 3, H, W]) pair -- the state draw is shared over the boundary copies --
        or a full tensor, or None for ``sample_noise``.  Returns a new tensor shaped like x."""
        B, nb, Cc, H, W = shape
        t = int(t)
        xs = x.reshape(shape)
        k = known.reshape(shape).to(xs.device, xs.dtype)
        m = torch.broadcast_to(known_mask.to(xs.device), tuple(shape))
        if t < 0:
            q = k
        else:
            if z is None:
                z = self.sample_noise(shape, xs.device)
            elif isinstance(z, (tuple, list)):
                z = torch.cat([z[0].expand(-1, nb, -1, -1, -1), z[1]], dim=2)
            z = z.reshape(shape).to(xs.device, xs.dtype)
            q = self.sqrt_alphas_cumprod[t].to(xs.device) * k + self.sqrt_one_minus_alphas_cumprod[t].to(xs.device) * z
        return torch.where(m, q, xs).reshape(x.shape)

    def _known_z(self, shape, noise, row, tag, seed, sample_offset, device):
        """The z of one overwrite on the routes that loop in Python -- the tape's known rows (``row`` None: known_init), else the
        library's counter-based draw under the known region's seed word, keyed like known2d_kernel keys it (``tag``)."""
        B, nb, Cc, H, W = shape
        if noise is not None:
            return noise.known_init if row is None else (noise.known_state[row], noise.known_boundary[row])
        cp = self.model.padded_channels
        z = torch.empty((B * nb, H * W, cp), dtype=torch.float32, device=device)
        with torch.cuda.device(device):
            _ffi.check(_ffi.lib().cindm_fill_noise2d(_ffi.ptr(z), B, nb, H * W, Cc, cp, (int(seed) ^ KNOWN_SEED) & (2 ** 64 - 1), sample_offset,
                                                     int(tag), _ffi.current_stream(device)))
        return from_device_layout(z, Cc, H, W)

    def _known_arm(self, h, kn, shape, noise, rows, device):
        """Arms the library handle with the known region for the next chain call (``cindm_ddpm1d_set_known2d``): values and the
        packed mask (one byte per channel group of four) in the library's layout, the tape's known rows channel-last.  Returns
        the device tensors, which the caller keeps alive over the chain call."""
        B, nb, Cc, H, W = shape
        cp = self.model.padded_channels
        k, m = kn
        kd = to_device_layout(k.reshape(B * nb, Cc, H, W).to(device, torch.float32), cp)
        md = to_device_layout(m.reshape(B * nb, Cc, H, W).to(device, torch.float32), cp).reshape(B * nb, H * W, cp // 4, 4)
        bits = (md * torch.tensor([1.0, 2.0, 4.0, 8.0], device=device)).sum(-1).to(torch.uint8).contiguous()
        zi_s = zi_b = z_s = z_b = None
        if noise is not None:
            zi_s = _state_cl(noise.known_init[0].to(device, torch.float32))
            zi_b = _boundary_cl(noise.known_init[1].to(device, torch.float32))
            z_s = _state_cl(noise.known_state[rows].to(device, torch.float32))
            z_b = _boundary_cl(noise.known_boundary[rows].to(device, torch.float32))
        _ffi.check(_ffi.lib().cindm_ddpm1d_set_known2d(h, _ffi.ptr(kd), _ffi.ptr(bits), _ffi.ptr(zi_s), _ffi.ptr(zi_b), _ffi.ptr(z_s),
                                                       _ffi.ptr(z_b), 0 if z_s is None else z_s[0].numel(),
                                                       0 if z_b is None else z_b[0].numel(), B * nb, H * W, cp))
        return kd, bits, zi_s, zi_b, z_s, z_b

    # ------------------------------------------------------------------ one reverse step
    @torch.no_grad()
    def _step(self, shape, x, t, clip_denoised, noise, add_noise=True):
        """(x_{t-1} without guidance, x_start, model_mean), all [B*nb, C, H, W]."""
        if not x.is_cuda:
            raise _ffi.CindmError("sampling needs ROCm device tensors; there is no CPU execution path")
        B, nb, Cc, H, W = shape
        cp = self.model.padded_channels
        xd = to_device_layout(x.float(), cp)
        x0 = torch.zeros_like(xd)
        mean = torch.zeros_like(xd)
        h, ws = self._prepare(B * nb, x.device)
        ns = nbnd = None
        if noise is not None and t > 0:
            nz = noise.reshape(B, nb, Cc, H, W).to(x.device, torch.float32)
            ns = _state_cl(nz[:, :1, :-3])
            nbnd = _boundary_cl(nz[:, :, -3:])
        elif t > 0 and add_noise:
            nz = self.sample_noise(shape, x.device)
            ns = _state_cl(nz[:, :1, :-3])
            nbnd = _boundary_cl(nz[:, :, -3:])
        with torch.cuda.device(x.device):
            _ffi.check(_ffi.lib().cindm_ddpm2d_step(h, self.model._h, _ffi.ptr(xd), B, nb, self._share_mode(),
                                                    int(clip_denoised), _ffi.ptr(ns), _ffi.ptr(nbnd), 0, 0, int(t), None,
                                                    _ffi.ptr(x0), _ffi.ptr(mean), _ffi.ptr(ws), ws.numel(),
                                                    _ffi.current_stream(x.device)))
        f = lambda y: from_device_layout(y, Cc, H, W)
        return f(xd), f(x0), f(mean)

    @torch.no_grad()
    def model_predictions(self, shape, x, t, x_self_cond=None, clip_x_start=False, rederive_pred_noise=False, share_noise=True):
        """:727-754 (all three objectives).  x [B*nb, C, H, W] -> ModelPrediction(pred_noise, pred_x_start): the Unet's output
        with its state channels shared over the boundary copies of a design (``share_noise``; mean or sum by
        ``use_average_share``), x_start = predict_start_from_noise (clamped when ``clip_x_start``), and with
        ``clip_x_start and rederive_pred_noise`` the noise re-derived from the clamped x_start.  One library call
        (``cindm_ddpm2d_predict``: U-Net + one element-wise kernel)."""
        if not x.is_cuda:
            raise _ffi.CindmError("sampling needs ROCm device tensors; there is no CPU execution path")
        if x_self_cond is not None:
            raise NotImplementedError("self-conditioning is outside this build's scope")
        B, nb, Cc, H, W = shape
        ti = self._t_int(t)
        cp = self.model.padded_channels
        xd = to_device_layout(x.float(), cp)
        eps, x0 = torch.zeros_like(xd), torch.zeros_like(xd)
        h, ws = self._prepare(B * nb, x.device)
        with torch.cuda.device(x.device):
            _ffi.check(_ffi.lib().cindm_ddpm2d_predict(h, self.model._h, _ffi.ptr(xd), B, nb,
                                                       int(bool(self.use_average_share)) | (_ffi.OBJECTIVES[self.objective] << 4),
                                                       int(bool(share_noise)), int(bool(clip_x_start)), int(bool(rederive_pred_noise)),
                                                       ti, None, _ffi.ptr(eps), _ffi.ptr(x0), _ffi.ptr(ws), ws.numel(),
                                                       _ffi.current_stream(x.device)))
        return ModelPrediction(from_device_layout(eps, Cc, H, W), from_device_layout(x0, Cc, H, W))

    @torch.no_grad()
    def p_mean_variance(self, shape, x, t, x_self_cond=None, clip_denoised=True):
        """:757-773.  Returns (model_mean, posterior_variance, posterior_log_variance, x_start)."""
        ti = self._t_int(t)
        _, x0, mean = self._step(shape, x, ti, clip_denoised, None, add_noise=False)
        return mean, self.posterior_variance[ti].view(1, 1, 1, 1), self.posterior_log_variance_clipped[ti].view(1, 1, 1, 1), x0

    @torch.no_grad()
    def p_sample(self, shape, x, t: int, x_self_cond=None, clip_denoised=True, design_fn=None, design_guidance="standard",
                 *, noise=None, recur_noise=None):
        """:788-889.  x [B*nb, C, H, W]; returns (x_{t-1}, x_start).  ``recur_noise`` [R, B*nb, C, H, W]: the relaxation
        draws of the "-recurrence-N" branch (else ``sample_noise``)."""
        t = int(t)
        if "recurrence" in design_guidance:
            # :846-889, literally: the posterior mean is computed once; every iteration subtracts the raw design gradient
            # taken at the current relaxed x (model_mean - grad_design) and re-noises; design_fn is required there
            if design_fn is None:
                raise ValueError("the 2-D recurrence guidance needs design_fn (the reference dereferences its gradient)")
            R = int(design_guidance.split("-")[-1])
            _, x_start, mean = self._step(shape, x, t, clip_denoised, None, add_noise=False)
            ratio = self.alphas_cumprod / self.alphas_cumprod_prev
            pred = mean
            xc = x.float()
            for r in range(R):
                with torch.enable_grad():
                    if design_guidance.startswith("standard"):
                        g = design_fn(xc.clone().detach().requires_grad_()).detach()
                    elif design_guidance.startswith("universal-forward-recurrence"):
                        g = design_fn(x_start.clone().detach().requires_grad_()).detach()
                    else:
                        raise NotImplementedError(design_guidance)
                pred = mean - g
                z = recur_noise[r].to(x.device) if recur_noise is not None else \
                    self.sample_noise(shape, x.device).view(-1, shape[2], shape[3], shape[4])
                xc = torch.sqrt(ratio)[t] * pred + torch.sqrt(1 - ratio)[t] * z
            if t > 0:
                z = noise.to(x.device) if noise is not None else self.sample_noise(shape, x.device).view(-1, shape[2], shape[3], shape[4])
                pred = pred + (0.5 * self.posterior_log_variance_clipped[t]).exp() * z
            return pred, x_start
        pred, x_start, _ = self._step(shape, x, t, clip_denoised, noise)
        if design_fn is None:
            return pred, x_start
        eta = (self.coeff_ratio * self.betas.flip(0))[t]

        def grad_of(z):
            with torch.enable_grad():
                return design_fn(z.clone().detach().requires_grad_()).detach()

        if design_guidance == "standard":
            shift = self.standard_fixed_ratio * grad_of(x)
        elif design_guidance == "standard-alpha":
            shift = eta * grad_of(x)
        elif design_guidance == "universal-forward":
            shift = self.forward_fixed_ratio * grad_of(x_start)
        elif design_guidance == "universal-backward":
            xc, shift = x_start.clone(), None
            for kk in range(self.backward_steps):
                gd = grad_of(xc)
                if kk == 1:
                    shift = self.forward_fixed_ratio * gd
                xc = xc - gd * self.backward_lr
            coef = (self.sqrt_alphas_cumprod * self.betas / (torch.sqrt(1 - self.betas) * (1 - self.alphas_cumprod)))[t]
            shift = shift - coef * (xc - x_start)
        else:
            raise ValueError(design_guidance)
        return pred - shift, x_start

    # ------------------------------------------------------------------ loops
    def _x_T(self, shape, noise, seed, sample_offset, device):
        """x_T in the device layout: the tape's init rows (state shared over a design's boundary copies), or the library's
        counter-based draw (``cindm_fill_noise2d``)."""
        B, nb, Cc, H, W = shape
        cp = self.model.padded_channels
        if noise is not None:
            return to_device_layout(torch.cat([noise.init[0].expand(-1, nb, -1, -1, -1), noise.init[1]], dim=2)
                                    .reshape(B * nb, Cc, H, W).to(device, torch.float32), cp)
        x = torch.empty((B * nb, H * W, cp), dtype=torch.float32, device=device)
        with torch.cuda.device(device):
            _ffi.check(_ffi.lib().cindm_fill_noise2d(_ffi.ptr(x), B, nb, H * W, Cc, cp, seed, sample_offset, self.num_timesteps,
                                                     _ffi.current_stream(device)))
        return x

    @staticmethod
    def _tape_cl(noise, device, rows=slice(None)):
        """(ns, nbnd): a tape's per-step draws (``rows`` of them) channel-last on the device, or (None, None) without a tape."""
        if noise is None:
            return None, None
        return (_state_cl(noise.step_state[rows].to(device, torch.float32)),
                _boundary_cl(noise.step_boundary[rows].to(device, torch.float32)))

    def _recorder(self, every, trajectory, n, shape, device, **when):
        """The DeviceRecorder of a library chain of ``n`` steps over ``shape`` [B, nb, C, H, W] (one record = the state in the
        library's layout, [B * nb, H * W, padded channels]), or None without the keyword."""
        if every is None:
            return None
        B, nb, Cc, H, W = shape
        return DeviceRecorder(n, every, trajectory, B * nb * H * W * self.model.padded_channels, device, **when)

    def _recorded(self, out, rec, shape):
        """What a sampling call returns: the designs, or (designs, ChainRecord) when it recorded."""
        if rec is None:
            return out
        if isinstance(rec, LoopRecorder):
            return out, rec.result(shape)
        B, nb, Cc, H, W = shape
        cp = self.model.padded_channels

        def unpack(rows):
            n = rows.shape[0]
            return from_device_layout(rows.reshape(n * B * nb, H * W, cp), Cc, H, W).reshape(n, B, nb, Cc, H, W)
        return out, rec.collect(self._handle(), unpack)

    def _chain2(self, shape, x, rec, call, known=None, ms=None):
        """One library chain on the state ``x`` (device layout, updated in place): the workspace, the recorder and the known
        region (``known`` = (region, tape, its rows)) armed, the entry ``call(L, h, ws)`` and what the sampling call returns."""
        B, nb, Cc, H, W = shape
        h, ws = self._prepare(B * nb, x.device)
        if rec is not None:
            rec.arm(h)
        keep = None if known is None else self._known_arm(h, known[0], shape, known[1], known[2], x.device)      # (alive over the call)
        self._arm_multistep(ms, h)      # (``ms``: the multistep solver of a DDIM call, DiffusionHandle._multistep)
        with torch.cuda.device(x.device):
            _ffi.check(call(_ffi.lib(), h, ws))
        return self._recorded(from_device_layout(x, Cc, H, W).reshape(B, nb, Cc, H, W), rec, shape)

    def _force_part(self, fo, shape, device, buffers=True):
        """A ForceObjective's part of a guided library call: (surrogate handle, its scalar arguments in ABI order, gradient buffer,
        surrogate workspace).  ``buffers=False``: the shape check alone (the routes that loop in Python call the objective itself)."""
        B, nb, Cc, H, W = shape
        if (fo.B, fo.nb) != (B, nb) or Cc != 3 * fo.frames + 3:
            raise ValueError("ForceObjective was built for another batch / boundary / frame count")
        if not buffers:
            return None
        fo.model.sync_weights()
        nfb = _ffi.lib().cindm_airfoil_design_workspace_bytes(fo.model._h, B, nb, fo.frames_per_pass)
        wsf = torch.empty(nfb, dtype=torch.uint8, device=device)
        g = torch.empty((B * nb, H * W, self.model.padded_channels), dtype=torch.float32, device=device)
        return fo.model._h, (fo.frames, fo.p_min, fo.p_max, fo.lambda_force, fo.lambda_overlap, fo.factor, int(fo.sum_boundary)), g, wsf

    @torch.no_grad()
    def p_sample_loop(self, shape, design_fn=None, design_guidance="standard", return_all_timesteps=None, *,
                      noise=None, seed=0, sample_offset=0, use_graph=True, t_stop=0, device=None, fused=True,
                      return_trajectory_every=None, trajectory=("x",), known=None, known_mask=None, cond=None, solver="ddim"):
        """:893-907.  Returns [B, nb, C, H, W].  ``noise``: a NoiseTape2D (parity runs); otherwise x_T and the
        per-step draws come from the library's counter-based generator keyed by (seed, sample_offset + design).
        ``return_trajectory_every=k`` with ``trajectory=("x",)`` / ``("x", "x0")``: returns (designs, ChainRecord) with the state
        [n_records, B, nb, C, H, W] after every k-th step and after the last one (record.py; recorded inside the captured step on the
        library routes, cloned per step on the routes that loop in Python).
        Replacement conditioning (build-only; the reference's 2-D sampler takes no condition): ``known`` [B, nb, C, H, W] with
        ``known_mask`` (bool, broadcastable to it) names a region of the state and its clean values k; ``cond`` [B, 3 * cond_frames,
        H, W] is the convenience for "the first 3 * cond_frames channels are known on every boundary copy" (on the same channels
        as ``known`` it is a ValueError).  With q(k, t, z) = sqrt_alphas_cumprod[t] k + sqrt_one_minus_alphas_cumprod[t] z:
        before the first step, at t0 = T - 1, x[m] = q(k, t0, z_init); after the step at t (its update and guidance shift),
        x[m] = q(k, t - 1, z) for t >= 1 and x[m] = k after t = 0 -- so the result carries k exactly (with ``t_stop`` > 0 the chain
        ends at level t_stop - 1, like the rest of its state).  z is drawn like ``sample_noise`` at every step (tape rows
        ``known_init`` / ``known_state[t]`` / ``known_boundary[t]``, else the counter-based generator under a seed word of its own).
        This differs on purpose from the 1-D inpainting, which copies the reference: level t after the step at t, and nothing on
        the last DDIM pair.  The state channels of known and mask must be identical over the boundary copies (ValueError).  Inside
        the captured step on the library routes (known2d_kernel), ``known_replace`` on the routes that loop in Python; a recorder
        records after the overwrite.
        ``solver``: "ddim" (nothing changes); "dpmpp-2m" is a ValueError here -- this is the DDPM chain (see ddim_sample)."""
        if check_solver(self, solver):
            raise ValueError("solver='dpmpp-2m' runs on the DDIM chains: p_sample_loop is the DDPM chain (sample() with "
                             "sampling_timesteps < timesteps, or ddim_sample)")
        B, nb, Cc, H, W = shape
        T = self.num_timesteps
        kn = self._known_region(shape, known, known_mask, cond, noise, T)
        device = device or self.betas.device
        if device.type != "cuda":
            raise _ffi.CindmError("sampling needs a ROCm device; there is no CPU execution path")
        karm = None if kn is None else (kn, noise, slice(None))
        # (the device record buffer is allocated only on the routes that are library chains)
        device_rec = lambda: self._recorder(return_trajectory_every, trajectory, T - int(t_stop), shape, device, t_start=T - 1)
        x = self._x_T(shape, noise, seed, sample_offset, device)
        stream, share = _ffi.current_stream(device), self._share_mode()
        if design_fn is None:
            ns, nbnd = self._tape_cl(noise, device)
            return self._chain2(shape, x, device_rec(), lambda L, h, ws: L.cindm_ddpm2d_sample(
                h, self.model._h, _ffi.ptr(x), B, nb, share, _ffi.ptr(ns), _ffi.ptr(nbnd), seed, sample_offset, T - 1, int(t_stop),
                _ffi.ptr(ws), ws.numel(), stream, int(use_graph)), karm)
        from .forceunet import ForceObjective
        if isinstance(design_fn, ForceObjective) and design_guidance == "standard-alpha" and fused:
            # the library's own objective: surrogate forward + input gradient, the reverse step and the guidance shift are
            # ONE captured graph per timestep (cindm_ddpm2d_sample_force), as PointObjective is in the 1-D path
            fh, fargs, g, wsf = self._force_part(design_fn, shape, device)
            eta = (self.coeff_ratio * self.betas.flip(0)).to(device, torch.float32).contiguous()
            ns, nbnd = self._tape_cl(noise, device)
            return self._chain2(shape, x, device_rec(), lambda L, h, ws: L.cindm_ddpm2d_sample_force(
                h, self.model._h, fh, _ffi.ptr(x), B, nb, share, _ffi.ptr(ns), _ffi.ptr(nbnd), seed, sample_offset, T - 1, int(t_stop),
                *fargs, _ffi.ptr(eta), _ffi.ptr(g), _ffi.ptr(ws), ws.numel(), _ffi.ptr(wsf), wsf.numel(), stream, int(use_graph)), karm)
        # this route loops in Python: the same record, cloned per step
        rec = None if return_trajectory_every is None else LoopRecorder(T - int(t_stop), return_trajectory_every, trajectory, t_start=T - 1)
        img = from_device_layout(x, Cc, H, W)
        if kn is not None:
            img = self.known_replace(shape, img, kn[0], kn[1], T - 1, self._known_z(shape, noise, None, T, seed, sample_offset, device))
        for i, t in enumerate(reversed(range(int(t_stop), T))):
            nz = None
            if noise is not None and t > 0:
                nz = torch.cat([noise.step_state[t].expand(-1, nb, -1, -1, -1), noise.step_boundary[t]], dim=2)
            img, x_start = self.p_sample(shape, img, t, None, design_fn=design_fn, design_guidance=design_guidance, noise=nz)
            if kn is not None:
                img = self.known_replace(shape, img, kn[0], kn[1], t - 1,
                                         None if t == 0 else self._known_z(shape, noise, t, t - 1, seed, sample_offset, device))
            if rec is not None:
                rec.after(i, img, x_start)
        return self._recorded(img.reshape(B, nb, Cc, H, W), rec, shape)

    # ------------------------------------------------------------------ DDIM
    def ddim_guidance_weights(self):
        """fp32 [S]: the "standard-alpha" guidance weight of every DDIM step -- for the pair (t, t_next) of ddim_schedule() the sum
        (in float64, rounded once) of eta = coeff_ratio * betas.flip(0) over the DDPM steps t_next+1 .. t that the step stands for,
        i.e. the guidance ``p_sample`` would have applied on the way.  Strides of one step give eta[t] itself."""
        times, _ = self.ddim_schedule()
        eta = (self.coeff_ratio * self.betas.detach().to("cpu", torch.float32).flip(0)).double()
        return torch.stack([eta[tn + 1:t + 1].sum() for t, tn in zip(times[:-1], times[1:])]).float()

    @torch.no_grad()
    def ddim_sample(self, shape, design_fn=None, design_guidance="standard", return_all_timesteps=False, *, noise=None, seed=0,
                    sample_offset=0, use_graph=True, init_img=None, step_range=None, device=None, fused=True,
                    return_trajectory_every=None, trajectory=("x",), known=None, known_mask=None, cond=None, solver="ddim",
                    history=None):
        """DDIM sampling of the 2-D path (:910-949; the reference's own body cannot run, so this build defines it from its
        working pieces).  Returns [B, nb, C, H, W].  With (times, coefs) = ddim_schedule(), for each pair (t, t_next):
        (pred_noise, x_start) = model_predictions(x, t, clip_x_start=True, rederive_pred_noise=True, share_noise=True);
        x = x_start if t_next < 0, else x_start * sqrt(alpha_next) + c * pred_noise + sigma * z, with z = sample_noise (state
        channels shared over the boundary copies of a design, boundary channels per image).  x_T is sample_noise too.
        The whole loop is one library call (``cindm_ddpm2d_sample_ddim``: one captured HIP graph step replayed per DDIM step).
        Guided: ``design_fn`` = a ``ForceObjective`` with ``design_guidance="standard-alpha"`` subtracts, at every step (the last
        pair included), ``ddim_guidance_weights()[i] * design_fn(x_t)`` -- the gradient at the step's INPUT state, as p_sample's
        "standard-alpha" branch takes it -- from that update; x_T and z are the unguided chain's.  One library call too
        (``cindm_ddpm2d_sample_ddim_force``); ``fused=False`` runs the same definition step by step from Python.
        Build-only keywords: ``noise`` = a NoiseTape2D whose ``step_*`` rows are indexed by the DDIM STEP index; otherwise x_T
        and z come from the library's counter-based generator keyed by (seed, sample_offset + design); ``init_img`` +
        ``step_range=(i0, i1)`` run DDIM steps i0 .. i1-1 from a given state (teacher-forced segments for parity tests: the
        deterministic sampler amplifies a 1e-6 difference of the U-Net to 1e-3 over long chains).
        ``return_trajectory_every`` / ``trajectory``: as p_sample_loop, steps counted from the first step this call runs; the stream
        ``x`` only -- the 2-D DDIM update kernels have no x0 operand.
        Replacement conditioning: ``known`` / ``known_mask`` / ``cond`` as p_sample_loop (build-only).  Before the first step this
        call runs, at t0 = times[i0], x[m] = q(k, t0, z_init); after the step of the pair (t, t_next) -- its update and guidance
        shift -- x[m] = q(k, t_next, z) when t_next >= 0 and x[m] = k when t_next < 0, so the result carries k exactly.  z is drawn
        like sample_noise at every step, whatever sigma is (tape rows ``known_init`` / ``known_state[i]`` / ``known_boundary[i]`` by
        DDIM step index).  This differs on purpose from the 1-D inpainting, which copies the reference: level t after the step at
        t, and nothing on the last DDIM pair.  A recorder records after the overwrite.
        ``solver="dpmpp-2m"``: the second-order multistep solver on the same grid at no extra U-Net evaluation --
        step i adds ``multistep_kappa()[i] * (x_start_i - x_start_{i-1})`` to its DDIM value (each operation rounded once) ahead of
        the guidance shift, the known region and the recorder; the first step and the last pair are plain DDIM steps.  Inside the
        update kernel on the library routes; ``fused=False`` applies it in torch on ``model_predictions``' x_start.  Needs
        ``ddim_sampling_eta == 0`` and ``sampling_timesteps < timesteps`` (ValueError).  With ``step_range=(i0, i1)`` the call takes
        ``history=`` [B, nb, C, H, W] (the x_start of step i0 - 1: required when i0 > 0) and returns (result, history of step i1 - 1).
        Refused (NotImplementedError): any other ``design_fn`` or guidance (the reference has no working guided 2-D DDIM),
        share_noise False and ``return_all_timesteps``."""
        from .forceunet import ForceObjective
        ms_on = self._check_solver(solver, step_range, history)
        if design_fn is not None and not (isinstance(design_fn, ForceObjective) and design_guidance == "standard-alpha"):
            raise NotImplementedError("DDIM with design_fn: only a ForceObjective under design_guidance='standard-alpha' has a DDIM form "
                                      "(the reference has no working guided 2-D DDIM; its ddim_sample takes no design_fn); sample with "
                                      "sampling_timesteps == timesteps for any other design_fn or guidance")
        if not self.share_noise:
            raise NotImplementedError("DDIM with share_noise=False: the reference's 2-D DDIM shares the predicted noise "
                                      "(model_predictions share_noise=True); there is no DDIM form of the shared posterior mean")
        if return_all_timesteps:
            raise NotImplementedError("return_all_timesteps is outside this build's scope (the reference's 2-D sampler does not build it)")
        if return_trajectory_every is not None and stream_mask(trajectory) & 2:
            raise NotImplementedError("trajectory 'x0' in 2-D DDIM: the DDIM update kernels have no x0 operand (the DDPM loop records it)")
        B, nb, Cc, H, W = shape
        kn = self._known_region(shape, known, known_mask, cond, noise,
                                (len(self.ddim_schedule()[0]) - 1) if step_range is None else int(step_range[1]))
        device = device or self.betas.device
        if device.type != "cuda":
            raise _ffi.CindmError("sampling needs a ROCm device; there is no CPU execution path")
        fo = design_fn
        force = None if fo is None else self._force_part(fo, shape, device, buffers=fused)
        cp = self.model.padded_channels
        times, coefs = self.ddim_schedule()
        i0, i1 = (0, len(times) - 1) if step_range is None else step_range
        if not 0 <= i0 < i1 <= len(times) - 1:
            raise ValueError(f"step_range must satisfy 0 <= i0 < i1 <= {len(times) - 1}")
        if noise is not None:
            if (noise.step_state.shape[0] < i1 or noise.step_boundary.shape[0] < i1 or tuple(noise.step_state.shape[1:]) != (B, 1, Cc - 3, H, W)
                    or tuple(noise.step_boundary.shape[1:]) != (B, nb, 3, H, W)):
                raise ValueError(f"the noise tape needs step_state [>= {i1}, {B}, 1, {Cc - 3}, {H}, {W}] and step_boundary "
                                 f"[>= {i1}, {B}, {nb}, 3, {H}, {W}] (rows indexed by the DDIM step)")
        if init_img is not None:
            x = to_device_layout(init_img.reshape(B * nb, Cc, H, W).to(device, torch.float32), cp)
        else:
            x = self._x_T(shape, noise, seed, sample_offset, device)
        ms = self._multistep(ms_on, i0, i1, history, x,
                             pack=lambda v: to_device_layout(v.reshape(B * nb, Cc, H, W).to(device, torch.float32), cp))
        # (a segment call of the multistep solver hands the history of its last step back beside its result)
        handed = (lambda out: (out, from_device_layout(ms[1], Cc, H, W).reshape(B, nb, Cc, H, W))) \
            if (ms is not None and step_range is not None) else (lambda out: out)
        if fo is not None and not fused:
            # the same definition from existing calls: the objective, one unguided DDIM step, the shift in torch
            w = self.ddim_guidance_weights()
            img = from_device_layout(x, Cc, H, W)
            lrec = None if return_trajectory_every is None else \
                LoopRecorder(i1 - i0, return_trajectory_every, trajectory, times=times[i0:i1 + 1])
            if kn is not None:
                img = self.known_replace(shape, img, kn[0], kn[1], times[i0], self._known_z(shape, noise, None, self.num_timesteps, seed,
                                                                                           sample_offset, device))
            x_prev = None if (ms is None or ms[2] is None) else from_device_layout(ms[2], Cc, H, W)
            for i in range(i0, i1):
                g = fo(img)
                if ms is not None:      # the x_start the step's update forms (clamped; the same U-Net evaluation, made once more)
                    x_start = self.model_predictions(shape, img, times[i], clip_x_start=True, rederive_pred_noise=True).pred_x_start
                img = self.ddim_sample(shape, noise=noise, seed=seed, sample_offset=sample_offset, use_graph=use_graph, init_img=img,
                                       step_range=(i, i + 1), device=device).reshape(B * nb, Cc, H, W)
                if ms is not None:      # the multistep term (kappa == 0 reads no history; the last pair returns x_start)
                    if times[i + 1] >= 0 and float(ms[0][i - i0]) != 0.0:
                        img = img + ms[0][i - i0].to(device) * (x_start - x_prev)
                    x_prev = x_start
                img = img - w[i] * g
                if kn is not None:
                    tn = times[i + 1]
                    img = self.known_replace(shape, img, kn[0], kn[1], tn,
                                             None if tn < 0 else self._known_z(shape, noise, i, tn, seed, sample_offset, device))
                if lrec is not None:
                    lrec.after(i - i0, img)
            if ms is not None:
                ms[1].copy_(to_device_layout(x_prev, cp))
            return handed(self._recorded(img.reshape(B, nb, Cc, H, W), lrec, shape))
        times, coefs = times[i0:i1 + 1], coefs[i0:i1].contiguous()
        S = len(times) - 1
        rec = self._recorder(return_trajectory_every, trajectory, S, shape, device, times=times)
        ns, nbnd = self._tape_cl(noise, device, slice(i0, i1))
        karm = None if kn is None else (kn, noise, slice(i0, i1))
        # the per-step device tables live in a caller tensor (the library allocates nothing): [S][4] coefficients + [S] time_next
        # (the multistep solver's kappa sits behind them: a sixth word per step)
        if self._ddim_tab is None or self._ddim_tab.numel() < 6 * S or self._ddim_tab.device != device:
            self._ddim_tab = torch.empty(6 * max(S, self.sampling_timesteps), dtype=torch.float32, device=device)
        tab = self._ddim_tab
        tarr = (C.c_int32 * (S + 1))(*times)
        stream, share = _ffi.current_stream(device), self._share_mode()
        if fo is not None:
            # the library's own objective: surrogate gradient, U-Net and the update that carries the shift are ONE captured graph
            # per DDIM step (cindm_ddpm2d_sample_ddim_force); the weights ride in the 4th word of the table rows
            fh, fargs, g, wsf = force
            w = self.ddim_guidance_weights()[i0:i1].contiguous()
            return handed(self._chain2(shape, x, rec, lambda L, h, ws: L.cindm_ddpm2d_sample_ddim_force(
                h, self.model._h, fh, _ffi.ptr(x), B, nb, share, S, tarr, _ffi.ptr(coefs), _ffi.ptr(w), _ffi.ptr(tab), tab.numel() * 4,
                _ffi.ptr(ns), _ffi.ptr(nbnd), seed, sample_offset, *fargs, _ffi.ptr(g), _ffi.ptr(ws), ws.numel(), _ffi.ptr(wsf),
                wsf.numel(), stream, int(use_graph)), karm, ms))
        return handed(self._chain2(shape, x, rec, lambda L, h, ws: L.cindm_ddpm2d_sample_ddim(
            h, self.model._h, _ffi.ptr(x), B, nb, share, S, tarr, _ffi.ptr(coefs), _ffi.ptr(tab), tab.numel() * 4, _ffi.ptr(ns),
            _ffi.ptr(nbnd), seed, sample_offset, _ffi.ptr(ws), ws.numel(), stream, int(use_graph)), karm, ms))

    @torch.no_grad()
    def sample(self, batch_size=16, design_fn=None, design_guidance="standard", num_boundaries=1,
               return_all_timesteps=False, **kw):
        """:960-963 (``sampling_timesteps < timesteps``: ddim_sample).  ``kw``: the build-only keywords of p_sample_loop /
        ddim_sample, ``return_trajectory_every=`` / ``trajectory=`` and the replacement conditioning ``known=`` / ``known_mask=`` /
        ``cond=`` among them, and ``solver=`` ("ddim" | "dpmpp-2m", see ddim_sample)."""
        check_solver(self, kw.get("solver", "ddim"))
        S = self.image_size
        shape = (batch_size, num_boundaries, self.channels, S, S)
        if self.is_ddim_sampling:
            return self.ddim_sample(shape, design_fn, design_guidance, return_all_timesteps=return_all_timesteps, **kw)
        return self.p_sample_loop(shape, design_fn, design_guidance, return_all_timesteps=return_all_timesteps, **kw)

    def forward(self, *a, **k):
        raise NotImplementedError("training (p_losses) is out of this build's scope (SURVEY.md section 8)")
