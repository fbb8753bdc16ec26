"""GaussianDiffusion1D (sampling half) on MI355X: the reference's constructor / buffers / ``sample``
surface (model/diffusion_1d.py:801-2406 of AI4Science-WestlakeU/cindm) over the HIP library.

What runs where
  * every U-Net evaluation, the window / body-pair gather, the score composition, x0 prediction,
    clamp, posterior mean and the noise add run in ``libcindm_hip.so``;
  * with ``design_fn=None`` (and no recurrence / overwrite) the whole reverse loop is ONE call
    (``cindm_ddpm1d_sample``: one hipGraph-captured step replayed per timestep);
  * ``design_fn`` guidance is a user Python callable: its gradient is taken by PyTorch autograd
    between two library calls per step, exactly where the reference takes it.
  * DDIM (``sampling_timesteps < timesteps``, ``ddim_sample`` :1724-1804): unguided = ONE library call
    (``cindm_ddpm1d_sample_ddim``, same captured-step replay with per-step coefficient tables); guided by a ``PointObjective``,
    a ``WaypointObjective``, a ``QuadraticObjective`` or a ``PairDistanceObjective`` ("standard" / "standard-alpha" with ``-recurrence-N``) = ONE library call too (``cindm_ddpm1d_sample_ddim_guided``: relaxation
    iterations and the DDIM update of (eps + grad, x_start) inside the captured step, state and step state ping-ponged); guided by
    any other callable or guidance (recurrence guidance) = library predictions + the user's gradient per step.
  * autoregressive time composition (``autoregress_time_compose_sample`` :2240-2327): the whole rollout -- every segment's
    DDIM chain and the hand-over of its tail to the next segment -- is ONE library call (``cindm_ddpm1d_sample_autoregress``,
    the DDIM step's captured graph replayed for every segment).
  * parallel time composition (``composing_time_sample`` :1807-1854): all segments side by side as ONE DDIM chain on
    (n_composed + 1) * B rows (``cindm_ddpm1d_sample_timecompose``); the update of every step also hands each segment's noisy tail
    over to the next segment's condition.
  * the Langevin (ULA) phase of ``sample_compose_multibodies`` for N > 401 (:2002-2022, ``sample_step_ULA`` :2048-2073): ONE library
    call for the whole phase (``cindm_ddpm1d_sample_ula``: one captured Langevin iteration replayed (N - 401) * L times, timestep and
    inner index advancing on the device), then the DDPM loop above from t = 400 on the drifted conditioning rows.
Training (``forward`` / ``p_losses``) and the UHMC samplers of the reference (dead code there: undefined names) are out of this
build's scope and raise NotImplementedError.
"""
import ctypes as C
from collections import namedtuple

import torch
from torch import nn

from . import _ffi
from .diffusion_base import DiffusionHandle
from .objectives import PointObjective, SumObjective, _TableObjective
from .record import DeviceRecorder, LoopRecorder, record_schedule, stream_mask
from .schedule import check_solver, make_schedule, ula_schedule

ModelPrediction = namedtuple("ModelPrediction", ["pred_noise", "pred_x_start"])


class NoiseTape:
    """Explicit noise for parity runs, replacing the reference's ``torch.randn`` draws:
    ``init`` [B,L,F] (x_T, :1673 / :1987); ``step`` [T,B,L,F] indexed by timestep (:1281 / :1118);
    ``recur`` [T,R,B,L,F] relaxation draws (:1365); ``cond`` [T,B,Lc,F] inpainting draws (:1717).
    ``autoregress_time_compose_sample`` reads a leading SEGMENT index: ``init`` [K,B,R,F] (each segment's x_T, :2299 /
    :2264) and ``step`` [K,S,B,R,F] (segment k's draw of DDIM step i, :2315 / :2280).
    ``ula`` [n_t,L,B,Lc+R,F]: the Langevin draws of ``sample_compose_multibodies`` with N > 401 (:2056), on the WHOLE state, in
    the order they are drawn: row 0 of the first axis is timestep N - 1.
    Keyword-only, the draws of a known region's forward diffusion (``known=`` of the sampling calls): ``known_init``
    [B,L,F] (rule 1), ``known_step`` [rows,B,L,F] indexed like ``step`` (by t, or by the DDIM step index), ``known_recur``
    [rows,iters,B,L,F] shaped like ``recur`` (record r is used after relaxation r; the last one is unused)."""

    def __init__(self, init, step, recur=None, cond=None, ula=None, *, known_init=None, known_step=None, known_recur=None):
        self.init, self.step, self.recur, self.cond, self.ula = init, step, recur, cond, ula
        self.known_init, self.known_step, self.known_recur = known_init, known_step, known_recur

    def to(self, device):
        f = lambda t: None if t is None else t.to(device=device, dtype=torch.float32).contiguous()
        return NoiseTape(f(self.init), f(self.step), f(self.recur), f(self.cond), f(self.ula), known_init=f(self.known_init),
                         known_step=f(self.known_step), known_recur=f(self.known_recur))


# the seed word of a known region's counter-based draws (known1d_kernel's kKnown1dSeed): distinct from the step, relaxation and
# inpainting draws' words
KNOWN_SEED = 0x6b6e6f776e316421


def _exists(x):
    return x is not None


_SEGMENT_SEED_STRIDE = 0x9E3779B97F4A7C15


def autoregress_segment_seeds(seed, n_seg):
    """The seeds of the autoregressive rollout's segments: seed_k = (seed + k * 0x9E3779B97F4A7C15) mod 2**64, so seed_0 = seed
    and a one-segment rollout is ``ddim_sample(seed=seed)``.  Segment k draws its x_T and its step noise as
    ``ddim_sample(seed=seed_k)`` does."""
    return [(int(seed) + k * _SEGMENT_SEED_STRIDE) % (1 << 64) for k in range(n_seg)]


def autoregress_segments(conditioned_steps, rollout_steps, n_composed, is_single_step_prediction=False, prediction_steps=40):
    """Number of segments of ``autoregress_time_compose_sample`` (:2252-2259 / :2296): n_composed + 1, or
    ceil(prediction_steps / conditioned_steps) for the single-step variant.  Raises for the cases where the reference fails."""
    Lc, R = int(conditioned_steps), int(rollout_steps)
    if Lc == 0:
        raise NotImplementedError("autoregress_time_compose_sample with conditioned_steps == 0: the reference hands img[:, -0:] (the whole "
                                  "state) over as the next condition and its slice assignment into the output fails on shape")
    if R < Lc:
        raise NotImplementedError(f"autoregress_time_compose_sample with rollout_steps (image_size) {R} < conditioned_steps {Lc}: the next "
                                  "segment's condition img[:, -conditioned_steps:] is shorter than the model's horizon needs")
    if not is_single_step_prediction:
        if int(n_composed) < 0:
            raise ValueError(f"n_composed must be >= 0, got {n_composed}")
        return int(n_composed) + 1
    P = int(prediction_steps)
    if P < 1:
        raise ValueError(f"prediction_steps must be >= 1, got {P}")
    K = -(-P // Lc)
    if K * R != P:
        raise ValueError(f"single-step prediction: ceil(prediction_steps / conditioned_steps) * rollout_steps = {K} * {R} != prediction_steps "
                         f"{P}: the reference's last slice assignment into its [B, {P}, F] output fails on shape")
    return K


def time_compose_segments(conditioned_steps, image_size, n_composed):
    """Number of segments of ``composing_time_sample`` (:1815): n_composed + 1.  Raises for the cases where the reference fails
    or returns nothing."""
    Lc, R = int(conditioned_steps), int(image_size)
    if Lc == 0:
        raise NotImplementedError("composing_time_sample with conditioned_steps == 0: the reference hands img_infered[:, -0:] (the whole "
                                  "state) over as the next condition and its slice assignment fails on shape")
    if int(n_composed) < 1:
        raise ValueError(f"n_composed must be >= 1, got {n_composed}: the reference returns an empty second tensor")
    if R < Lc:
        raise ValueError(f"composing_time_sample with image_size {R} < conditioned_steps {Lc}: the next segment's condition "
                         "img_infered[:, -conditioned_steps:] is shorter than the model's horizon needs")
    return int(n_composed) + 1


def time_compose_assemble(x, n_seg):
    """What ``composing_time_sample`` returns (:1848-1854) from the final state x [n_seg * B, R, F], segment-major: segment 0
    [B, R, F] and the last min(20, R) rows (the reference's literal ``-20:``) of segments 1 .. n_seg - 1, in segment order along
    the row axis: [B, (n_seg - 1) * min(20, R), F]."""
    B = x.shape[0] // n_seg
    return x[:B].clone(), torch.cat([x[k * B:(k + 1) * B, -20:] for k in range(1, n_seg)], dim=1)


class GaussianDiffusion1D(DiffusionHandle, nn.Module):
    """Drop-in for the reference's ``GaussianDiffusion1D`` (constructor :802-822)."""

    def __init__(self, model, model_unconditioned=None, betas_inference=None, *, image_size, conditioned_steps,
                 timesteps=1000, sampling_timesteps=None, loss_type="l1", objective="pred_noise",
                 beta_schedule="cosine", ddim_sampling_eta=0., auto_normalize=True, loss_weight_discount=0.95,
                 num_time_steps_UHMC=100, is_diffusion_condition=None, backward_steps=5, backward_lr=1):
        super().__init__()
        self.model = model
        self.model_unconditioned = model_unconditioned
        self.betas_inference = betas_inference
        self.channels = self.model.channels
        self.is_diffusion_condition = is_diffusion_condition
        self.self_condition = False
        self.num_timesteps_UHMC = num_time_steps_UHMC
        self.image_size = image_size
        self.conditioned_steps = conditioned_steps
        self.rollout_steps = image_size
        self.objective = objective
        self.backward_steps = backward_steps
        self.backward_lr = backward_lr
        assert objective in {"pred_noise", "pred_x0", "pred_v"}, "objective must be pred_noise, pred_x0 or pred_v"
        tables = make_schedule(beta_schedule, timesteps, objective)
        self.num_timesteps = int(timesteps)
        self._check_model_timesteps(model, timesteps)
        self.loss_type = loss_type
        self.loss_weight_discount = loss_weight_discount
        self.sampling_timesteps = sampling_timesteps if _exists(sampling_timesteps) else timesteps
        assert self.sampling_timesteps <= timesteps
        self.is_ddim_sampling = self.sampling_timesteps < timesteps
        self.ddim_sampling_eta = ddim_sampling_eta
        for name in _ffi.SCHED_NAMES:               # the 13 buffers, same names and order (:873-910)
            self.register_buffer(name, tables[name])
        self._h = None
        self._tab_sig = None
        self._ws = None

    def _compose_desc(self, mode, n_composed, compose_start_step, window, n_bodies, clip=True, uncond_coef=1.4):
        c = _ffi.ComposeDesc()
        c.mode, c.n_windows, c.compose_start_step, c.window = mode, n_composed + 1, compose_start_step, window
        c.n_bodies, c.cond_steps = n_bodies, self.conditioned_steps
        # (coefficient_unconditioned_grad: 1.4 in the 4-body branch of gradient(), :1900; the 3-body branch subtracts the plain prediction, :1958)
        c.objective, c.clip_denoised, c.uncond_coef = _ffi.OBJECTIVES[self.objective], int(clip), uncond_coef
        return c

    def _desc_for(self, x_shape, compose_mode=None, n_composed=0, compose_start_step=4, single_model_step=-1,
                  compose_n_bodies=2, clip=True, outside=False):
        """Maps the reference's keyword soup onto a compose descriptor."""
        if outside:
            if compose_mode == "mean":
                mode = _ffi.COMPOSE_MEAN_OUTSIDE
            elif compose_mode == "noise_sum":
                mode = _ffi.COMPOSE_NOISESUM_OUTSIDE
            else:
                raise ValueError(f"unknown compose_mode {compose_mode!r}")
            return self._compose_desc(mode, n_composed, compose_start_step, single_model_step, compose_n_bodies, clip)
        if compose_mode is not None and "inside" in compose_mode:
            if compose_mode == "mean-inside":
                mode = _ffi.COMPOSE_MEAN_INSIDE
            elif compose_mode == "sum-inside":
                mode = _ffi.COMPOSE_SUM_INSIDE
            else:
                raise ValueError(f"unknown compose_mode {compose_mode!r}")
            return self._compose_desc(mode, n_composed, compose_start_step, single_model_step, compose_n_bodies, clip)
        nb = x_shape[-1] // 4
        if self.model_unconditioned is not None:           # :1003-1004 -> gradient()
            if nb != 4:
                raise NotImplementedError("model_predictions calls gradient(x, t, 4) whatever the state's width (model/diffusion_1d.py:1004): "
                                          "with model_unconditioned set the state must hold 4 bodies (the 3-body branch: gradient(x_t, t, 3))")
            return self._compose_desc(_ffi.COMPOSE_MULTIBODY, 0, 0, self.model.horizon, nb, clip)
        return self._compose_desc(_ffi.COMPOSE_PLAIN, 0, 0, self.model.horizon, nb, clip)

    def _prepare(self, desc, B, device):
        self.model.sync_weights()
        if desc.mode == _ffi.COMPOSE_MULTIBODY:
            self.model_unconditioned.sync_weights()
        L = _ffi.lib()
        h = self._handle()
        un = self.model_unconditioned._h if desc.mode == _ffi.COMPOSE_MULTIBODY else None
        nbytes = L.cindm_ddpm1d_workspace_bytes(h, self.model._h, un, C.byref(desc), B)
        if nbytes == 0:
            raise _ffi.CindmError(L.cindm_last_error().decode() or "invalid composition")
        if self._ws is None or self._ws.numel() < nbytes or self._ws.device != device:
            self._ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
        return h, un, self._ws

    _warned_crowded = False

    def last_chain_info(self):
        """What the last library chain (``sample`` / ``ddim_sample`` / the built-in guided loop) of this object did:
        ``recovered`` -- an in-kernel exchange timed out and the chain was re-run once on the exchange-free plan;
        ``exchange_free_up_front`` -- another chain was already in flight on this device in this process, so this one ran on the
        exchange-free plan from the start (correct, about 10 % slower); ``chains_in_flight`` when it started, itself included."""
        info = (C.c_int32 * 4)()
        _ffi.check(_ffi.lib().cindm_ddpm1d_last_chain_info(self._handle(), info))
        return {"recovered": bool(info[0]), "exchange_free_up_front": bool(info[1]), "chains_in_flight": int(info[2]),
                "range_fallback": int(info[3])}

    def _chain(self, img, desc, call, result=None):
        """One library chain over ``img`` (in place): ``call(h, un, ws)`` issues it.  The FIRST chain after a weight synchronisation
        also carries the range rule on the caller's own data (TemporalUnet1D.range_guard): x_T is kept, the designs are
        checked once, and a chain that came back inf / nan from the split-fp16 kernels is repeated on the exact fp32-MFMA kernels.
        ``result``: the tensor the chain hands back, when that is not ``img`` (the autoregressive rollout's output; its ``call``
        draws every x_T itself and re-runs from the caller's condition) -- it is what is checked and returned."""
        device, B = img.device, img.shape[0]
        h, un, ws = self._prepare(desc, B, device)
        models = [self.model] + ([self.model_unconditioned] if un is not None else [])
        pend = [m for m in models if m.range_guard_pending()]
        x0 = img.clone() if pend else None
        call(h, un, ws)
        self._note_chain()

        def rerun():
            img.copy_(x0)
            call(*self._prepare(desc, B, device))        # (the fp32 plan sizes its own workspace)
            self._note_chain()
        res = img if result is None else result
        for m in pend:
            m.range_guard(lambda: res, rerun, device)
        return res

    def _note_chain(self):
        info = self.last_chain_info()
        if info["exchange_free_up_front"] and not GaussianDiffusion1D._warned_crowded:
            GaussianDiffusion1D._warned_crowded = True
            import warnings
            warnings.warn("cindm_amd: a sampling chain started while another was in flight on the same device; the fast kernels exchange "
                          "data between co-resident workgroups and are built for ONE chain per device, so this chain ran on the "
                          "exchange-free plan (correct, slower).  Run chains one after the other, or one process per GPU.", RuntimeWarning)
        return info

    def _recorder(self, every, trajectory, n, shape, device, **when):
        """The DeviceRecorder of a library chain of ``n`` steps over a state of ``shape`` [B, L, F], or None without the keyword."""
        if every is None:
            return None
        return DeviceRecorder(n, every, trajectory, shape[0] * shape[1] * shape[2], device, **when)

    @staticmethod
    def _arm(rec, h):
        """First thing a chain's ``call`` does: the chain call consumes the recorder, so every issue -- the range-rule re-run
        included -- arms it again."""
        if rec is not None:
            rec.arm(h)

    @staticmethod
    def _arm_tables(obj, h, img):
        """A WaypointObjective's, QuadraticObjective's, PairDistanceObjective's or SumObjective's tables, armed like the recorder: the guided chain call consumes them, so every
        issue arms again."""
        if obj is not None:
            obj.arm(h, img.shape[0], img.device)

    @staticmethod
    def _builtin(design_fn, design_guidance, B, L, n_bodies):
        """(descriptor, tables) when ``design_fn`` under ``design_guidance`` runs inside the captured step -- a PointObjective whose
        last_n_step fits the state, a WaypointObjective, a QuadraticObjective, a PairDistanceObjective or a SumObjective of these -- else (None, None).  A table objective whose tables
        do not fit the state [B, L, 4 * n_bodies] is a ValueError on every route, before any device work."""
        if isinstance(design_fn, (_TableObjective, SumObjective)):
            design_fn.check_state(B, L, n_bodies)
            dz = design_fn.descriptor(design_guidance)
            return dz, (design_fn if dz is not None else None)
        if isinstance(design_fn, PointObjective) and design_fn.last_n_step <= L:
            return design_fn.descriptor(design_guidance), None
        return None, None

    def _recorded(self, out, rec):
        """What a sampling call returns: the designs, or (designs, ChainRecord) when it recorded."""
        if rec is None:
            return out
        if isinstance(rec, LoopRecorder):
            return out, rec.result()
        shape = tuple(out.shape)
        return out, rec.collect(self._handle(), lambda rows: rows.reshape((rows.shape[0],) + shape))

    def last_step_info(self):
        """(kernel launches, update fused into the U-Net's last kernel?) of the reverse step emitted last -- as launched
        by the library, not a model of it (``cindm_ddpm1d_last_step_info``)."""
        n, f = C.c_int32(), C.c_int32()
        _ffi.check(_ffi.lib().cindm_ddpm1d_last_step_info(self._handle(), C.byref(n), C.byref(f)))
        return int(n.value), bool(f.value)

    @staticmethod
    def _f32(t, device=None):
        return None if t is None else t.detach().to(device=device or t.device, dtype=torch.float32).contiguous()

    # ------------------------------------------------------------------ replacement conditioning (known region)
    def _known_region(self, full, known, known_mask, cond, initial_state_overwrite, noise=None, rows=0, recur_iters=0, init=True):
        """The known region of a sampling call over the state ``full`` = (B, L, F) as (values fp32, mask bool), each [B, L, F] or --
        shared by all designs -- [L, F]; None without one.  Host checks only (ValueError), made before any device work: shapes,
        finite values on the region, rule 5 (no row also claimed by ``cond`` inpainting or ``initial_state_overwrite``) and the
        tape's known rows (``rows`` of them at least, ``recur_iters`` relaxation records per row for a guided chain)."""
        if known is None:
            if known_mask is not None:
                raise ValueError("known_mask without known")
            return None
        B, L, F = full
        if known_mask is None:
            raise ValueError(f"known needs known_mask (bool, broadcastable to [{B}, {L}, {F}])")
        if tuple(known.shape) not in ((B, L, F), (L, F)):
            raise ValueError(f"known must be [{B}, {L}, {F}] (per design) or [{L}, {F}] (shared by all designs), got {tuple(known.shape)}")
        if known_mask.dtype != torch.bool:
            raise ValueError("known_mask must be a bool tensor")
        if known_mask.dim() > 3:
            raise ValueError(f"known_mask {tuple(known_mask.shape)} does not broadcast to {(B, L, F)}")
        per_design = known_mask.dim() == 3 and known_mask.shape[0] != 1
        try:
            m = torch.broadcast_to(known_mask[0] if (known_mask.dim() == 3 and not per_design) else known_mask,
                                   (B, L, F) if per_design else (L, F)).contiguous()
        except RuntimeError as e:
            raise ValueError(f"known_mask {tuple(known_mask.shape)} does not broadcast to {(B, L, F)}") from e
        k = known.detach().to(torch.float32).contiguous()
        kb, mb = torch.broadcast_tensors(k, m.to(k.device))
        if not bool(torch.isfinite(kb[mb]).all()):
            raise ValueError("known holds non-finite values on the region")
        claimed = []
        if self.conditioned_steps == 0 and cond is not None:
            claimed.append(("cond (inpainting, conditioned_steps == 0)", cond.shape[1]))
        if initial_state_overwrite is not None:
            claimed.append(("initial_state_overwrite", initial_state_overwrite.shape[1]))
        for name, n in claimed:
            if bool(m[..., :n, :].any()):
                raise ValueError(f"the known region touches rows 0 .. {n - 1}, which {name} claims: name each row through one mechanism")
        if noise is not None:
            ok = noise.known_step is not None and noise.known_step.dim() == 4 and noise.known_step.shape[0] >= rows and \
                tuple(noise.known_step.shape[1:]) == (B, L, F)
            ok = ok and (not init or (noise.known_init is not None and tuple(noise.known_init.shape) == (B, L, F)))
            if recur_iters > 1:
                kr = noise.known_recur
                ok = ok and kr is not None and kr.dim() == 5 and kr.shape[0] >= rows and kr.shape[1] >= recur_iters and \
                    tuple(kr.shape[2:]) == (B, L, F)
            if not ok:
                raise ValueError(f"a noise tape used with a known region needs known_init [{B}, {L}, {F}], known_step [>= {rows}, {B}, {L}, {F}]"
                                 + (f" and known_recur [>= {rows}, >= {recur_iters}, {B}, {L}, {F}]" if recur_iters > 1 else ""))
        return k, m

    def known_replace(self, x, known, mask, level, z=None):
        """The definition of the known region in torch (what the library's known1d_kernel does inside the captured step,
        and what the routes that loop in Python call): ``x[m] = q(k, level, z)`` for ``level >= 0``, ``x[m] = k`` for ``level < 0``,
        with ``q = sqrt_alphas_cumprod[level] * k + sqrt_one_minus_alphas_cumprod[level] * z`` -- two products and a sum, three
        tensor operations.  x [B, L, F]; known and mask [B, L, F] or broadcastable to it; z [B, L, F] (None: ``torch.randn_like``).
        An empty mask returns x itself; otherwise a new tensor."""
        level = int(level)
        m = torch.broadcast_to(mask.to(x.device), x.shape)
        if not bool(m.any()):
            return x
        k = torch.broadcast_to(known.to(x.device, x.dtype), x.shape)
        if level < 0:
            q = k
        else:
            z = torch.randn_like(x) if z is None else z.to(x.device, x.dtype)
            a = self.sqrt_alphas_cumprod[level].to(x.device) * k
            b = self.sqrt_one_minus_alphas_cumprod[level].to(x.device) * z
            q = a + b
        return torch.where(m, q, x)

    def _known_z(self, full, row, word, seed, sample_offset, device):
        """The z of one overwrite on the routes that loop in Python: the tape's row when there is one, else the library's
        counter-based draw under the known region's seed word, keyed (sample_offset + b, ``word``, element) as known1d_kernel keys it."""
        if row is not None:
            return row
        z = torch.empty(full, dtype=torch.float32, device=device)
        with torch.cuda.device(device):
            _ffi.check(_ffi.lib().cindm_fill_normal(_ffi.ptr(z), full[0], full[1] * full[2], C.c_uint64((int(seed) ^ KNOWN_SEED) & (2 ** 64 - 1)),
                                                    sample_offset, int(word), _ffi.current_stream(device)))
        return z

    def _known_armer(self, kn, full, noise, device, init=True):
        """``arm(h)`` for a library chain with the region ``kn`` (None without one): every issue of the chain call arms the handle
        again (``cindm_ddpm1d_set_known1d``; the call consumes the region).  The device tensors live as long as the closure."""
        if kn is None:
            return None
        kd = kn[0].to(device)
        md = kn[1].to(device=device, dtype=torch.uint8).contiguous()
        zi = zs = zr = None
        if noise is not None:
            zi, zs, zr = noise.known_init, noise.known_step, noise.known_recur
        B, L, F = full

        def arm(h):
            _ffi.check(_ffi.lib().cindm_ddpm1d_set_known1d(
                h, _ffi.ptr(kd), int(kd.dim() == 3), _ffi.ptr(md), int(md.dim() == 3), _ffi.ptr(zi), _ffi.ptr(zs),
                0 if zs is None else zs[0].numel(), _ffi.ptr(zr), 0 if zr is None else zr[0].numel(), int(init), B, L, F))
        return arm

    @staticmethod
    def _arm_known(arm, h):
        if arm is not None:
            arm(h)

    # ------------------------------------------------------------------ reference-named helpers
    def predict_start_from_noise(self, x_t, t, noise):
        return self.sqrt_recip_alphas_cumprod[t].view(-1, 1, 1) * x_t - self.sqrt_recipm1_alphas_cumprod[t].view(-1, 1, 1) * noise

    def q_posterior(self, x_start, x_t, t):
        mean = self.posterior_mean_coef1[t].view(-1, 1, 1) * x_start + self.posterior_mean_coef2[t].view(-1, 1, 1) * x_t
        return mean, self.posterior_variance[t].view(-1, 1, 1), self.posterior_log_variance_clipped[t].view(-1, 1, 1)

    def q_sample(self, x_start, t, noise=None):
        """:2399-2406 (a two-table elementwise expression on the state; plumbing, not on the hot loop)."""
        if noise is None:
            noise = torch.randn_like(x_start)
        return self.sqrt_alphas_cumprod[t].view(-1, 1, 1) * x_start + self.sqrt_one_minus_alphas_cumprod[t].view(-1, 1, 1) * noise

    def _models(self, desc):
        return [self.model] + ([self.model_unconditioned] if desc.mode == _ffi.COMPOSE_MULTIBODY else [])

    def _timed_out(self, desc, device):
        """True when an in-kernel exchange of the U-Nets a step with ``desc`` runs timed out since the last poll (every
        model's flag is read and cleared); synchronises.  Raises instead when the model opted out of the recovery."""
        hit, opted_out = False, False
        for m in self._models(desc):                 # every model's flag is read (and cleared) before anything is raised
            rc = m.poll_raw(device)
            hit = hit or rc
            opted_out = opted_out or (rc and not m.recover_exchange_timeouts)
        if opted_out:
            raise _ffi.CindmError(self.model.TIMEOUT_TEXT)
        return hit

    def _rerun_exchange_free(self, fn, desc, device):
        """``fn()`` once more with the step's U-Nets on their exchange-free kernels (TemporalUnet1D.rerun_exchange_free for
        a step that may run two models)."""
        ms = self._models(desc)
        for m in ms:
            m.exchange_free(True)
        try:
            out = fn()
            if self._timed_out(desc, device):
                raise _ffi.CindmError(self.model.TIMEOUT_TEXT)
        finally:
            for m in ms:
                m.exchange_free(False)
        for m in ms:
            m.note_recovered()
        return out

    @torch.no_grad()
    def _predict(self, x, cond, t, desc, check=True):
        """(model_mean, x_start, pred_noise) = p_mean_variance(x, cond, t, ...) (:1033-1044) on the device.
        ``check``: read the U-Nets' exchange flags before returning (the Python loops pass False and check once at
        their end: the predictions of a step only feed the next one until then)."""
        if not x.is_cuda:
            raise _ffi.CindmError("sampling needs ROCm device tensors; there is no CPU execution path")
        x = self._f32(x)
        cond_d = self._f32(cond, x.device) if (cond is not None and self.conditioned_steps != 0) else None
        B = x.shape[0]
        h, un, ws = self._prepare(desc, B, x.device)
        mean, x0, eps = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)

        def launch():
            with torch.cuda.device(x.device):
                _ffi.check(_ffi.lib().cindm_ddpm1d_predict(h, self.model._h, un, C.byref(desc), _ffi.ptr(x), _ffi.ptr(cond_d),
                                                           int(t), None, B, _ffi.ptr(mean), _ffi.ptr(x0), _ffi.ptr(eps),
                                                           _ffi.ptr(ws), ws.numel(), _ffi.current_stream(x.device)))

        launch()
        if check and self._timed_out(desc, x.device):
            self._rerun_exchange_free(launch, desc, x.device)
        return mean, x0, eps

    def model_predictions(self, x, cond, t, x_self_cond=None, clip_x_start=False, rederive_pred_noise=False, **kwargs):
        """:951-1031.  Returns ModelPrediction(pred_noise, pred_x_start) (x_start unclamped unless clip_x_start)."""
        desc = self._desc_for(x.shape, kwargs.get("compose_mode"), kwargs.get("n_composed", 0),
                              kwargs.get("compose_start_step", 4), kwargs.get("single_model_step", -1),
                              kwargs.get("compose_n_bodies", 2), clip=clip_x_start)
        _, x0, eps = self._predict(x, cond, self._t_int(t), desc)
        return ModelPrediction(eps, x0)

    def p_mean_variance(self, x, cond, t, x_self_cond=None, clip_denoised=True, **kwargs):
        """:1033-1044.  Returns (model_mean, posterior_variance, posterior_log_variance, x_start, pred_noise)."""
        ti = self._t_int(t)
        desc = self._desc_for(x.shape, kwargs.get("compose_mode"), kwargs.get("n_composed", 0),
                              kwargs.get("compose_start_step", 4), kwargs.get("single_model_step", -1),
                              kwargs.get("compose_n_bodies", 2), clip=clip_denoised)
        mean, x0, eps = self._predict(x, cond, ti, desc)
        return mean, self.posterior_variance[ti].view(1, 1, 1), self.posterior_log_variance_clipped[ti].view(1, 1, 1), x0, eps

    @torch.no_grad()
    def gradient(self, x_t, t, n_bodies, scalar_for_gradient=None):
        """:1857-1982: pair + unconditioned composition of eps; for t > 400 the Langevin score -scalar_for_gradient[t] * eps (:1924 /
        :1980; ``scalar_for_gradient`` = ``schedule.ula_schedule(betas_inference)[0]``, required there as in the reference).  ``n_bodies == 4`` (:1865-1926): six pairs, the single-body
        predictions weighted by 1.4 -- what ``model_predictions`` calls (:1004).  ``n_bodies == 3`` (:1927-1982, reached only by a direct
        call): three pairs, weight 1; the reference slices its batched pair output with the literal bounds 0:20 / 20:40 / 40:60, so its
        branch is defined for a batch of 20 only -- here any batch gives what batch 20 gives there (golden at 20:
        tests/golden/gradient3_1d_r6.npz)."""
        if n_bodies not in (3, 4) or self.model_unconditioned is None:
            raise NotImplementedError("gradient(): n_bodies must be 3 or 4, with model_unconditioned set")
        if x_t.shape[-1] != 4 * n_bodies:
            raise ValueError(f"gradient(): x_t has {x_t.shape[-1]} features, n_bodies = {n_bodies} needs {4 * n_bodies}")
        ti = self._t_int(t)
        if ti > 400 and scalar_for_gradient is None:
            raise NotImplementedError("gradient(): t > 400 dereferences scalar_for_gradient (unreachable for N <= 401): pass "
                                      "scalar_for_gradient (schedule.ula_schedule(betas_inference)[0]), as sample_step_ULA does")
        desc = self._compose_desc(_ffi.COMPOSE_MULTIBODY, 0, 0, self.model.horizon, n_bodies, clip=False,
                                  uncond_coef=1.4 if n_bodies == 4 else 1.0)
        desc.cond_steps = 0                             # x_t here already is cat(cond, x)
        _, _, eps = self._predict(x_t, None, ti, desc)
        if ti > 400:                                    # (-1 * scalar[t]) * eps: the zero-dim factor is rounded to fp32 once
            return eps * (-float(torch.as_tensor(scalar_for_gradient)[ti].to(torch.float32)))
        return eps

    # ------------------------------------------------------------------ one reverse step
    def _design_shift(self, design_fn, design_guidance, x, x_start, t):
        """Gradient term of the guided step (:1072-1106 / :1235-1269 / :1468-1512), PyTorch autograd on the
        user's callable."""
        eta = self.betas[t] / torch.sqrt(self.alphas_cumprod_prev)[t]
        g = design_guidance

        def grad_of(z):
            with torch.enable_grad():
                zc = z.clone().detach().requires_grad_()
                return torch.autograd.grad(design_fn(zc), zc)[0]

        if g.startswith("standard"):
            gd = grad_of(x)
            if g == "standard" or g.startswith("standard-recurrence"):
                return gd
            if g == "standard-alpha" or g.startswith("standard-alpha-recurrence"):
                return eta * gd
            raise ValueError(g)
        if g.startswith("universal-forward"):
            gd = grad_of(x_start)
            return gd if "pure" in g else eta * gd
        if g.startswith("universal-backward"):
            xc, final = x_start.clone(), None
            for kk in range(self.backward_steps):
                gd = grad_of(xc)
                if kk == 1:
                    final = gd if "pure" in g else eta * gd
                xc = xc - gd * self.backward_lr
            coef = (self.sqrt_alphas_cumprod * self.betas / (torch.sqrt(1 - self.betas) * (1 - self.alphas_cumprod)))[t]
            return final - coef * (xc - x_start)
        raise ValueError(g)

    @torch.no_grad()
    def _guided_step(self, x, cond, t, desc, design_fn, design_guidance, initial_state_overwrite, noise, recur_noise,
                     ddim_return=False, check=True, after_relax=None):
        """Shared body of p_sample / p_sample_compose_inside / p_sample_compose_outside.  ``ddim_return``: the
        sampling_timesteps != timesteps convention of the recurrence branch (:1372-1376): returns
        (pred_noise + grad_design_final, x_start) of the last iteration.  ``after_relax(r, x)``: what a known region does to the
        state after relaxation r (all but the last iteration, whose relaxed state is never used)."""
        R = int(design_guidance.split("-")[-1]) if "recurrence" in design_guidance else 0
        x = self._f32(x)
        logvar = self.posterior_log_variance_clipped[t]
        x_start = None
        eps = shift = None
        for r in range(max(R, 1)):
            mean, x_start, eps = self._predict(x, cond, t, desc, check=check)
            pred = mean
            if design_fn is not None:
                shift = self._design_shift(design_fn, design_guidance, x, x_start, t)
                pred = mean - shift
            if initial_state_overwrite is not None:
                k = initial_state_overwrite.shape[1]
                pred = torch.cat([initial_state_overwrite.to(pred), pred[:, k:]], 1)
            if R:
                ratio = self.alphas_cumprod / self.alphas_cumprod_prev
                z = recur_noise[r] if recur_noise is not None else torch.randn_like(pred)
                x = torch.sqrt(ratio)[t] * pred + torch.sqrt(1 - ratio)[t] * z
                if after_relax is not None and r < max(R, 1) - 1:
                    x = after_relax(r, x)
        if ddim_return:
            return eps + shift, x_start
        if t > 0:
            z = noise if noise is not None else torch.randn_like(x)
            pred = pred + (0.5 * logvar).exp() * z
        return pred, x_start

    @torch.no_grad()
    def p_sample(self, x, cond, t: int, x_self_cond=None, clip_denoised=True, design_fn=None,
                 design_guidance="standard", initial_state_overwrite=None, *, noise=None, recur_noise=None):
        """:1047-1186.  Returns (x_{t-1}, x_start)."""
        desc = self._desc_for(x.shape, None, clip=clip_denoised)
        return self._guided_step(x, cond, int(t), desc, design_fn, design_guidance, initial_state_overwrite, noise, recur_noise)

    @torch.no_grad()
    def p_sample_compose_inside(self, x, cond, t: int, x_self_cond=None, clip_denoised=True, design_fn=None,
                                design_guidance="standard", initial_state_overwrite=None, compose_mode="mean-inside",
                                n_composed=0, compose_start_step=4, single_model_step=-1, compose_n_bodies=2,
                                *, noise=None, recur_noise=None):
        """:1190-1376."""
        ddim = self.sampling_timesteps != self.num_timesteps and "recurrence" in design_guidance     # :1372-1376
        assert "inside" not in compose_mode or single_model_step > 0
        desc = self._desc_for(x.shape, compose_mode, n_composed, compose_start_step, single_model_step, compose_n_bodies,
                              clip=clip_denoised)
        return self._guided_step(x, cond, int(t), desc, design_fn, design_guidance, initial_state_overwrite, noise, recur_noise,
                                 ddim_return=ddim)

    @torch.no_grad()
    def p_sample_compose_outside(self, x, cond, t: int, x_self_cond=None, clip_denoised=True, design_fn=None,
                                 design_guidance="standard", compose_mode="mean", n_composed=0, compose_start_step=4,
                                 single_model_step=-1, compose_n_bodies=2, initial_state_overwrite=None,
                                 *, noise=None, recur_noise=None):
        """:1380-1652."""
        assert single_model_step > 0
        desc = self._desc_for(x.shape, compose_mode, n_composed, compose_start_step, single_model_step, compose_n_bodies,
                              clip=clip_denoised, outside=True)
        return self._guided_step(x, cond, int(t), desc, design_fn, design_guidance, initial_state_overwrite, noise, recur_noise)

    # ------------------------------------------------------------------ loops
    @torch.no_grad()
    def _run_loop(self, img, cond, desc, t_start, t_end, *, noise_steps, seed, sample_offset, inpaint_cond,
                  inpaint_noise_steps, use_graph=True, rec=None, karm=None):
        """The unguided reverse loop as one library call (cindm_ddpm1d_sample).  ``karm``: the known region's ``arm(h)`` or None."""
        B = img.shape[0]
        cond_d = self._f32(cond, img.device) if (cond is not None and self.conditioned_steps != 0) else None
        inp = self._f32(inpaint_cond, img.device)

        def call(h, un, ws):
            self._arm(rec, h)
            self._arm_known(karm, h)
            with torch.cuda.device(img.device):
                _ffi.check(_ffi.lib().cindm_ddpm1d_sample(
                    h, self.model._h, un, C.byref(desc), _ffi.ptr(img), _ffi.ptr(cond_d), _ffi.ptr(noise_steps),
                    C.c_uint64(seed), sample_offset, _ffi.ptr(inp), 0 if inp is None else inp.shape[1],
                    _ffi.ptr(inpaint_noise_steps), t_start, t_end, B, _ffi.ptr(ws), ws.numel(),
                    _ffi.current_stream(img.device), int(use_graph)))
        return self._chain(img, desc, call)

    @torch.no_grad()
    def _run_guided_loop(self, img, cond, desc, dz, t_start, t_end, *, noise, seed, sample_offset, inpaint_cond,
                         initial_state_overwrite, use_graph=True, rec=None, tables=None, karm=None):
        """Reverse steps t_start .. t_end guided by the built-in objective as one library call
        (cindm_ddpm1d_sample_guided); ``noise`` rows (step / recur / cond) are indexed by t.  ``tables``: the WaypointObjective,
        QuadraticObjective or PairDistanceObjective whose descriptor ``dz`` is (modes 3 / 4, 5, 6): every issue of the call arms its tables."""
        device, B = img.device, img.shape[0]
        cond_d = self._f32(cond, device) if (cond is not None and self.conditioned_steps != 0) else None
        inp = self._f32(inpaint_cond, device)
        iso = self._f32(initial_state_overwrite, device)

        def call(h, un, ws):
            self._arm(rec, h)
            self._arm_tables(tables, h, img)
            self._arm_known(karm, h)
            with torch.cuda.device(device):
                _ffi.check(_ffi.lib().cindm_ddpm1d_sample_guided(
                    h, self.model._h, un, C.byref(desc), C.byref(dz), _ffi.ptr(img), _ffi.ptr(cond_d),
                    _ffi.ptr(None if noise is None else noise.step), _ffi.ptr(None if noise is None else noise.recur),
                    C.c_uint64(seed), sample_offset, _ffi.ptr(inp), 0 if inp is None else inp.shape[1],
                    _ffi.ptr(None if noise is None else noise.cond), _ffi.ptr(iso), 0 if iso is None else iso.shape[1],
                    int(t_start), int(t_end), B, _ffi.ptr(ws), ws.numel(), _ffi.current_stream(device), int(use_graph)))
        return self._chain(img, desc, call)

    @torch.no_grad()
    def _run_guided_ddim(self, img, cond, desc, dz, times, coefs, *, noise, seed, sample_offset, inpaint_cond,
                         initial_state_overwrite, use_graph=True, rec=None, tables=None, karm=None, ms=None):
        """DDIM steps ``times[0] .. times[-2]`` guided by the built-in objective as one library call
        (cindm_ddpm1d_sample_ddim_guided); ``noise`` rows (step / recur / cond) are indexed by the position in ``times``.
        ``tables``: as _run_guided_loop."""
        device, B = img.device, img.shape[0]
        S = len(times) - 1
        cond_d = self._f32(cond, device) if (cond is not None and self.conditioned_steps != 0) else None
        inp = self._f32(inpaint_cond, device)
        iso = self._f32(initial_state_overwrite, device)
        tarr = (C.c_int32 * (S + 1))(*times)
        carr = coefs.contiguous()

        def call(h, un, ws):
            self._arm(rec, h)
            self._arm_tables(tables, h, img)
            self._arm_known(karm, h)
            self._arm_multistep(ms, h)
            with torch.cuda.device(device):
                _ffi.check(_ffi.lib().cindm_ddpm1d_sample_ddim_guided(
                    h, self.model._h, un, C.byref(desc), C.byref(dz), _ffi.ptr(img), _ffi.ptr(cond_d), S, tarr, _ffi.ptr(carr),
                    _ffi.ptr(None if noise is None else noise.step), _ffi.ptr(None if noise is None else noise.recur),
                    C.c_uint64(seed), sample_offset, _ffi.ptr(inp), 0 if inp is None else inp.shape[1],
                    _ffi.ptr(None if noise is None else noise.cond), _ffi.ptr(iso), 0 if iso is None else iso.shape[1],
                    B, _ffi.ptr(ws), ws.numel(), _ffi.current_stream(device), int(use_graph)))
        return self._chain(img, desc, call)

    def _init_state(self, shape, device, noise, seed, sample_offset, tag):
        if noise is not None:
            return self._f32(noise.init, device).clone()
        img = torch.empty(shape, dtype=torch.float32, device=device)
        with torch.cuda.device(device):
            _ffi.check(_ffi.lib().cindm_fill_normal(_ffi.ptr(img), shape[0], shape[1] * shape[2], C.c_uint64(seed),
                                                    sample_offset, tag, _ffi.current_stream(device)))
        return img

    @staticmethod
    def _draw_seed():
        return int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item())

    @torch.no_grad()
    def p_sample_loop(self, shape, cond, n_composed=0, compose_start_step=4, compose_n_bodies=2, compose_mode="mean",
                      design_fn=None, design_guidance="standard", initial_state_overwrite=None, initialization_mode=0,
                      initialization_img=None, *, noise=None, seed=None, sample_offset=0, use_graph=True, t_stop=0,
                      return_trajectory_every=None, trajectory=("x",), known=None, known_mask=None, solver="ddim"):
        """:1656-1720.  Build-only keywords: ``noise`` (NoiseTape, explicit draws), ``seed`` /
        ``sample_offset`` (counter-based generator keyed by global sample index), ``t_stop`` (truncate),
        ``return_trajectory_every=k`` with ``trajectory=("x",)`` / ``("x", "x0")``: returns (designs, ChainRecord) with the state after
        every k-th step and after the last one (record.py; recorded inside the captured step on the library routes).
        Replacement conditioning (build-only): ``known`` [B, L_tot, F] or [L_tot, F] (shared by all designs) with
        ``known_mask`` (bool, broadcastable to the state) names a region of the returned state and its clean values k.  With
        q(k, l, z) = sqrt_alphas_cumprod[l] k + sqrt_one_minus_alphas_cumprod[l] z the region is set to q(k, T - 1, z_init) before the
        first step, to q(k, t, z) after every relaxation iteration of a guided step at t, and to q(k, t - 1, z) after the step (k
        itself after t = 0), so it comes back exactly; z per element from the tape's ``known_init`` / ``known_step[t]`` /
        ``known_recur[t][r]``, else counter-based under a seed word of its own.  The region overwrites last and may not touch rows
        that ``cond`` inpainting or ``initial_state_overwrite`` claim (ValueError).  Inside the captured step on the library routes
        (known1d_kernel), ``known_replace`` on the route that loops in Python; a recorder's x stream is taken after the overwrite.
        ``solver``: "ddim" (nothing changes); "dpmpp-2m" is a ValueError here -- this is the DDPM chain (see ddim_sample)."""
        if check_solver(self, solver):
            raise ValueError("solver='dpmpp-2m' runs on the DDIM chains: p_sample_loop is the DDPM chain (sample() with "
                             "sampling_timesteps < timesteps, or ddim_sample)")
        full = (shape[0], shape[1] + n_composed * compose_start_step, compose_n_bodies * 4)
        fast = design_fn is None and "recurrence" not in design_guidance and initial_state_overwrite is None
        iters = max(int(design_guidance.split("-")[-1]) if "recurrence" in design_guidance else 0, 1)
        kn = self._known_region(full, known, known_mask, cond, initial_state_overwrite, noise, self.num_timesteps, 0 if fast else iters)
        device = self.betas.device
        if device.type != "cuda":
            raise _ffi.CindmError("GaussianDiffusion1D is on the CPU: move it to a ROCm device; there is no CPU execution path")
        if seed is None and noise is None:
            seed = self._draw_seed()
        seed = 0 if seed is None else int(seed)
        if noise is not None:
            noise = noise.to(device)
        B, T1 = shape[0], shape[1]
        assert compose_start_step < T1
        dz, tables = self._builtin(design_fn, design_guidance, B, full[1], compose_n_bodies)
        karm = self._known_armer(kn, full, noise, device)
        init = self._init_state(full, device, noise, seed, sample_offset, self.num_timesteps)
        if initialization_mode == 0:
            img = init
        elif initialization_mode == 1:
            img = self._f32(initialization_img, device).reshape(full).clone()
        else:
            img = self._f32(initialization_img, device).reshape(full) + init
        inside = "inside" in compose_mode
        desc = self._desc_for(full, compose_mode, n_composed, compose_start_step, T1, compose_n_bodies, outside=not inside)
        inpaint = cond if (self.conditioned_steps == 0 and cond is not None) else None
        t_first, n_steps = self.num_timesteps - 1, self.num_timesteps - int(t_stop)
        # (the device record buffer is allocated only on the routes that are library chains)
        device_rec = lambda: self._recorder(return_trajectory_every, trajectory, n_steps, full, device, t_start=t_first)
        if dz is not None:
            # built-in objective: the guided loop (gradient, overwrite, relaxations) stays inside the captured step
            rec = device_rec()
            return self._recorded(self._run_guided_loop(img, cond, desc, dz, t_first, t_stop, noise=noise, seed=seed,
                                                        sample_offset=sample_offset, inpaint_cond=inpaint,
                                                        initial_state_overwrite=initial_state_overwrite, use_graph=use_graph,
                                                        rec=rec, tables=tables, karm=karm), rec)
        if fast:
            rec = device_rec()
            return self._recorded(self._run_loop(img, cond, desc, t_first, t_stop,
                                                 noise_steps=None if noise is None else noise.step, seed=seed,
                                                 sample_offset=sample_offset, inpaint_cond=inpaint,
                                                 inpaint_noise_steps=None if noise is None else noise.cond,
                                                 use_graph=use_graph, rec=rec, karm=karm), rec)
        img_T = img
        # this route loops in Python: the same record, cloned per step
        rec = None if return_trajectory_every is None else LoopRecorder(n_steps, return_trajectory_every, trajectory, t_start=t_first)

        kz = lambda row, word: self._known_z(full, row, word, seed, sample_offset, device)

        def chain():
            # (the steps' predictions only feed the next step: the exchange flags are read once, after the last one)
            img = img_T
            if rec is not None:
                rec.reset()
            if kn is not None:      # rule 1
                img = self.known_replace(img, kn[0], kn[1], t_first, kz(None if noise is None else noise.known_init, self.num_timesteps))
            for i, t in enumerate(reversed(range(t_stop, self.num_timesteps))):
                nz = None if noise is None else noise.step[t]
                rn = None if (noise is None or noise.recur is None) else noise.recur[t]
                relaxed = {} if kn is None else dict(after_relax=lambda r, x, t=t: self.known_replace(
                    x, kn[0], kn[1], t, kz(None if noise is None else noise.known_recur[t][r], t + 0x10000 * (r + 1))))
                img, x_start = self._guided_step(img, cond, t, desc, design_fn, design_guidance, initial_state_overwrite, nz, rn,
                                                 check=False, **relaxed)
                if inpaint is not None:
                    zc = noise.cond[t] if (noise is not None and noise.cond is not None) else torch.randn_like(inpaint)
                    img[:, :inpaint.shape[1], :] = self.q_sample(self._f32(inpaint, device), t, zc)
                if kn is not None:      # the region overwrites last, at the level the step has reached
                    img = self.known_replace(img, kn[0], kn[1], t - 1,
                                             None if t == 0 else kz(None if noise is None else noise.known_step[t], t - 1))
                if rec is not None:
                    rec.after(i, img, x_start)
            return img

        img = chain()
        if self._timed_out(desc, device):
            img = self._rerun_exchange_free(chain, desc, device)
        return self._recorded(img, rec)

    @torch.no_grad()
    def sample(self, batch_size=16, cond=None, is_composing_time=False, n_composed=2, compose_start_step=4,
               compose_n_bodies=2, compose_mode="mean", design_fn=None, design_guidance="standard",
               initial_state_overwrite=None, initialization_mode=0, initialization_img=None, **build_kw):
        """:2330-2376.  ``build_kw``: noise=, seed=, sample_offset=, use_graph=, t_stop=, return_trajectory_every=, trajectory=,
        known=, known_mask= (see p_sample_loop; the known region is held by the DDPM and the DDIM route alike), solver= ("ddim" |
        "dpmpp-2m", see ddim_sample)."""
        check_solver(self, build_kw.get("solver", "ddim"))
        self.is_ddim_sampling = self.sampling_timesteps < self.num_timesteps
        if self.is_ddim_sampling:               # :2348-2363
            build_kw.pop("t_stop", None)
            return self.ddim_sample((batch_size, self.image_size, self.channels), cond=cond, n_composed=n_composed,
                                    compose_start_step=compose_start_step, compose_n_bodies=compose_n_bodies,
                                    compose_mode=compose_mode, design_fn=design_fn, design_guidance=design_guidance,
                                    initial_state_overwrite=initial_state_overwrite,
                                    initialization_mode=initialization_mode, initialization_img=initialization_img,
                                    **build_kw)
        return self.p_sample_loop((batch_size, self.image_size, self.channels), cond=cond, n_composed=n_composed,
                                  compose_start_step=compose_start_step, compose_n_bodies=compose_n_bodies,
                                  compose_mode=compose_mode, design_fn=design_fn, design_guidance=design_guidance,
                                  initial_state_overwrite=initial_state_overwrite,
                                  initialization_mode=initialization_mode, initialization_img=initialization_img,
                                  **build_kw)

    # ------------------------------------------------------------------ Langevin (ULA) phase
    def _ula_refusals(self, N, L, n_bodies):
        """What the Langevin phase cannot run, with the reason (before any device work)."""
        if n_bodies != 4:
            raise NotImplementedError(f"the Langevin phase with n_bodies = {n_bodies}: p_sample calls gradient(x, t, 4) whatever was passed "
                                      "(model/diffusion_1d.py:1004), so only n_bodies = 4 can finish in the reference either")
        if self.model_unconditioned is None:
            raise NotImplementedError("the Langevin phase needs model_unconditioned: its score is gradient()'s pair + single-body composition")
        if self.objective != "pred_noise":
            raise NotImplementedError(f"the Langevin phase with objective {self.objective!r}: its score is the composed noise prediction")
        if int(L) < 0:
            raise ValueError(f"L (Langevin iterations per timestep) must be >= 0, got {L}")
        if int(N) > self.num_timesteps:
            raise ValueError(f"N = {N} > num_timesteps = {self.num_timesteps}: the U-Net has no timestep {int(N) - 1}")
        bi = self.betas_inference
        if bi is None:
            raise ValueError("the Langevin phase (N > 401) needs betas_inference (the script passes linear_beta_schedule(N)): it is None")
        if len(bi) < int(N):
            raise ValueError(f"betas_inference has {len(bi)} entries, shorter than N = {N}: the Langevin phase indexes it by the timestep")

    @torch.no_grad()
    def _run_ula(self, x, t_hi, t_lo, L, *, scalar=None, tape=None, seed=0, sample_offset=0, use_graph=True):
        """Langevin iterations for t = t_hi .. t_lo, L per timestep, in place on the whole state x [B, Lc + R, 16] as one library
        chain (cindm_ddpm1d_sample_ula).  ``scalar``: gradient()'s factor table indexed by t (default: from betas_inference);
        ``tape`` [n_t, L, B, Lc + R, 16] explicit draws in processing order."""
        device, B = x.device, x.shape[0]
        if tuple(x.shape[1:]) != (self.conditioned_steps + self.rollout_steps, 16) or not x.is_contiguous():
            raise ValueError(f"the Langevin state must be a contiguous [B, {self.conditioned_steps + self.rollout_steps}, 16] tensor "
                             f"(cat(cond, x) of 4 bodies), got {tuple(x.shape)}")
        n_t = t_hi - t_lo + 1
        if L == 0 or n_t <= 0:
            return x
        sc, ss, sd = ula_schedule(self.betas_inference)
        if scalar is not None:
            sc = torch.as_tensor(scalar).detach().to("cpu", torch.float32)
        idx = torch.arange(t_hi, t_lo - 1, -1)
        sc, ss, sd = sc[idx].contiguous(), ss[idx].contiguous(), sd[idx].contiguous()
        if tape is not None:
            if tape.dim() != 5 or tape.shape[0] < n_t or tuple(tape.shape[1:]) != (L,) + tuple(x.shape):
                raise ValueError(f"Langevin noise must be [>= {n_t}, {L}, {B}, {x.shape[1]}, 16] (timestep-major, first timestep first), "
                                 f"got {tuple(tape.shape)}")
            tape = self._f32(tape, device)[:n_t].contiguous()
        desc = self._compose_desc(_ffi.COMPOSE_MULTIBODY, 0, 0, self.model.horizon, 4, clip=False, uncond_coef=1.4)
        desc.cond_steps = 0                             # the conditioning rows are rows of the state here
        tab = torch.empty(n_t * 16, dtype=torch.uint8, device=device)

        def call(h, un, ws):
            with torch.cuda.device(device):
                _ffi.check(_ffi.lib().cindm_ddpm1d_sample_ula(
                    h, self.model._h, un, C.byref(desc), _ffi.ptr(x), int(t_hi), int(t_lo), int(L), _ffi.ptr(sc), _ffi.ptr(ss),
                    _ffi.ptr(sd), _ffi.ptr(tab), tab.numel(), _ffi.ptr(tape), C.c_uint64(seed), sample_offset, B,
                    _ffi.ptr(ws), ws.numel(), _ffi.current_stream(device), int(use_graph)))
        return self._chain(x, desc, call)

    @torch.no_grad()
    def sample_step_ULA(self, x, ts, num_samples_per_step, n_bodies, N, scalar_for_gradient, *, noise=None, seed=None,
                        sample_offset=0, use_graph=True):
        """:2048-2073: ``num_samples_per_step`` Langevin iterations at timestep ts[0] on the whole state x [B, Lc + R, 16]:
        x <- x + gradient(x, t, n_bodies, scalar_for_gradient) * ss_t + randn_like(x) * std_t with ss = betas_inference * 0.035,
        std = (2 ss) ** .5.  Returns the new state (x is not modified).  The one-timestep form of the library's Langevin chain.
        gradient() scales the composed eps by -scalar_for_gradient[t] for t > 400 only (:1923-1926); at t <= 400 it returns eps
        itself, so the update ADDS eps * ss_t.  The library's update always multiplies by the negated table entry: for t <= 400 it
        is handed -1.0 in place of scalar_for_gradient[t], the factor is +1 and the product exact.  (The chain of
        ``sample_compose_multibodies`` stops at t = 401 and never takes this branch.)
        Build-only keywords: ``noise`` [num_samples_per_step, B, Lc + R, 16] explicit draws, ``seed`` / ``sample_offset``
        (counter-based draws keyed by (seed, sample_offset + b, t, l)), ``use_graph``."""
        t = self._t_int(ts)
        L = int(num_samples_per_step)
        self._ula_refusals(t + 1, L, n_bodies)
        if scalar_for_gradient is None or len(scalar_for_gradient) <= t:
            raise ValueError(f"scalar_for_gradient must cover timestep {t}")
        if not x.is_cuda:
            raise _ffi.CindmError("sampling needs ROCm device tensors; there is no CPU execution path")
        if seed is None and noise is None:
            seed = self._draw_seed()
        out = self._f32(x).clone()
        tape = None if noise is None else noise.reshape((1,) + tuple(noise.shape))
        scalar = torch.as_tensor(scalar_for_gradient).detach().to("cpu", torch.float32)
        if t <= 400:                                    # :1923-1926: the unscaled eps; -(-1.0) * eps is eps bit for bit
            scalar = torch.full_like(scalar, -1.0)
        return self._run_ula(out, t, t, L, scalar=scalar, tape=tape, seed=0 if seed is None else int(seed),
                             sample_offset=sample_offset, use_graph=use_graph)

    @torch.no_grad()
    def sample_compose_multibodies(self, cond, N, L, n_bodies, *, noise=None, seed=None, sample_offset=0,
                                   use_graph=True, t_stop=0, full_state=False, return_trajectory_every=None, trajectory=("x",),
                                   solver="ddim"):
        """:1986-2042: x = cat(cond, noise); for i = N-1 .. 401: L Langevin iterations on the whole x (``sample_step_ULA``, the
        conditioning rows drift too); for i = 400 .. 0: x[:, cs:] = p_sample(x[:, cs:], x[:, :cs], i).  Returns
        [B, rollout_steps, 4*n_bodies].  N <= 401 has no Langevin phase (L and n_bodies are not looked at, as before).
        Build-only keywords: ``noise`` (NoiseTape; ``ula`` feeds the Langevin draws), ``seed`` / ``sample_offset``, ``use_graph``,
        ``t_stop`` (truncate; > 400 stops inside the Langevin phase, after timestep t_stop), ``full_state`` (return the whole
        [B, conditioned_steps + rollout_steps, F] state, drifted conditioning rows first), ``return_trajectory_every`` /
        ``trajectory`` (N <= 401 only; the records hold the [B, rollout_steps, F] state; see p_sample_loop)."""
        if check_solver(self, solver):
            raise NotImplementedError("solver='dpmpp-2m': sample_compose_multibodies is a Langevin phase followed by DDPM steps; the "
                                      "multistep solver runs on the DDIM chains")
        ula = N > 401
        if ula and return_trajectory_every is not None:
            raise NotImplementedError("return_trajectory_every with N > 401: the Langevin chain's step index is (timestep, inner iteration) "
                                      "and the library does not record it")
        if ula:
            self._ula_refusals(N, L, n_bodies)
        if not cond.is_cuda:
            raise _ffi.CindmError("sampling needs ROCm device tensors; there is no CPU execution path")
        device = cond.device
        if seed is None and noise is None:
            seed = self._draw_seed()
        seed = 0 if seed is None else int(seed)
        if noise is not None:
            noise = noise.to(device)
        B = cond.shape[0]
        shape = (B, self.rollout_steps, cond.shape[2])
        img = self._init_state(shape, device, noise, seed, sample_offset, self.num_timesteps)
        desc = self._desc_for(shape, None)
        t_first, cs = N - 1, self.conditioned_steps
        if ula:
            L = int(L)
            if noise is not None and noise.ula is None and L > 0:
                raise ValueError("noise.ula is required with N > 401 and L > 0 (the Langevin draws, [n_t, L, B, Lc + R, F])")
            x = torch.cat([self._f32(cond, device), img], dim=1).contiguous()
            self._run_ula(x, N - 1, max(401, t_stop), L, tape=None if noise is None else noise.ula, seed=seed,
                          sample_offset=sample_offset, use_graph=use_graph)
            if t_stop > 400:
                return x if full_state else x[:, cs:].contiguous()
            # the DDPM phase is conditioned on the DRIFTED rows, not on the caller's cond (:2033)
            img, cond, t_first = x[:, cs:].contiguous(), x[:, :cs].contiguous(), 400
        rec = self._recorder(return_trajectory_every, trajectory, t_first - int(t_stop) + 1, shape, device, t_start=t_first)
        out = self._run_loop(img, cond, desc, t_first, t_stop, noise_steps=None if noise is None else noise.step,
                             seed=seed, sample_offset=sample_offset, inpaint_cond=None, inpaint_noise_steps=None,
                             use_graph=use_graph, rec=rec)
        record = None if rec is None else self._recorded(out, rec)[1]
        out = torch.cat([self._f32(cond, device), out], dim=1) if full_state else out
        return out if rec is None else (out, record)

    # ------------------------------------------------------------------ out of scope
    def forward(self, *a, **k):
        raise NotImplementedError("training loss (p_losses, :2438-2501) is out of this build's scope")

    # ------------------------------------------------------------------ DDIM
    @torch.no_grad()
    def ddim_sample(self, shape, cond, n_composed=None, clip_denoised=True, compose_start_step=4, compose_n_bodies=2,
                    compose_mode="mean", design_fn=None, design_guidance="standard", initial_state_overwrite=None,
                    initialization_mode=0, initialization_img=None, *, noise=None, seed=None, sample_offset=0,
                    use_graph=True, init_img=None, step_range=None, return_trajectory_every=None, trajectory=("x",),
                    known=None, known_mask=None, solver="ddim", history=None):
        """:1724-1804.  Build-only keywords: ``init_img`` + ``step_range=(i0, i1)`` run DDIM steps i0 .. i1-1 from a given
        state (teacher-forced segments for parity tests: the deterministic sampler amplifies a 1e-6 perturbation of the
        U-Net to 1e-3 .. 1e-2 over 50 .. 250 steps with random-init weights -- measured on the CPU reference itself).
        ``noise``: a NoiseTape whose ``step`` / ``recur`` / ``cond`` rows are indexed by the DDIM STEP index.
        Without ``design_fn`` the whole loop is one library call (``cindm_ddpm1d_sample_ddim``); as in the reference the
        prediction then ignores the compose keywords (:1755).  With ``design_fn`` (recurrence guidance only -- the
        reference's non-recurrence branch does not return a noise prediction, :1283) the prediction honours them.  A
        ``PointObjective`` (last_n_step <= L), ``WaypointObjective``, ``QuadraticObjective`` or ``PairDistanceObjective`` under "standard" / "standard-alpha" ``-recurrence-N`` (N >= 1) runs as one library
        chain (``cindm_ddpm1d_sample_ddim_guided``; counter-based draws keyed by (seed, sample_offset + b, t, element) when there
        is no tape); any other callable or guidance: each step is ``recurrence`` library predictions + the user's autograd
        gradient, and the DDIM update of the tiny state runs in torch.
        ``return_trajectory_every`` / ``trajectory``: as p_sample_loop; steps are counted from the first step this call runs.
        ``known`` / ``known_mask``: replacement conditioning as p_sample_loop -- q(k, times[0], z_init) before the first step (skipped
        with ``init_img``, whose caller hands over a state that is already at its level, so that teacher-forced segments chain
        exactly), q(k, t, z) after every relaxation iteration, q(k, times[i + 1], z) after step i, k itself after the last pair; the
        tape's ``known_step`` / ``known_recur`` rows are indexed by the DDIM step.
        ``solver="dpmpp-2m"`` (build-only): the second-order multistep solver on the same grid at no extra U-Net
        evaluation -- step i adds ``multistep_kappa()[i] * (x_start_i - x_start_{i-1})`` to its DDIM value (each operation rounded
        once) ahead of the inpainting overwrite, the known region and the recorder; the first step and the last pair are plain DDIM
        steps.  Inside the captured step on the library routes, in torch on the route that loops in Python.  Needs
        ``ddim_sampling_eta == 0`` and ``sampling_timesteps < timesteps`` (ValueError).  With ``step_range=(i0, i1)`` the call
        takes ``history=`` (the x_start of step i0 - 1: required when i0 > 0) and returns (result, history of step i1 - 1)."""
        ms_on = self._check_solver(solver, step_range, history)
        n_pairs = len(self.ddim_schedule()[0]) - 1
        iters = max(int(design_guidance.split("-")[-1]) if "recurrence" in design_guidance else 0, 1)
        kn = self._known_region(tuple(shape), known, known_mask, cond, initial_state_overwrite, noise,
                                n_pairs if step_range is None else int(step_range[1]), 0 if design_fn is None else iters,
                                init=init_img is None)
        device = self.betas.device
        if device.type != "cuda":
            raise _ffi.CindmError("GaussianDiffusion1D is on the CPU: move it to a ROCm device; there is no CPU execution path")
        if seed is None and noise is None:
            seed = self._draw_seed()
        seed = 0 if seed is None else int(seed)
        if noise is not None:
            noise = noise.to(device)
        B = shape[0]
        dz, tables = self._builtin(design_fn, design_guidance, B, shape[1], compose_n_bodies)
        if init_img is not None:
            img = self._f32(init_img, device).clone()
        else:
            img = self._init_state(tuple(shape), device, noise, seed, sample_offset, self.num_timesteps)
        times, coefs = self.ddim_schedule()
        i0, i1 = (0, len(times) - 1) if step_range is None else step_range
        times, coefs = times[i0:i1 + 1], coefs[i0:i1].contiguous()
        if noise is not None:
            sl = lambda v: None if v is None else v[i0:i1].contiguous()
            noise = NoiseTape(noise.init, sl(noise.step), sl(noise.recur), sl(noise.cond), known_init=noise.known_init,
                              known_step=sl(noise.known_step), known_recur=sl(noise.known_recur))
        S = len(times) - 1
        full = tuple(img.shape)
        ms = self._multistep(ms_on, i0, i1, history, img)
        # (a segment call of the multistep solver hands the history of its last step back beside its result)
        handed = (lambda out: (out, ms[1])) if (ms is not None and step_range is not None) else (lambda out: out)
        karm = self._known_armer(kn, full, noise, device, init=init_img is None)
        kz = lambda row, word: self._known_z(full, row, word, seed, sample_offset, device)
        inpaint = cond if (self.conditioned_steps == 0 and cond is not None) else None
        if design_fn is None:
            desc = self._desc_for(shape, None, clip=clip_denoised)
            cond_d = self._f32(cond, device) if (cond is not None and self.conditioned_steps != 0) else None
            inp = self._f32(inpaint, device)
            tarr = (C.c_int32 * (S + 1))(*times)
            carr = coefs.contiguous()

            rec = self._recorder(return_trajectory_every, trajectory, S, tuple(img.shape), device, times=times)

            def call(h, un, ws):
                self._arm(rec, h)
                self._arm_known(karm, h)
                self._arm_multistep(ms, h)
                with torch.cuda.device(device):
                    _ffi.check(_ffi.lib().cindm_ddpm1d_sample_ddim(
                        h, self.model._h, un, C.byref(desc), _ffi.ptr(img), _ffi.ptr(cond_d), S, tarr, _ffi.ptr(carr),
                        _ffi.ptr(None if noise is None else noise.step), C.c_uint64(seed), sample_offset, _ffi.ptr(inp),
                        0 if inp is None else inp.shape[1], _ffi.ptr(None if noise is None else noise.cond), B,
                        _ffi.ptr(ws), ws.numel(), _ffi.current_stream(device), int(use_graph)))
            return handed(self._recorded(self._chain(img, desc, call), rec))
        if "recurrence" not in design_guidance:
            raise NotImplementedError("DDIM with design_fn needs a '-recurrence-N' guidance (the reference's other branch "
                                      "returns x_{t-1}, not a noise prediction, :1283)")
        n_composed = 0 if n_composed is None else n_composed
        desc = self._desc_for(shape, compose_mode, n_composed, compose_start_step, shape[1], compose_n_bodies,
                              clip=True)     # p_sample_compose_inside's own default: clip_denoised is not forwarded (:1758-1770)
        if dz is not None and dz.recurrence >= 1:
            # built-in objective: relaxations, gradient, overwrite and the DDIM update stay inside the captured step
            rec = self._recorder(return_trajectory_every, trajectory, S, tuple(img.shape), device, times=times)
            return handed(self._recorded(self._run_guided_ddim(img, cond, desc, dz, times, coefs, noise=noise, seed=seed,
                                                               sample_offset=sample_offset, inpaint_cond=inpaint,
                                                               initial_state_overwrite=initial_state_overwrite, use_graph=use_graph,
                                                               rec=rec, tables=tables, karm=karm, ms=ms), rec))
        coefs = coefs.to(device)
        kap = None if ms is None else ms[0].to(device)
        img_T = img
        # this route loops in Python: the same record, cloned per step
        rec = None if return_trajectory_every is None else LoopRecorder(S, return_trajectory_every, trajectory, times=times)

        def chain():
            img = img_T
            x_prev = None if ms is None else ms[2]
            if rec is not None:
                rec.reset()
            if kn is not None and init_img is None:      # rule 1
                img = self.known_replace(img, kn[0], kn[1], times[0], kz(None if noise is None else noise.known_init, self.num_timesteps))
            for i, (t, tn) in enumerate(zip(times[:-1], times[1:])):
                rn = None if (noise is None or noise.recur is None) else noise.recur[i]
                relaxed = {} if kn is None else dict(after_relax=lambda r, x, i=i, t=t: self.known_replace(
                    x, kn[0], kn[1], t, kz(None if noise is None else noise.known_recur[i][r], t + 0x10000 * (r + 1))))
                eps, x_start = self._guided_step(img, cond, t, desc, design_fn, design_guidance, initial_state_overwrite,
                                                 None, rn, ddim_return=True, check=False, **relaxed)
                if tn < 0:
                    img = x_start
                else:
                    z = noise.step[i] if noise is not None else torch.randn_like(img)
                    img = x_start * coefs[i, 0] + coefs[i, 1] * eps + coefs[i, 2] * z
                    if ms is not None and float(ms[0][i]) != 0.0:      # the multistep term (kappa == 0 reads no history)
                        img = img + kap[i] * (x_start - x_prev)
                    if inpaint is not None:
                        zc = noise.cond[i] if (noise is not None and noise.cond is not None) else torch.randn_like(inpaint)
                        img[:, :inpaint.shape[1], :] = self.q_sample(self._f32(inpaint, device), t, zc)
                if kn is not None:      # the region overwrites last, at the level the step has reached (the last pair: k itself)
                    img = self.known_replace(img, kn[0], kn[1], tn, None if tn < 0 else kz(None if noise is None else noise.known_step[i], tn))
                if rec is not None:
                    rec.after(i, img, x_start)
                x_prev = x_start
            if ms is not None:
                ms[1].copy_(x_prev)
            return img

        img = chain()
        if self._timed_out(desc, device):
            img = self._rerun_exchange_free(chain, desc, device)
        return handed(self._recorded(img, rec))

    # ------------------------------------------------------------------ autoregressive time composition
    @torch.no_grad()
    def autoregress_time_compose_sample(self, batch_size, cond, n_composed, is_single_step_prediction=False, prediction_steps=40,
                                        *, noise=None, seed=None, sample_offset=0, use_graph=True, return_trajectory_every=None,
                                        trajectory=("x",), solver="ddim"):
        """:2240-2327 (the default ``--time_compose_method autoregress`` of inference/inference_1d_composing_time_steps.py, :179-213).
        K segments -- n_composed + 1, or ceil(prediction_steps / conditioned_steps) with ``is_single_step_prediction`` --
        each an unguided DDIM chain on a fresh x_T [B, rollout_steps, F] conditioned on ``cond`` (segment 0) or on the last
        conditioned_steps rows of the previous segment; exactly ``ddim_sample(design_fn=None)``'s prediction and update per step
        (:2266-2287 / :2301-2322; clip_x_start, eta = ddim_sampling_eta).  Returns [B, K * rollout_steps, F], segment k at
        rows k R .. (k+1) R.  ``batch_size`` is not used (B = cond.shape[0]), as in the reference.
        Build-only keywords as ``ddim_sample``: ``seed`` (segment k uses ``autoregress_segment_seeds(seed, K)[k]``, so segment k
        equals ``ddim_sample(seed=seed_k)`` on its condition), ``sample_offset``, ``use_graph``, ``noise`` = NoiseTape(init
        [K,B,R,F], step [K,S,B,R,F]).  The whole rollout is one library call (``cindm_ddpm1d_sample_autoregress``)."""
        if check_solver(self, solver):
            raise NotImplementedError("solver='dpmpp-2m': the autoregressive rollout runs the first-order DDIM update only")
        if return_trajectory_every is not None:
            raise NotImplementedError("return_trajectory_every: the autoregressive rollout's step index is (segment, step) and the "
                                      "library does not record it; record a segment with ddim_sample(seed=autoregress_segment_seeds(...)[k])")
        K = autoregress_segments(self.conditioned_steps, self.rollout_steps, n_composed, is_single_step_prediction,
                                 prediction_steps)
        Lc, R = self.conditioned_steps, self.rollout_steps
        if cond is None or cond.dim() != 3 or cond.shape[1] != Lc:
            raise ValueError(f"cond must be [B, conditioned_steps = {Lc}, F], got {None if cond is None else tuple(cond.shape)}")
        if cond.shape[2] != self.channels:
            raise ValueError(f"cond has {cond.shape[2]} features, the model's transition_dim is {self.channels}")
        device = self.betas.device
        if device.type != "cuda":
            raise _ffi.CindmError("GaussianDiffusion1D is on the CPU: move it to a ROCm device; there is no CPU execution path")
        if seed is None and noise is None:
            seed = self._draw_seed()
        seed = 0 if seed is None else int(seed)
        B, F = cond.shape[0], cond.shape[2]
        shape = (B, R, F)
        times, coefs = self.ddim_schedule()
        S = len(times) - 1
        init = step = None
        if noise is not None:
            noise = noise.to(device)
            init, step = noise.init, noise.step
            if init is None or tuple(init.shape) != (K,) + shape or step is None or tuple(step.shape) != (K, S) + shape:
                raise ValueError(f"noise: init must be [{K}, {B}, {R}, {F}] and step [{K}, {S}, {B}, {R}, {F}] (segment first)")
        desc = self._desc_for(shape, None, clip=True)
        cond_d = self._f32(cond, device)
        img = torch.empty(shape, dtype=torch.float32, device=device)
        cond_buf = torch.empty((B, Lc, F), dtype=torch.float32, device=device)
        out = torch.empty((B, K * R, F), dtype=torch.float32, device=device)
        tarr = (C.c_int32 * (S + 1))(*times)
        carr = coefs.contiguous()
        sarr = (C.c_uint64 * K)(*autoregress_segment_seeds(seed, K))

        def call(h, un, ws):
            with torch.cuda.device(device):
                _ffi.check(_ffi.lib().cindm_ddpm1d_sample_autoregress(
                    h, self.model._h, un, C.byref(desc), _ffi.ptr(img), _ffi.ptr(cond_d), _ffi.ptr(cond_buf), _ffi.ptr(out), K, S,
                    tarr, _ffi.ptr(carr), sarr, _ffi.ptr(init), _ffi.ptr(step), sample_offset, B, _ffi.ptr(ws), ws.numel(),
                    _ffi.current_stream(device), int(use_graph)))
        return self._chain(img, desc, call, result=out)

    # ------------------------------------------------------------------ parallel time composition
    @torch.no_grad()
    def composing_time_sample(self, shape, cond, clip_denoised=True, n_composed=2, *, noise=None, seed=None, sample_offset=0,
                              use_graph=True, return_trajectory_every=None, trajectory=("x",), solver="ddim"):
        """:1807-1854 (the ``EBMs_compose`` method of inference/inference_1d_composing_time_steps.py, :171-178).  All
        K = n_composed + 1 segments are denoised side by side by ONE unguided DDIM chain on K * B rows: at the top of every
        step segment k + 1 takes the last conditioned_steps rows of segment k's current, still noisy state as its condition
        (segment 0 keeps ``cond``); prediction and update per step are ``ddim_sample(design_fn=None)``'s (:1838-1846;
        clip_x_start = ``clip_denoised``, eta = ddim_sampling_eta; under pred_x0 / pred_v with the clamp on pred_noise is
        re-derived from the CLAMPED x_start, :1018-1027, as in ``ddim_sample``).  S sequential steps where ``autoregress_time_compose_sample``
        takes K * S -- and another algorithm: the later segments never see a finished condition.
        ``shape`` = (B, image_size, F) with B = cond.shape[0].  Returns (img [B, R, F], img_infered [B, n_composed * min(20, R), F]):
        segment 0, and the last min(20, R) rows of segments 1 .. K - 1 in order (the reference's literal ``-20:``).
        Build-only keywords as ``autoregress_time_compose_sample``: ``seed`` (segment k draws under
        ``autoregress_segment_seeds(seed, K)[k]``: its x_T and step noise are ``ddim_sample(seed=seed_k)``'s, so ``img`` IS
        ``ddim_sample(shape, cond, seed=seed)``), ``sample_offset``, ``use_graph``, ``noise`` = NoiseTape(init [K,B,R,F], step
        [S,K,B,R,F], indexed by the DDIM step).  ``return_trajectory_every`` / ``trajectory``: as ``ddim_sample``; the call then
        returns ((img, img_infered), ChainRecord) with ``.x`` / ``.x0`` [n_records, K, B, R, F].  One library call
        (``cindm_ddpm1d_sample_timecompose``): the update of every step also performs the hand-over."""
        if check_solver(self, solver):
            raise NotImplementedError("solver='dpmpp-2m': the parallel time composition runs the first-order DDIM update only")
        Lc, R = self.conditioned_steps, self.image_size
        K = time_compose_segments(Lc, R, n_composed)
        if cond is None or cond.dim() != 3 or cond.shape[1] != Lc:
            raise ValueError(f"cond must be [B, conditioned_steps = {Lc}, F], got {None if cond is None else tuple(cond.shape)}")
        if self.model_unconditioned is None and cond.shape[2] != self.channels:      # (with it: four bodies, checked by _desc_for)
            raise ValueError(f"cond has {cond.shape[2]} features, the model's transition_dim is {self.channels}")
        B, F = cond.shape[0], cond.shape[2]
        if tuple(shape) != (B, R, F):
            raise ValueError(f"shape must be (B, image_size, F) = {(B, R, F)} for this cond and model, got {tuple(shape)}")
        if K * B > 65535:
            raise ValueError(f"(n_composed + 1) * B = {K * B} rows: the library chain runs at most 65535")
        rows = (K * B, R, F)
        desc = self._desc_for(rows, None, clip=clip_denoised)
        times, coefs = self.ddim_schedule()
        S = len(times) - 1
        init = step = None
        if noise is not None:
            init, step = noise.init, noise.step
            if init is None or tuple(init.shape) != (K, B, R, F) or step is None or tuple(step.shape) != (S, K, B, R, F):
                raise ValueError(f"noise: init must be [{K}, {B}, {R}, {F}] and step [{S}, {K}, {B}, {R}, {F}] (step first, then segment)")
        if return_trajectory_every is not None:
            record_schedule(S, return_trajectory_every)
            stream_mask(trajectory)
        device = self.betas.device
        if device.type != "cuda":
            raise _ffi.CindmError("GaussianDiffusion1D is on the CPU: move it to a ROCm device; there is no CPU execution path")
        if seed is None and noise is None:
            seed = self._draw_seed()
        seed = 0 if seed is None else int(seed)
        if noise is not None:
            noise = noise.to(device)
            init, step = noise.init, noise.step
        cond_d = self._f32(cond, device)
        x = torch.empty(rows, dtype=torch.float32, device=device)
        cond_buf = torch.empty((K * B, Lc, F), dtype=torch.float32, device=device)
        tarr = (C.c_int32 * (S + 1))(*times)
        carr = coefs.contiguous()
        sarr = (C.c_uint64 * K)(*autoregress_segment_seeds(seed, K))
        rec = self._recorder(return_trajectory_every, trajectory, S, rows, device, times=times)

        def call(h, un, ws):
            self._arm(rec, h)
            with torch.cuda.device(device):
                _ffi.check(_ffi.lib().cindm_ddpm1d_sample_timecompose(
                    h, self.model._h, un, C.byref(desc), _ffi.ptr(x), _ffi.ptr(cond_d), _ffi.ptr(cond_buf), K, S, tarr,
                    _ffi.ptr(carr), sarr, _ffi.ptr(init), _ffi.ptr(step), sample_offset, B, _ffi.ptr(ws), ws.numel(),
                    _ffi.current_stream(device), int(use_graph)))
        out = time_compose_assemble(self._chain(x, desc, call), K)
        if rec is None:
            return out
        return out, rec.collect(self._handle(), lambda r: r.reshape((r.shape[0], K, B, R, F)))
