"""DDPM schedule tables (host, init-time only): the 13 fp32 buffers GaussianDiffusion1D /
GaussianDiffusion register (model/diffusion_1d.py:846-910, model/diffusion_2d.py:600-674 of the
reference).  Everything is derived in fp64 from beta and only then cast to fp32
(SURVEY.md Appendix A.5 / B.4)."""
import math

import torch


def beta_schedule(kind, timesteps):
    T = timesteps
    if kind == "linear":                 # model/diffusion_1d.py:464-468
        s = 1000 / T
        return torch.linspace(s * 1e-4, s * 0.02, T, dtype=torch.float64)
    grid = torch.linspace(0, T, T + 1, dtype=torch.float64)
    if kind == "cosine":                 # :470-480, s = 0.008
        f = torch.cos((grid / T + 0.008) / 1.008 * math.pi * 0.5) ** 2
    elif kind == "sigmoid":              # model/diffusion_2d.py:518-531, start -3, end 3, tau 1
        lo, hi = torch.tensor(-3.0).sigmoid(), torch.tensor(3.0).sigmoid()
        f = (hi - (grid / T * 6.0 - 3.0).sigmoid()) / (hi - lo)
    else:
        raise ValueError(f"unknown beta schedule {kind}")
    f = f / f[0]
    return torch.clip(1 - f[1:] / f[:-1], 0, 0.999)


def make_schedule(kind="cosine", timesteps=1000, objective="pred_noise"):
    beta = beta_schedule(kind, timesteps)
    alpha = 1.0 - beta
    abar = torch.cumprod(alpha, dim=0)
    abar_prev = torch.cat([torch.ones(1, dtype=torch.float64), abar[:-1]])
    pvar = beta * (1.0 - abar_prev) / (1.0 - abar)
    snr = abar / (1 - abar)
    weight = {"pred_noise": torch.ones_like(snr), "pred_x0": snr, "pred_v": snr / (snr + 1)}[objective]
    tab = dict(
        betas=beta, alphas_cumprod=abar, alphas_cumprod_prev=abar_prev,
        sqrt_alphas_cumprod=abar.sqrt(), sqrt_one_minus_alphas_cumprod=(1.0 - abar).sqrt(),
        log_one_minus_alphas_cumprod=(1.0 - abar).log(), sqrt_recip_alphas_cumprod=(1.0 / abar).sqrt(),
        sqrt_recipm1_alphas_cumprod=(1.0 / abar - 1).sqrt(), posterior_variance=pvar,
        posterior_log_variance_clipped=pvar.clamp(min=1e-20).log(),
        posterior_mean_coef1=beta * abar_prev.sqrt() / (1.0 - abar),
        posterior_mean_coef2=(1.0 - abar_prev) * alpha.sqrt() / (1.0 - abar),
        loss_weight=weight,
    )
    return {k: v.to(torch.float32) for k, v in tab.items()}


def ddim_schedule(diffusion):
    """(times [S+1] descending to -1, coefs [S,3] = (sqrt(alpha_next), c, sigma)) of ddim_sample (model/diffusion_1d.py:1743-1777,
    the same recurrence as model/diffusion_2d.py:913-949) for a GaussianDiffusion1D / GaussianDiffusion, in the reference's fp32
    tensor arithmetic (time_next = -1 indexes the last table entry, as the reference's negative index does; that step returns
    x_start and its coefficients are not used)."""
    d = diffusion
    T, S, eta = d.num_timesteps, d.sampling_timesteps, d.ddim_sampling_eta
    # the table is a pure function of (T, S, eta, alphas_cumprod): built once (250 iterations of scalar tensor arithmetic and
    # a device -> host copy cost 7 ms per ddim_sample call, 8 % of a 250-step chain of 256 designs)
    key = (T, S, float(eta), d.alphas_cumprod.data_ptr(), d.alphas_cumprod._version)
    cached = getattr(d, "_ddim_cache", None)
    if cached is not None and cached[0] == key:
        return list(cached[1]), cached[2].clone()
    times = torch.linspace(-1, T - 1, steps=S + 1)
    times = list(reversed(times.int().tolist()))
    ac = d.alphas_cumprod.detach().to("cpu", torch.float32)
    coefs = torch.zeros((S, 3), dtype=torch.float32)
    for i, (time, time_next) in enumerate(zip(times[:-1], times[1:])):
        alpha, alpha_next = ac[time], ac[time_next]
        sigma = eta * ((1 - alpha / alpha_next) * (1 - alpha_next) / (1 - alpha)).sqrt()
        c = (1 - alpha_next - sigma ** 2).sqrt()
        coefs[i, 0], coefs[i, 1], coefs[i, 2] = alpha_next.sqrt(), c, sigma
    coefs = torch.nan_to_num(coefs, nan=0.0)
    d._ddim_cache = (key, list(times), coefs.clone())
    return times, coefs


SOLVERS = ("ddim", "dpmpp-2m")


def multistep_kappa(diffusion):
    """fp32 [S]: the per-step factor of the second-order multistep solver (DPM-Solver++ 2M in data-prediction form)
    on the ``ddim_schedule()`` grid.  For the pair (t, t') of step i, with alpha = sqrt(abar_t), sigma = sqrt(1 - abar_t),
    lambda = ln(alpha / sigma) (primes for t') and h_i = lambda' - lambda,
        kappa_i = (alpha' - sigma' alpha / sigma) h_i / (2 h_{i-1}),   kappa_0 = 0,   kappa_i = 0 for the last pair (t' < 0),
    so that "DDIM update + kappa_i (X_i - X_{i-1})" is the solver's step.  Computed in float64 from ``alphas_cumprod`` and rounded
    once; cached like ``ddim_schedule``.  ValueError when lambda is not strictly increasing along the grid (h <= 0)."""
    d = diffusion
    T, S = d.num_timesteps, d.sampling_timesteps
    key = (T, S, d.alphas_cumprod.data_ptr(), d.alphas_cumprod._version)
    cached = getattr(d, "_kappa_cache", None)
    if cached is not None and cached[0] == key:
        return cached[1].clone()
    times, _ = ddim_schedule(d)
    ac = d.alphas_cumprod.detach().to("cpu", torch.float64)
    grid = [t for t in times if t >= 0]
    a = torch.stack([ac[t] for t in grid]).sqrt()
    s = torch.stack([1.0 - ac[t] for t in grid]).sqrt()
    lam = torch.log(a / s)
    h = lam[1:] - lam[:-1]                       # h[i]: step i, for every pair whose t' >= 0
    if not bool(torch.isfinite(lam).all()) or not bool((h > 0).all()):
        raise ValueError("multistep_kappa: lambda = ln(alpha / sigma) is not strictly increasing along the DDIM time grid")
    kappa = torch.zeros(len(times) - 1, dtype=torch.float64)
    for i in range(1, len(h)):
        kappa[i] = (a[i + 1] - s[i + 1] * a[i] / s[i]) * h[i] / (2.0 * h[i - 1])
    kappa = kappa.to(torch.float32)
    d._kappa_cache = (key, kappa.clone())
    return kappa


def check_solver(diffusion, solver):
    """What the ``solver=`` keyword of the sampling methods refuses, before any device work: an unknown name, and for "dpmpp-2m" a
    stochastic chain (``ddim_sampling_eta != 0``) or one that is not a DDIM chain (``sampling_timesteps == timesteps``).  Returns
    True for the multistep solver."""
    if solver not in SOLVERS:
        raise ValueError(f"unknown solver {solver!r}: one of {SOLVERS}")
    if solver == "ddim":
        return False
    if float(diffusion.ddim_sampling_eta) != 0.0:
        raise ValueError("solver='dpmpp-2m' is deterministic: ddim_sampling_eta must be 0")
    if not diffusion.sampling_timesteps < diffusion.num_timesteps:
        raise ValueError("solver='dpmpp-2m' runs on the DDIM chains: construct the diffusion with sampling_timesteps < timesteps")
    return True


ULA_STEP_SCALE = 0.035         # sample_step_ULA's step size: betas_inference * 0.035 (model/diffusion_1d.py:2050)


def ula_schedule(betas_inference):
    """(scalar, ss, std), each fp32 [len(betas_inference)] indexed by the timestep i, of the Langevin phase of
    sample_compose_multibodies (model/diffusion_1d.py:1998-1999, :2050, :2054) in the reference's tensor arithmetic at the
    dtype of ``betas_inference`` (fp64 for linear_beta_schedule):
        scalar = sqrt(1 / (1 - cumprod(1 - betas_inference)))     the factor of gradient()'s -scalar[i] * eps (:1924)
        ss     = betas_inference * 0.035                          the step size
        std    = (2 * ss) ** .5                                   the noise scale
    cast to fp32 last: the reference multiplies them as zero-dim tensors into fp32 tensors, which rounds each to fp32 once."""
    b = torch.as_tensor(betas_inference).detach().to("cpu")
    if b.dim() != 1 or not b.is_floating_point():
        raise ValueError("betas_inference must be a 1-D floating-point tensor")
    scalar = torch.sqrt(1 / (1 - torch.cumprod(1. - b, dim=0)))
    ss = b * ULA_STEP_SCALE
    std = (2 * ss) ** .5
    return scalar.to(torch.float32), ss.to(torch.float32), std.to(torch.float32)
