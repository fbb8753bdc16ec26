"""CPU: the second-order multistep solver (``solver="dpmpp-2m"``) as far as the host goes -- the kappa table against an
independent float64 computation, the identity "DDIM update + kappa (X - X_prev)" == DPM-Solver++(2M) in data-prediction form, the
solver's order on an analytic Gaussian score, the keyword's refusals and the binding.  No kernel is launched here.

The Gaussian-score check: data N(mu, s^2) per coordinate; at level (alpha, sigma) the marginal is N(alpha mu, alpha^2 s^2 + sigma^2),
the exact denoiser is E[x0 | x] = mu + alpha s^2 (x - alpha mu) / (alpha^2 s^2 + sigma^2), and the probability-flow ODE carries
x_T to alpha mu + sqrt((alpha^2 s^2 + sigma^2) / (alpha_T^2 s^2 + sigma_T^2)) (x_T - alpha_T mu).  The state before the final
step (the final step returns X itself, for both solvers) is compared with that solution.  Bound: the multistep error is at most a
quarter of DDIM's in every case (the issue's bound; the worst ratio it reports is 4.7)."""
import ctypes as C
import math
import os
import re

import pytest
import torch

import cindm_amd
from cindm_amd import _ffi
from cindm_amd.schedule import ddim_schedule, multistep_kappa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HZ = 24


def _diff1d(S, kind="cosine", eta=0.0, timesteps=1000):
    m = cindm_amd.TemporalUnet1D(HZ, 8, False, attention=True)
    return cindm_amd.GaussianDiffusion1D(m, image_size=HZ, conditioned_steps=0, timesteps=timesteps, sampling_timesteps=S,
                                         loss_type="l1", beta_schedule=kind, ddim_sampling_eta=eta)


@pytest.fixture(scope="module")
def unet2d_host():
    return cindm_amd.Unet(dim=64, dim_mults=(1, 2), channels=21)


def _diff2d(m, S, eta=0.0):
    return cindm_amd.GaussianDiffusion(m, image_size=64, frames=6, timesteps=1000, sampling_timesteps=S, ddim_sampling_eta=eta)


def _levels(d):
    """(times, alpha [S + 1], sigma [S + 1]) in float64 on the DDIM grid; the entries of time -1 are not used."""
    times, _ = ddim_schedule(d)
    ac = d.alphas_cumprod.double()
    a = [math.sqrt(float(ac[t])) if t >= 0 else float("nan") for t in times]
    s = [math.sqrt(1.0 - float(ac[t])) if t >= 0 else float("nan") for t in times]
    return times, a, s


def _kappa_f64(d):
    """kappa from lambda, step by step in Python floats (float64): independent of schedule.multistep_kappa's tensor code."""
    times, a, s = _levels(d)
    S = len(times) - 1
    lam = [math.log(a[j] / s[j]) if times[j] >= 0 else None for j in range(S + 1)]
    out = [0.0] * S
    for i in range(1, S):
        if times[i + 1] < 0:
            continue
        h, h_prev = lam[i + 1] - lam[i], lam[i] - lam[i - 1]
        out[i] = (a[i + 1] - s[i + 1] * a[i] / s[i]) * h / (2.0 * h_prev)
    return out


def _ulp32(v):
    v32 = torch.tensor(v, dtype=torch.float32)
    return float((torch.nextafter(v32.abs(), torch.tensor(float("inf"))) - v32.abs()).double())


# ------------------------------------------------------------------ 1. the table
@pytest.mark.parametrize("kind", ["cosine", "sigmoid"])
@pytest.mark.parametrize("S", [5, 6, 50, 250])
def test_kappa_matches_float64_lambda_computation(kind, S):
    d = _diff1d(S, kind)
    k = multistep_kappa(d)
    assert k.dtype == torch.float32 and tuple(k.shape) == (S,)
    assert float(k[0]) == 0.0 and float(k[-1]) == 0.0        # the first step has no history, the last pair returns X
    ref = _kappa_f64(d)
    for i in range(S):
        assert abs(float(k[i].double()) - ref[i]) <= _ulp32(ref[i]), (i, float(k[i]), ref[i])
    assert all(float(v) != 0.0 for v in k[1:-1])
    assert torch.equal(d.multistep_kappa(), k)


def test_kappa_cache_follows_alphas_cumprod():
    d = _diff1d(6)
    k0 = multistep_kappa(d)
    k0[1] = 123.0                                            # (the caller's copy is its own)
    assert float(multistep_kappa(d)[1]) != 123.0
    assert d._kappa_cache[1] is not None
    k1 = multistep_kappa(d)
    d.alphas_cumprod.mul_(0.9)                               # in place: the version counter moves
    k2 = multistep_kappa(d)
    assert not torch.equal(k1, k2)
    ref = _kappa_f64(d)
    assert all(abs(float(k2[i].double()) - ref[i]) <= _ulp32(ref[i]) for i in range(6))


def test_kappa_refuses_a_grid_whose_lambda_does_not_increase():
    d = _diff1d(5)
    d.alphas_cumprod.copy_(d.alphas_cumprod.flip(0))         # noise level falls with t: lambda decreases along the grid
    with pytest.raises(ValueError, match="strictly increasing"):
        multistep_kappa(d)


# ------------------------------------------------------------------ 2. the identity
@pytest.mark.parametrize("kind", ["cosine", "sigmoid"])
def test_ddim_plus_kappa_term_is_dpm_solver_pp_2m(kind):
    """On random float64 tensors with E = (x - alpha X) / sigma, per step of an S = 10 grid."""
    d = _diff1d(10, kind)
    times, a, s = _levels(d)
    kap = _kappa_f64(d)
    g = torch.Generator().manual_seed(5)
    for i in range(1, 9):
        x, X, Xp = (torch.randn((3, 7), generator=g, dtype=torch.float64) for _ in range(3))
        E = (x - a[i] * X) / s[i]
        ours = a[i + 1] * X + s[i + 1] * E + kap[i] * (X - Xp)
        lam = lambda j: math.log(a[j] / s[j])
        h, h_prev = lam(i + 1) - lam(i), lam(i) - lam(i - 1)
        r = h_prev / h
        D = (1.0 + 1.0 / (2.0 * r)) * X - (1.0 / (2.0 * r)) * Xp
        theirs = (s[i + 1] / s[i]) * x - a[i + 1] * math.expm1(-h) * D
        assert float((ours - theirs).abs().max() / theirs.abs().max()) < 1e-12, i


# ------------------------------------------------------------------ 3. the order, on an analytic score
MU, SD = 0.3, 0.5


def _gaussian_chain(d, kappa, x_T):
    """(state before the final step, exact ODE solution there): float64 loop, X = the exact denoiser, E the exact noise."""
    times, a, s = _levels(d)
    var = lambda j: a[j] ** 2 * SD ** 2 + s[j] ** 2
    x, X_prev = x_T.clone(), None
    S = len(times) - 1
    for i in range(S - 1):
        X = MU + a[i] * SD ** 2 * (x - a[i] * MU) / var(i)
        E = (x - a[i] * X) / s[i]
        x = a[i + 1] * X + s[i + 1] * E
        if kappa is not None and float(kappa[i]) != 0.0:
            x = x + float(kappa[i]) * (X - X_prev)
        X_prev = X
    exact = a[S - 1] * MU + math.sqrt(var(S - 1) / var(0)) * (x_T - a[0] * MU)
    return x, exact


@pytest.mark.parametrize("kind", ["cosine", "sigmoid"])
@pytest.mark.parametrize("S", [10, 20, 40, 80, 160])
def test_multistep_error_is_a_quarter_of_ddims_on_a_gaussian_score(kind, S):
    d = _diff1d(S, kind)
    times, a, s = _levels(d)
    g = torch.Generator().manual_seed(11)
    x_T = a[0] * MU + math.sqrt(a[0] ** 2 * SD ** 2 + s[0] ** 2) * torch.randn(4096, generator=g, dtype=torch.float64)
    x1, exact = _gaussian_chain(d, None, x_T)
    x2, _ = _gaussian_chain(d, multistep_kappa(d), x_T)          # (the fp32 table, as the chains use it)
    e1, e2 = float((x1 - exact).abs().max()), float((x2 - exact).abs().max())
    print(f"[multistep] {kind} S={S}: multistep {e2:.4e}  ddim {e1:.4e}  ratio {e1 / e2:.2f}")
    assert e2 <= 0.25 * e1, (e2, e1)


# ------------------------------------------------------------------ 4. refusals (before any device work)
def test_refusals_1d():
    shape = (2, HZ, 8)
    with pytest.raises(ValueError, match="unknown solver"):
        _diff1d(5).ddim_sample(shape, None, solver="dpm")
    with pytest.raises(ValueError, match="unknown solver"):
        _diff1d(5).sample(batch_size=2, solver="euler")
    with pytest.raises(ValueError, match="ddim_sampling_eta"):
        _diff1d(5, eta=0.5).ddim_sample(shape, None, solver="dpmpp-2m")
    with pytest.raises(ValueError, match="ddim_sampling_eta"):
        _diff1d(5, eta=0.5).sample(batch_size=2, solver="dpmpp-2m")
    full = _diff1d(1000)                                      # sampling_timesteps == timesteps: the DDPM chain
    with pytest.raises(ValueError, match="sampling_timesteps < timesteps"):
        full.sample(batch_size=2, solver="dpmpp-2m")
    with pytest.raises(ValueError, match="sampling_timesteps < timesteps"):
        full.ddim_sample(shape, None, solver="dpmpp-2m")
    with pytest.raises(ValueError, match="DDPM chain"):
        _diff1d(5).p_sample_loop(shape, None, solver="dpmpp-2m")
    d = _diff1d(5)
    cond = torch.zeros((2, 4, 8))
    with pytest.raises(NotImplementedError, match="autoregressive"):
        d.autoregress_time_compose_sample(2, cond, 1, solver="dpmpp-2m")
    with pytest.raises(NotImplementedError, match="time composition"):
        d.composing_time_sample(shape, cond, solver="dpmpp-2m")
    with pytest.raises(NotImplementedError, match="Langevin"):
        d.sample_compose_multibodies(cond, 1000, 2, 4, solver="dpmpp-2m")
    with pytest.raises(ValueError, match="unknown solver"):
        d.sample_compose_multibodies(cond, 1000, 2, 4, solver="heun")
    # the segment form's history: required from step 1 on, refused at step 0 and with the first-order solver
    with pytest.raises(ValueError, match="history"):
        d.ddim_sample(shape, None, solver="ddim", history=torch.zeros(shape), step_range=(1, 2), init_img=torch.zeros(shape))
    # (the default keeps reaching the device check it reached before)
    with pytest.raises(cindm_amd.CindmError):
        d.ddim_sample(shape, None)
    with pytest.raises(cindm_amd.CindmError):
        d.ddim_sample(shape, None, solver="dpmpp-2m")


def test_refusals_2d(unet2d_host):
    shape = (1, 2, 21, 64, 64)
    with pytest.raises(ValueError, match="unknown solver"):
        _diff2d(unet2d_host, 4).ddim_sample(shape, solver="dpm")
    with pytest.raises(ValueError, match="ddim_sampling_eta"):
        _diff2d(unet2d_host, 4, eta=0.2).sample(batch_size=1, num_boundaries=2, solver="dpmpp-2m")
    with pytest.raises(ValueError, match="sampling_timesteps < timesteps"):
        _diff2d(unet2d_host, 1000).sample(batch_size=1, num_boundaries=2, solver="dpmpp-2m")
    with pytest.raises(ValueError, match="DDPM chain"):
        _diff2d(unet2d_host, 4).p_sample_loop(shape, solver="dpmpp-2m")
    with pytest.raises(cindm_amd.CindmError):
        _diff2d(unet2d_host, 4).ddim_sample(shape, solver="dpmpp-2m")


# ------------------------------------------------------------------ 5. the binding
def test_binding_exists_and_abi_version_is_unchanged():
    L = _ffi.lib()
    assert "cindm_ddpm1d_set_multistep" in _ffi.SIGNATURES and hasattr(L, "cindm_ddpm1d_set_multistep")
    hdr = open(os.path.join(ROOT, "include", "cindm_hip.h")).read()
    assert re.search(r"int\s+cindm_ddpm1d_set_multistep\s*\(", hdr)
    assert L.cindm_abi_version() == _ffi.ABI_VERSION == 4
    # a null handle is refused with a message, not dereferenced
    k = (C.c_float * 2)(0.0, 0.1)
    assert L.cindm_ddpm1d_set_multistep(None, k, 2, None, 0) != 0
    assert b"null handle" in L.cindm_last_error() or b"multistep" in L.cindm_last_error()
