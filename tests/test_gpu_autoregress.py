"""GPU (MI355X): the autoregressive time composition (GaussianDiffusion1D.autoregress_time_compose_sample,
cindm_ddpm1d_sample_autoregress) against the reference's own rollout (tests/golden/autoregress_1d.npz, same noise draws), its
bitwise identity with a Python composition of the public ddim_sample, size-independent bitwise properties, the time-out
recovery of the whole rollout, and the horizon-8 U-Net of the single-step variant against the oracle.

Tolerances as tests/test_gpu_parity.py: U-Net forwards 2e-5, free-running chains 1e-4."""
import os

import numpy as np
import pytest
import torch

import cindm_amd
import cindm_oracle as O
from cindm_amd.diffusion1d import autoregress_segment_seeds
from test_autoregress_host import CASES
from test_gpu_parity import TOL_CHAIN, TOL_FWD, build_unet, rel

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def unet24(device):
    return build_unet(device, 24, 8)


@pytest.fixture(scope="module")
def unet8h(device):
    return build_unet(device, 8, 8)


def _diff(model, device, Lc, R, S, eta):
    return cindm_amd.GaussianDiffusion1D(model, image_size=R, conditioned_steps=Lc, timesteps=1000, sampling_timesteps=S,
                                         loss_type="l1", ddim_sampling_eta=eta).to(device)


def _cond(B, Lc, seed):
    return (torch.rand((B, Lc, 8), generator=torch.Generator().manual_seed(seed)) - 0.5)


# ------------------------------------------------------------------ against the reference
@pytest.mark.parametrize("tag", sorted(CASES))
def test_autoregress_golden(gold_dir, device, unet24, unet8h, tag):
    g = np.load(os.path.join(gold_dir, "autoregress_1d.npz"))
    hz, Lc, R, n_composed, single, P, S, eta, B = CASES[tag]
    d = _diff((unet24 if hz == 24 else unet8h)[0], device, Lc, R, S, eta)
    tape = cindm_amd.NoiseTape(torch.from_numpy(g[f"{tag}.init"]), torch.from_numpy(g[f"{tag}.step"]))
    cond = torch.from_numpy(g[f"{tag}.cond"]).to(device)
    out = d.autoregress_time_compose_sample(B, cond, n_composed, is_single_step_prediction=single, prediction_steps=P, noise=tape)
    assert tuple(out.shape) == tuple(g[f"{tag}.out"].shape)
    assert rel(out, g[f"{tag}.out"]) < TOL_CHAIN, tag
    K = g[f"{tag}.seg"].shape[0]
    for k in range(K):
        assert rel(out[:, k * R:(k + 1) * R], g[f"{tag}.seg"][k]) < TOL_CHAIN, (tag, k)


# ------------------------------------------------------------------ bitwise: one call == composed ddim_sample calls
VARIANTS = {"default": (24, 4, 20, 2, False, 40), "single_step": (8, 4, 4, 0, True, 12)}


def _composed(d, cond, K, seed, sample_offset):
    segs, c = [], cond
    for s in autoregress_segment_seeds(seed, K):
        img = d.ddim_sample((cond.shape[0], d.rollout_steps, cond.shape[2]), c, seed=s, sample_offset=sample_offset)
        segs.append(img.clone())
        c = img[:, -d.conditioned_steps:].clone()
    return torch.cat(segs, dim=1)


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_rollout_equals_composed_ddim_sample(device, unet24, unet8h, variant):
    hz, Lc, R, n_composed, single, P = VARIANTS[variant]
    d = _diff((unet24 if hz == 24 else unet8h)[0], device, Lc, R, 10, 1.0)
    K = P // Lc if single else n_composed + 1
    cond = _cond(5, Lc, 11).to(device)
    for off in (0, 9):
        out = d.autoregress_time_compose_sample(5, cond, n_composed, is_single_step_prediction=single, prediction_steps=P,
                                                seed=1234, sample_offset=off)
        assert tuple(out.shape) == (5, K * R, 8)
        want = _composed(d, cond, K, 1234, off)
        assert torch.equal(out, want), (variant, off)


def test_rollout_bitwise_properties(device, unet24):
    d = _diff(unet24[0], device, 4, 20, 12, 1.0)
    cond = _cond(16, 4, 12).to(device)
    run = lambda **kw: d.autoregress_time_compose_sample(16, cond, 2, **{"seed": 77, **kw}).clone()
    a = run()
    assert bool(torch.isfinite(a).all())
    assert torch.equal(a, run(use_graph=False))
    assert torch.equal(a, run())
    b = run(seed=78)
    assert not torch.equal(a, b)
    for k in range(3):                    # every segment depends on the seed
        assert not torch.equal(a[:, 20 * k:20 * (k + 1)], b[:, 20 * k:20 * (k + 1)]), k
    lo = d.autoregress_time_compose_sample(6, cond[:6], 2, seed=77, sample_offset=0)
    hi = d.autoregress_time_compose_sample(10, cond[6:], 2, seed=77, sample_offset=6)
    assert torch.equal(a[:6], lo) and torch.equal(a[6:], hi)
    assert float(a.abs().max()) <= 1.0 + 1e-5             # every segment ends on the clamped x_start


def test_segment_x_T_differ(device, unet24):
    """Segment k's x_T is the draw of ddim_sample(seed = seed_k): two segments never start from the same noise."""
    d = _diff(unet24[0], device, 4, 20, 8, 0.0)
    s0, s1 = autoregress_segment_seeds(5, 2)
    x0 = d._init_state((4, 20, 8), device, None, s0, 0, d.num_timesteps)
    x1 = d._init_state((4, 20, 8), device, None, s1, 0, d.num_timesteps)
    assert not torch.equal(x0, x1)
    assert float((x0 - x1).abs().mean()) > 0.5
    # and the rollout uses them: with eta = 0 a segment is a function of its condition and its x_T, and segment 1 is the
    # chain from seed_1's x_T on segment 0's tail, not the chain from seed_0's
    cond = _cond(4, 4, 13).to(device)
    out = d.autoregress_time_compose_sample(4, cond, 1, seed=5)
    tail = out[:, 16:20].contiguous()
    assert torch.equal(out[:, 20:], d.ddim_sample((4, 20, 8), tail, seed=s1))
    assert not torch.equal(out[:, 20:], d.ddim_sample((4, 20, 8), tail, seed=s0))


# ------------------------------------------------------------------ recovery
def test_rollout_exchange_timeout_is_recovered_once(device):
    """dbg = 39 stands in for a partner workgroup kept off the chip (tests/test_gpu_paths.py::test_exchange_timeout_is_recovered):
    the whole rollout is re-run once on the exchange-free kernels and equals what that selection computes by itself."""
    m, _ = build_unet(device, 24, 8)
    m.set_option("auto_range", 0)
    d = _diff(m, device, 4, 20, 4, 0.5)
    cond = _cond(32, 4, 14).to(device)
    m.exchange_free(True)
    ref = d.autoregress_time_compose_sample(32, cond, 1, seed=3).clone()
    m.exchange_free(False)
    assert m.recovered == 0
    m.set_option("dbg", 39)
    try:
        got = d.autoregress_time_compose_sample(32, cond, 1, seed=3)
        info = d.last_chain_info()
    finally:
        m.set_option("dbg", 0)
    assert info["recovered"] and m.recovered == 1
    assert torch.equal(got, ref)


# ------------------------------------------------------------------ the single-step model: horizon 8 (levels 8 -> 4 -> 2 -> 1)
@pytest.mark.parametrize("att", [True, False])
@pytest.mark.parametrize("B", [1, 2, 7, 64])
def test_unet_horizon8_vs_oracle(device, att, B):
    m, sd = build_unet(device, 8, 8, att)
    x = torch.randn((B, 8, 8), generator=torch.Generator().manual_seed(800 + B))
    for t in (0, 321, 999):
        ref = O.unet1d_forward(sd, x, torch.full((B,), t, dtype=torch.long))
        out = m(x.to(device), torch.full((B,), t, device=device))
        assert rel(out, ref) < TOL_FWD, (att, B, t)
