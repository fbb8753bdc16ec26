"""GPU (MI355X): the Langevin (ULA) phase of sample_compose_multibodies (cindm_ddpm1d_sample_ula) through the Python face --
sample_step_ULA, gradient(..., scalar) above t = 400 and the two-phase N = 404 chain against the reference's own output
(tests/golden/ula_1d.npz, same noise draws) and against the CPU restatement of tests/test_ula_host.py; bitwise properties of the
chain (graph / stream, seeds, batch split, timestep-range split, L = 0); the exchange time-out recovery.

Tolerances as tests/test_gpu_parity.py: one update 2e-5 (the update multiplies the U-Net's error by ss * scalar < 1e-2 above
t = 400 -- asserted in tests/test_ula_host.py -- so the single-step bound needs no new number), free-running chains 1e-4."""
import os

import numpy as np
import pytest
import torch

import cindm_amd
import test_ula_host as U
from test_gpu_parity import TOL_CHAIN, TOL_STEP, build_unet, rel

pytestmark = pytest.mark.gpu


def _diff(device, m8, m4, N):
    d = cindm_amd.GaussianDiffusion1D(m8, image_size=U.R, conditioned_steps=U.LC, timesteps=1000, sampling_timesteps=1000,
                                      loss_type="l1", betas_inference=U.linear_beta_schedule(N)).to(device)
    d.model_unconditioned = m4
    return d


@pytest.fixture(scope="module")
def models(device):
    return build_unet(device, U.HZ, 8)[0], build_unet(device, U.HZ, 4)[0]


@pytest.fixture(scope="module")
def gold(gold_dir):
    return np.load(os.path.join(gold_dir, "ula_1d.npz"))


def _say(name, v):
    print(f"[ula] {name}: {v:.3e}")
    return v


# ------------------------------------------------------------------ against the reference
@pytest.mark.parametrize("tag", sorted(U.STEP_CASES))
def test_sample_step_ula_golden(device, models, gold, tag):
    N, t, L, B, _ = U.STEP_CASES[tag]
    d = _diff(device, *models, N)
    x, nz = U.step_inputs(tag)
    scalar = U.scalar_for_gradient(U.linear_beta_schedule(N))
    xd = x.to(device)
    out = d.sample_step_ULA(xd, torch.tensor([t] * B), L, 4, N, scalar, noise=nz.to(device))
    assert torch.equal(xd.cpu(), x)                                   # the caller's state is not modified
    assert _say(f"step {tag}", rel(out, gold[f"step.{tag}.out"])) < TOL_STEP
    assert not torch.equal(out[:, :U.LC].cpu(), x[:, :U.LC])          # the conditioning rows move


@pytest.mark.parametrize("L", [1, 3])
def test_langevin_iterations_vs_restatement_batch5(device, models, L):
    """A batch that is not a multiple of any tile (5 designs: 30 pair rows, 20 single-body rows)."""
    N, t, B = 1000, 731, 5
    d = _diff(device, *models, N)
    g = torch.Generator().manual_seed(5300 + L)
    x, nz = torch.randn((B, U.HZ, U.F), generator=g), torch.randn((L, B, U.HZ, U.F), generator=g)
    b = U.linear_beta_schedule(N)
    scalar = U.scalar_for_gradient(b)
    ref = U.restated_step_ula(U.oracle_diffusion(), x, t, L, b, scalar, nz)
    out = d.sample_step_ULA(x.to(device), torch.tensor([t] * B), L, 4, N, scalar, noise=nz.to(device))
    assert _say(f"batch5 L={L}", rel(out, ref)) < TOL_STEP


def test_gradient_above_400_golden(device, models, gold):
    N, t, B, _ = U.GRAD_CASE
    d = _diff(device, *models, N)
    scalar = U.scalar_for_gradient(U.linear_beta_schedule(N))
    out = d.gradient(U.grad_input().to(device), t, 4, scalar)
    assert _say("gradient", rel(out, gold["grad.out"])) < TOL_STEP
    with pytest.raises(NotImplementedError):
        d.gradient(U.grad_input().to(device), t, 4)


def test_two_phase_chain_golden(device, models, gold):
    N, L, B = U.CHAIN["N"], U.CHAIN["L"], U.CHAIN["B"]
    d = _diff(device, *models, N)
    cond, tape, ula = U.chain_inputs()
    noise = cindm_amd.NoiseTape(tape.init, tape.step, ula=ula)
    run = lambda **kw: d.sample_compose_multibodies(cond.to(device), N, L, 4, noise=noise, **kw)
    post = run(t_stop=401, full_state=True)
    assert tuple(post.shape) == (B, U.HZ, U.F)
    assert _say("chain post", rel(post, gold["chain.post"])) < TOL_CHAIN
    # the Langevin phase moves the conditioning rows: they match the reference's drifted rows, not the caller's cond
    assert rel(post[:, :U.LC], gold["chain.post"][:, :U.LC]) < TOL_CHAIN
    assert float((post[:, :U.LC].cpu() - cond).abs().max()) > 1e-3
    for k, t in enumerate(gold["chain.ckpt_t"]):
        out = run(t_stop=int(t))
        assert tuple(out.shape) == (B, U.R, U.F)
        assert _say(f"chain t={int(t)}", rel(out, gold["chain.ckpt"][k])) < TOL_CHAIN, int(t)
    assert rel(run(), gold["chain.final"]) < TOL_CHAIN
    full = run(full_state=True)
    assert rel(full[:, :U.LC], gold["chain.post"][:, :U.LC]) < TOL_CHAIN and rel(full[:, U.LC:], gold["chain.final"]) < TOL_CHAIN


# ------------------------------------------------------------------ bitwise
def test_chain_bitwise_properties(device, models):
    d = _diff(device, *models, 1000)
    cond = torch.rand((8, U.LC, U.F), generator=torch.Generator().manual_seed(21)).to(device)
    run = lambda c=cond, **kw: d.sample_compose_multibodies(c, 410, 2, 4, **{"seed": 31, "t_stop": 398, "full_state": True, **kw}).clone()
    a = run()
    assert bool(torch.isfinite(a).all())
    assert torch.equal(a, run(use_graph=False))                       # graph replay == plain stream
    assert torch.equal(a, run())                                      # the same seed twice
    assert not torch.equal(a, run(seed=32))
    lo, hi = run(cond[:4]), run(cond[4:], sample_offset=4)            # a batch of 8 == two batches of 4
    assert torch.equal(a[:4], lo) and torch.equal(a[4:], hi)
    info = d.last_chain_info()
    assert not info["recovered"] and info["chains_in_flight"] == 1


def test_timestep_range_split(device, models):
    """One library call over t = 409 .. 402 == two calls over 409 .. 406 and 405 .. 402 (the noise is keyed by (t, l), not by
    the position inside a call); odd and even iteration counts, graph and stream."""
    d = _diff(device, *models, 1000)
    x0 = torch.randn((5, U.HZ, U.F), generator=torch.Generator().manual_seed(22)).to(device)
    for L in (1, 3):
        for use_graph in (True, False):
            one = d._run_ula(x0.clone(), 409, 402, L, seed=7, sample_offset=3, use_graph=use_graph)
            two = d._run_ula(x0.clone(), 409, 406, L, seed=7, sample_offset=3, use_graph=use_graph)
            two = d._run_ula(two, 405, 402, L, seed=7, sample_offset=3, use_graph=use_graph)
            assert torch.equal(one, two), (L, use_graph)
            assert not torch.equal(one, x0)
    # and sample_step_ULA is the one-timestep form of the same chain
    scalar = U.scalar_for_gradient(U.linear_beta_schedule(1000))
    step = d.sample_step_ULA(x0, torch.tensor([409] * 5), 3, 4, 1000, scalar, seed=7, sample_offset=3)
    assert torch.equal(step, d._run_ula(x0.clone(), 409, 409, 3, seed=7, sample_offset=3))


def test_L0_is_the_401_step_chain(device, models):
    d = _diff(device, *models, 1000)
    cond = torch.rand((3, U.LC, U.F), generator=torch.Generator().manual_seed(23)).to(device)
    a = d.sample_compose_multibodies(cond, 1000, 0, 4, seed=41)
    b = d.sample_compose_multibodies(cond, 401, 0, 4, seed=41)
    assert bool(torch.isfinite(a).all()) and torch.equal(a, b)


def test_nan_in_state_reaches_the_output(device, models):
    """A NaN that enters the composed eps is not filtered by the update: the design that carries it comes back NaN."""
    d = _diff(device, *models, 1000)
    x = torch.randn((2, U.HZ, U.F), generator=torch.Generator().manual_seed(24))
    d._run_ula(x.to(device), 500, 500, 1, seed=1)                     # (a clean chain first: the range rule's one-time check is not what is tested)
    x[1, 7, 5] = float("nan")
    out = d._run_ula(x.to(device), 500, 500, 1, seed=1)
    assert bool(torch.isnan(out[1]).any())


# ------------------------------------------------------------------ recovery
def test_langevin_exchange_timeout_is_recovered_once(device):
    """dbg = 39 stands in for a partner workgroup kept off the chip (tests/test_gpu_paths.py::test_exchange_timeout_is_recovered):
    the Langevin chain is re-run once on the exchange-free kernels and equals what that selection computes by itself."""
    m8, _ = build_unet(device, U.HZ, 8)
    m4, _ = build_unet(device, U.HZ, 4)
    m8.set_option("auto_range", 0)
    d = _diff(device, m8, m4, 1000)
    cond = torch.rand((6, U.LC, U.F), generator=torch.Generator().manual_seed(25)).to(device)
    run = lambda: d.sample_compose_multibodies(cond, 404, 1, 4, seed=3, t_stop=401, full_state=True)
    m8.exchange_free(True)
    m4.exchange_free(True)
    ref = run().clone()
    m8.exchange_free(False)
    m4.exchange_free(False)
    assert m8.recovered == 0 and not d.last_chain_info()["recovered"]
    m8.set_option("dbg", 39)
    try:
        got = run()
        info = d.last_chain_info()
    finally:
        m8.set_option("dbg", 0)
    assert info["recovered"] and m8.recovered == 1 and m4.recovered == 1
    assert torch.equal(got, ref)
