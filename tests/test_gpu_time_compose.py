"""GPU (MI355X): the parallel time composition (GaussianDiffusion1D.composing_time_sample, cindm_ddpm1d_sample_timecompose)
against the reference's own run (tests/golden/time_compose_parallel.npz: same noise draws, the state after EVERY step), its
bitwise identity with ddim_sample on segment 0, size-independent bitwise properties, the per-step hand-over restated on the
public model_predictions, a batch past the level-pair plan, the time-out recovery and the recorder.

Tolerances as tests/test_gpu_parity.py: one step 2e-5, free-running chains 1e-4."""
import pytest
import torch

import cindm_amd
from cindm_amd.diffusion1d import autoregress_segment_seeds
from test_gpu_parity import TOL_CHAIN, TOL_STEP, build_unet, rel
from test_time_compose_host import B, CASES, F, load_case

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


def _cond(n, Lc, seed):
    return (torch.rand((n, Lc, 8), generator=torch.Generator().manual_seed(seed)) - 0.5)


# ------------------------------------------------------------------ against the reference
@pytest.mark.parametrize("tag", sorted(CASES))
def test_time_compose_golden(gold_dir, device, unet24, unet8h, tag):
    """Both returned tensors and the state after every step (return_trajectory_every=1: unclamped between steps, so the clamp
    of the last step hides nothing) within TOL_CHAIN of the reference's run on the same tapes."""
    hz, Lc, R, K, S, eta = CASES[tag]
    g = load_case(gold_dir, tag)
    d = _diff((unet24 if hz == 24 else unet8h)[0], device, Lc, R, S, eta)
    tape = cindm_amd.NoiseTape(g["init"], g["step"])
    (img, inf), rec = d.composing_time_sample((B, R, F), g["cond"].to(device), n_composed=K - 1, noise=tape, return_trajectory_every=1)
    assert tuple(img.shape) == (B, R, F) and tuple(inf.shape) == tuple(g["img_infered"].shape) == (B, (K - 1) * min(20, R), F)
    assert rec.step == list(range(1, S + 1)) and tuple(rec.x.shape) == (S, K, B, R, F)
    errs = [rel(rec.x[i], g["states"][i]) for i in range(S)]
    print(tag, "img", rel(img, g["img"]), "img_infered", rel(inf, g["img_infered"]), "states", errs)
    assert rel(img, g["img"]) < TOL_CHAIN and rel(inf, g["img_infered"]) < TOL_CHAIN, tag
    for i in range(S):
        assert errs[i] < TOL_CHAIN, (tag, i, errs[i])


# ------------------------------------------------------------------ bitwise: segment 0 is ddim_sample
@pytest.mark.parametrize("eta", [0.0, 1.0])
def test_segment0_is_ddim_sample(device, unet24, eta):
    """Segment 0 keeps the caller's cond and draws under seed_0 = seed: it is ddim_sample's chain, bit for bit.  (With
    conditioned_steps > 0 ddim_sample runs the stand-alone update kernel, so this compares two stand-alone updates.)"""
    d = _diff(unet24[0], device, 4, 20, 10, eta)
    cond = _cond(5, 4, 21).to(device)
    for off in (0, 9):
        img, inf = d.composing_time_sample((5, 20, 8), cond, seed=1234, sample_offset=off)
        want = d.ddim_sample((5, 20, 8), cond, seed=autoregress_segment_seeds(1234, 3)[0], sample_offset=off)
        assert d.last_step_info()[1] is False
        assert torch.equal(img, want), (eta, off)
        assert tuple(inf.shape) == (5, 40, 8) and bool(torch.isfinite(inf).all())


def test_time_compose_bitwise_properties(device, unet24):
    d = _diff(unet24[0], device, 4, 20, 12, 1.0)
    cond = _cond(16, 4, 22).to(device)
    run = lambda c=cond, **kw: torch.cat(d.composing_time_sample((c.shape[0], 20, 8), c, **{"seed": 77, **kw}), dim=1).clone()
    a = run()                                 # [16, 3 * 20, 8]: segment k at rows 20 k .. 20 (k + 1)
    assert tuple(a.shape) == (16, 60, 8) and bool(torch.isfinite(a).all())
    assert torch.equal(a, run(use_graph=False))
    assert torch.equal(a, run())
    b = run(seed=78)
    for k in range(3):                        # every segment depends on the seed
        assert not torch.equal(a[:, 20 * k:20 * (k + 1)], b[:, 20 * k:20 * (k + 1)]), k
    lo, hi = run(cond[:6], sample_offset=0), run(cond[6:], sample_offset=6)
    assert torch.equal(a[:6], lo) and torch.equal(a[6:], hi)
    assert float(a.abs().max()) <= 1.0 + 1e-5             # every segment ends on the clamped x_start


# ------------------------------------------------------------------ the hand-over, step by step
def test_handover_reads_the_current_noisy_state(device, unet24):
    """Record i is the state after step i: the state whose tails the hand-over of step i + 1 reads.  Step i + 1 of segment k
    restated on the public model_predictions -- the state rec.x[i][k], conditioned on the last Lc rows of rec.x[i][k - 1]
    (assembled in torch), the DDIM update in torch on the call's own tape -- must give rec.x[i + 1][k] within TOL_STEP.  A
    hand-over from a state one step older, from the final state, or to the wrong segment is orders of magnitude outside that."""
    K, n, R, Lc, S, eta = 4, 5, 20, 4, 5, 0.5
    d = _diff(unet24[0], device, Lc, R, S, eta)
    g = torch.Generator().manual_seed(23)
    cond = _cond(n, Lc, 23).to(device)
    tape = cindm_amd.NoiseTape(torch.randn((K, n, R, 8), generator=g), torch.randn((S, K, n, R, 8), generator=g))
    _, rec = d.composing_time_sample((n, R, 8), cond, n_composed=K - 1, noise=tape, return_trajectory_every=1)
    times, coefs = d.ddim_schedule()
    step = tape.step.to(device)
    assert float(rec.x[:-1].abs().max()) > 1.0             # the states in between are noisy, not clamped
    for i in range(S - 1):
        for k in (1, K - 1):
            c = rec.x[i][k - 1][:, R - Lc:].contiguous()
            eps, x0 = d.model_predictions(rec.x[i][k].contiguous(), c, times[i + 1], clip_x_start=True)
            san, cc, sg = (float(v) for v in coefs[i + 1])
            want = x0 if times[i + 2] < 0 else x0 * san + cc * eps + sg * step[i + 1, k]
            e = rel(rec.x[i + 1][k], want)
            print("step", i + 1, "segment", k, e)
            assert e < TOL_STEP, (i, k, e)
            if i == 0 and k == 1:             # the check can tell: the caller's cond in place of the hand-over is far outside
                eps2, x02 = d.model_predictions(rec.x[i][k].contiguous(), cond, times[i + 1], clip_x_start=True)
                assert rel(rec.x[i + 1][k], x02 * san + cc * eps2 + sg * step[i + 1, k]) > 100 * TOL_STEP


def test_multibody_prediction(device, unet24):
    """With model_unconditioned set the step composes six pair predictions and four single-body ones (gradient(), n_bodies = 4):
    segment 0 is still ddim_sample bit for bit, and a later segment's step is the public prediction on the handed-over tail."""
    single = build_unet(device, 24, 4)[0]
    n, R, Lc, S = 3, 20, 4, 4
    d = _diff(unet24[0], device, Lc, R, S, 1.0)
    d.model_unconditioned = single
    cond = (torch.rand((n, Lc, 16), generator=torch.Generator().manual_seed(27)) - 0.5).to(device)
    (img, inf), rec = d.composing_time_sample((n, R, 16), cond, n_composed=1, seed=41, sample_offset=2, return_trajectory_every=1)
    assert tuple(inf.shape) == (n, 20, 16) and bool(torch.isfinite(inf).all())
    assert torch.equal(img, d.ddim_sample((n, R, 16), cond, seed=41, sample_offset=2))
    times, _ = d.ddim_schedule()
    _, x0 = d.model_predictions(rec.x[S - 2][1].contiguous(), rec.x[S - 2][0][:, R - Lc:].contiguous(), times[S - 1], clip_x_start=True)
    assert rel(rec.x[S - 1][1], x0) < TOL_STEP          # (the last step returns x_start)


# ------------------------------------------------------------------ a wider plan
def test_rows_past_the_level_pair_plan(device, unet24):
    """3 x 110 = 330 rows run the U-Net's plan for more than 320 rows: finite, and a design's result is the one the 15-row
    chain computes for it."""
    d = _diff(unet24[0], device, 4, 20, 3, 1.0)
    cond = _cond(110, 4, 24).to(device)
    img, inf = d.composing_time_sample((110, 20, 8), cond, seed=5)
    assert bool(torch.isfinite(img).all()) and bool(torch.isfinite(inf).all())
    img5, inf5 = d.composing_time_sample((5, 20, 8), cond[:5], seed=5)
    assert torch.equal(img[:5], img5) and torch.equal(inf[:5], inf5)


# ------------------------------------------------------------------ recovery and recording
def test_exchange_timeout_is_recovered_once(device):
    """dbg = 39 stands in for a partner workgroup kept off the chip (tests/test_gpu_paths.py::test_exchange_timeout_is_recovered):
    the whole chain is re-run once on the exchange-free kernels and equals what that selection computes by itself."""
    m, _ = build_unet(device, 24, 8)
    m.set_option("auto_range", 0)
    d = _diff(m, device, 4, 20, 4, 0.5)
    cond = _cond(16, 4, 25).to(device)
    run = lambda: torch.cat(d.composing_time_sample((16, 20, 8), cond, n_composed=1, seed=3), dim=1).clone()
    m.exchange_free(True)
    ref = run()
    m.exchange_free(False)
    assert m.recovered == 0
    m.set_option("dbg", 39)
    try:
        got = run()
        info = d.last_chain_info()
    finally:
        m.set_option("dbg", 0)
    assert info["recovered"] and m.recovered == 1
    assert torch.equal(got, ref)


def test_recorded_call_returns_the_same_designs(device, unet24):
    d = _diff(unet24[0], device, 4, 20, 7, 1.0)
    cond = _cond(5, 4, 26).to(device)
    img, inf = d.composing_time_sample((5, 20, 8), cond, seed=9)
    (img_r, inf_r), rec = d.composing_time_sample((5, 20, 8), cond, seed=9, return_trajectory_every=3, trajectory=("x", "x0"))
    assert torch.equal(img, img_r) and torch.equal(inf, inf_r)
    assert rec.step == [3, 6, 7] and tuple(rec.x.shape) == tuple(rec.x0.shape) == (3, 3, 5, 20, 8)
    # the last record is the result; the last step returns its x_start
    assert torch.equal(rec.x[-1][0], img) and torch.equal(rec.x[-1][1], inf[:, :20]) and torch.equal(rec.x[-1][2], inf[:, 20:])
    assert torch.equal(rec.x0[-1], rec.x[-1]) and float(rec.x0.abs().max()) <= 1.0
