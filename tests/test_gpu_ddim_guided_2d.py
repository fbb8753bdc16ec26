"""GPU (MI355X): guided DDIM of the 2-D airfoil path with the library's own objective (GaussianDiffusion.ddim_sample with
design_fn = ForceObjective under "standard-alpha"; cindm_ddpm2d_sample_ddim_force, ddim2d_guided_update_kernel) against the CPU
oracle's pieces -- model_predictions_2d, ddim_coefs, airfoil_design_grad -- and the bitwise properties that tie it to the
unguided DDIM chain, the per-step loop and the guided DDPM chain.

Tolerances: single guided steps 2e-5 (the surrogate-gradient bound of tests/test_gpu_force.py), fused against the per-step loop
1e-6 (the DDPM twin's bound, test_guided_chain_fused_equals_loop)."""
import pytest
import torch

import cindm_amd
import cindm_oracle as O
from test_gpu_parity_2d import build_unet2d, rel

pytestmark = pytest.mark.gpu

TOL = 2e-5
CH, HW, FRAMES = 21, 64, 6
PMIN, PMAX = -37.7, 57.6
STEPS = (0, 24, 49)               # of S = 50: the first pair (t = 999), a middle one, the last (t_next = -1)


@pytest.fixture(scope="module")
def unet2d(device):
    return build_unet2d(device)


@pytest.fixture(scope="module")
def force(device):
    sd = O.synth_state_dict_2d(O.force_unet_param_shapes(), 7)
    m = cindm_amd.ForceUnet(dim=64, dim_mults=(1, 2, 4, 8), channels=4)
    m.load_state_dict(sd, strict=True)
    return m.to(device), sd


def _diff(unet2d, device, S, **kw):
    kw.setdefault("coeff_ratio", 0.05)
    return cindm_amd.GaussianDiffusion(unet2d[0], image_size=64, frames=FRAMES, cond_frames=2, timesteps=1000, loss_type="l2",
                                       sampling_timesteps=S, **kw).to(device)


def _objective(force, B, nb):
    return cindm_amd.ForceObjective(force[0], B, nb, FRAMES, p_min=PMIN, p_max=PMAX)


def _tape(seed, steps, shape):
    b, nb, c, h, w = shape
    g = torch.Generator().manual_seed(seed)
    init = (torch.randn((b, 1, c - 3, h, w), generator=g), torch.randn((b, nb, 3, h, w), generator=g))
    return cindm_amd.NoiseTape2D(init, torch.randn((steps, b, 1, c - 3, h, w), generator=g),
                                 torch.randn((steps, b, nb, 3, h, w), generator=g))


def _shared(x):
    """True when the state channels of every boundary copy of a design equal copy 0's, bit for bit."""
    return all(torch.equal(x[:, 0, :-3], x[:, k, :-3]) for k in range(1, x.shape[1]))


@pytest.fixture(scope="module")
def oracle_steps(unet2d, force):
    """Per teacher-forced step i of the S = 50 schedule: the input state and the oracle's (pred_noise, x_start, design gradient)
    there -- computed once; ddim_sampling_eta only enters the three-line combine."""
    shape = (1, 2, CH, HW, HW)
    od = O.Diffusion2D(unet2d[1], image_size=64, frames=FRAMES, coeff_ratio=0.05)
    pairs = O.ddim_time_pairs(1000, 50)
    gen = torch.Generator().manual_seed(41)
    out = {}
    for i in STEPS:
        x = torch.randn(shape, generator=gen) * (1.0 if i == 0 else 0.6)
        x[:, 1, :-3] = x[:, 0, :-3]                  # a state the chain can reach: the state channels shared over the boundaries
        img = x.reshape(2, CH, HW, HW)
        eps, x0 = O.model_predictions_2d(od, shape, img, pairs[i][0], clip_x_start=True, rederive_pred_noise=True)
        g = O.airfoil_design_grad(force[1], img, 1, 2, FRAMES, PMIN, PMAX)
        out[i] = (x, eps, x0, g)
    return od, pairs, out


@pytest.mark.parametrize("eta", [0.0, 0.5])
def test_guided_ddim2d_teacher_forced_steps_vs_oracle(device, unet2d, force, oracle_steps, eta):
    """One guided DDIM step from a given state, tape noise: the oracle's unguided update minus w_i times the oracle's design
    gradient at the step's input state.  On an MI355X: 1.97e-5 / 1.89e-5 at the first pair (eta 0 / 0.5; t = 999 carries the
    U-Net's error times sqrt_recipm1[999] * sqrt(alpha_979) through the unclamped x_start entries -- the flat bound holds
    narrowly there), 7.6e-8 at t = 519, 1.8e-7 at the last pair, where the shift is 2.8e-3 of the state."""
    od, pairs, pieces = oracle_steps
    shape = (1, 2, CH, HW, HW)
    d = _diff(unet2d, device, 50, ddim_sampling_eta=eta)
    fn = _objective(force, 1, 2)
    tape = _tape(7, 50, shape)
    w = d.ddim_guidance_weights()
    eta_tab = (d.coeff_ratio * d.betas.flip(0)).double().cpu()
    for i in STEPS:
        t, tn = pairs[i]
        x, eps, x0, g = pieces[i]
        assert float(w[i]) == float(eta_tab[tn + 1:t + 1].sum().float())
        if tn < 0:
            plain = x0
        else:
            san, cc, sg = O.ddim_coefs(od, t, tn, eta)
            z = O.sample_noise_2d(tape.step_state[i], tape.step_boundary[i]).reshape(2, CH, HW, HW)
            plain = x0 * san + cc * eps + sg * z
        ref = (plain - w[i] * g).reshape(shape)
        out = d.ddim_sample(shape, design_fn=fn, design_guidance="standard-alpha", init_img=x.to(device), step_range=(i, i + 1), noise=tape)
        unguided = d.ddim_sample(shape, init_img=x.to(device), step_range=(i, i + 1), noise=tape)
        r = rel(out, ref)
        print(f"guided DDIM step eta={eta} i={i} t={t} t_next={tn}: rel {r:.3e}, shift / state {float((w[i] * g).abs().max() / ref.abs().max()):.3e}")
        assert r < TOL, (eta, i, r)
        assert not torch.equal(out, unguided)


def test_guided_ddim2d_fused_equals_loop_equals_eager(device, unet2d, force):
    shape = (2, 2, CH, HW, HW)
    d = _diff(unet2d, device, 250, ddim_sampling_eta=0.5)
    fn = _objective(force, 2, 2)
    tape = _tape(31, 5, shape)
    kw = dict(design_fn=fn, design_guidance="standard-alpha", noise=tape, step_range=(0, 5))
    fused = d.ddim_sample(shape, **kw)
    loop = d.ddim_sample(shape, fused=False, **kw)
    eager = d.ddim_sample(shape, use_graph=False, **kw)
    assert bool(torch.isfinite(fused).all())
    r = rel(fused, loop)
    print(f"fused vs per-step loop: rel {r:.3e}")
    assert r < 1e-6
    assert torch.equal(fused, eager)
    assert not torch.equal(fused, d.ddim_sample(shape, noise=tape, step_range=(0, 5)))


def test_guided_ddim2d_zero_weight_is_the_unguided_chain(device, unet2d, force):
    """coeff_ratio = 0: every weight is 0, and the guided chain is the unguided one bit for bit -- the same x_T, the same draws
    (counter-based, sigma > 0) and the same update."""
    shape = (1, 2, CH, HW, HW)
    d = _diff(unet2d, device, 250, ddim_sampling_eta=0.5, coeff_ratio=0.0)
    assert not bool(d.ddim_guidance_weights().any())
    guided = d.ddim_sample(shape, design_fn=_objective(force, 1, 2), design_guidance="standard-alpha", seed=11, step_range=(0, 5))
    plain = d.ddim_sample(shape, seed=11, step_range=(0, 5))
    assert bool(torch.isfinite(guided).all()) and torch.equal(guided, plain)


def test_guided_ddim2d_state_sharing_as_the_guided_ddpm_chain(device, unet2d, force):
    """The update shares the PREDICTION over the boundary copies of a design, not the state: after guided steps the copies' state
    channels are identical exactly when the gradient's state channels are.  Whatever the guided DDPM chain does with the same
    models, objective and seed (three boundaries, three steps), the guided DDIM chain does too."""
    shape = (1, 3, CH, HW, HW)
    fn = _objective(force, 1, 3)
    ddpm = _diff(unet2d, device, 1000).p_sample_loop(shape, design_fn=fn, design_guidance="standard-alpha", seed=9, t_stop=997)
    ddim = _diff(unet2d, device, 250, ddim_sampling_eta=0.5).ddim_sample(shape, design_fn=fn, design_guidance="standard-alpha", seed=9,
                                                                         step_range=(0, 3))
    assert bool(torch.isfinite(ddpm).all()) and bool(torch.isfinite(ddim).all())
    print(f"state channels shared bit for bit: DDPM {_shared(ddpm)}, DDIM {_shared(ddim)}")
    assert _shared(ddim) == _shared(ddpm)
    assert not torch.equal(ddim[:, 0, -3:], ddim[:, 1, -3:])


def test_guided_ddim2d_batch_independence(device, unet2d, force):
    """A guided design does not depend on its batch (the sharding contract of cindm_amd.dist.sample2d_sharded): designs 0 and 1
    of a two-design run equal the one-design runs at sample_offset 0 and 1, bit for bit."""
    d = _diff(unet2d, device, 250, ddim_sampling_eta=0.5)
    kw = dict(design_guidance="standard-alpha", seed=3, step_range=(0, 3))
    full = d.ddim_sample((2, 2, CH, HW, HW), design_fn=_objective(force, 2, 2), **kw)
    fn1 = _objective(force, 1, 2)
    lo = d.ddim_sample((1, 2, CH, HW, HW), design_fn=fn1, sample_offset=0, **kw)
    hi = d.ddim_sample((1, 2, CH, HW, HW), design_fn=fn1, sample_offset=1, **kw)
    assert bool(torch.isfinite(full).all())
    assert torch.equal(full[:1], lo) and torch.equal(full[1:], hi)
    assert not torch.equal(lo, hi)


def test_guided_ddim2d_exchange_timeout_is_recovered(device, unet2d):
    """The surrogate's exchange time-out inside the guided DDIM chain (option `dbg` = 39 makes slab 1 of every image never publish,
    as in test_gpu_force.py::test_surrogate_exchange_timeout_is_recovered): the entry keeps x_T, reads the error word at the
    end and re-runs the chain once on the exchange-free derivative -- the result IS that derivative's chain."""
    sd = O.synth_state_dict_2d(O.force_unet_param_shapes(), 7)

    def model():
        m = cindm_amd.ForceUnet(dim=64, dim_mults=(1, 2, 4, 8), channels=4)
        m.load_state_dict(sd, strict=True)
        return m.to(device)

    shape = (1, 2, CH, HW, HW)
    d = _diff(unet2d, device, 250, ddim_sampling_eta=0.5)
    tape = _tape(31, 3, shape)
    kw = dict(design_guidance="standard-alpha", noise=tape, step_range=(0, 3))
    ref = model().set_option("gn_bwd_fused", 1)                     # the exchange-free derivative, selected up front
    want = d.ddim_sample(shape, design_fn=cindm_amd.ForceObjective(ref, 1, 2, FRAMES, p_min=PMIN, p_max=PMAX), **kw)
    m = model()
    m.set_option("dbg", 39)
    before = m.recovered
    got = d.ddim_sample(shape, design_fn=cindm_amd.ForceObjective(m, 1, 2, FRAMES, p_min=PMIN, p_max=PMAX), **kw)
    m.set_option("dbg", 0)
    assert m.recovered == before + 1 and bool(torch.isfinite(got).all()) and torch.equal(got, want)
