"""GPU (MI355X): DDIM sampling of the 2-D airfoil path (GaussianDiffusion.ddim_sample, cindm_ddpm2d_sample_ddim) against a
CPU reference built from pinned oracle pieces -- model_predictions_2d (clip_x_start, rederive_pred_noise), ddim_coefs and
ddim_time_pairs with the three-line DDIM combine -- plus size-independent bitwise properties.

Tolerances as tests/test_gpu_parity_2d.py: single steps 2e-5, teacher-forced segments 1e-4."""
import pytest
import torch

import cindm_amd
import cindm_oracle as O
from test_gpu_parity_2d import build_unet2d, rel

pytestmark = pytest.mark.gpu

TOL_STEP = 2e-5
TOL_CHAIN = 1e-4
S = 50
B, NB, CH, HW = 2, 2, 21, 64
SHAPE = (B, NB, CH, HW, HW)


@pytest.fixture(scope="module")
def unet2d(device):
    return build_unet2d(device)


def _diff(unet2d, device, **kw):
    kw.setdefault("sampling_timesteps", S)
    return cindm_amd.GaussianDiffusion(unet2d[0], image_size=64, frames=6, cond_frames=2, timesteps=1000, loss_type="l2",
                                       **kw).to(device)


def _tape(seed, steps, shape=SHAPE):
    """x_T and per-DDIM-step noise as sample_noise draws it: state [.., B, 1, C-3, H, W], boundary [.., B, nb, 3, H, W]."""
    b, nb, c, h, w = shape
    g = torch.Generator().manual_seed(seed)
    init = (torch.randn((b, 1, c - 3, h, w), generator=g), torch.randn((b, nb, 3, h, w), generator=g))
    return cindm_amd.NoiseTape2D(init, torch.randn((steps, b, 1, c - 3, h, w), generator=g),
                                 torch.randn((steps, b, nb, 3, h, w), generator=g))


def _oracle(od, x, i0, i1, tape, eta, shape=SHAPE):
    """DDIM steps i0 .. i1-1 of an S-step schedule from x [B, nb, C, H, W]; tape.step_* rows indexed by the DDIM step."""
    b, nb, c, h, w = shape
    pairs = O.ddim_time_pairs(od.num_timesteps, S)
    img = x.reshape(b * nb, c, h, w)
    for i in range(i0, i1):
        t, tn = pairs[i]
        eps, x0 = O.model_predictions_2d(od, shape, img, t, clip_x_start=True, rederive_pred_noise=True)
        if tn < 0:
            img = x0
            continue
        san, cc, sg = O.ddim_coefs(od, t, tn, eta)
        z = O.sample_noise_2d(tape.step_state[i], tape.step_boundary[i]).reshape(b * nb, c, h, w)
        img = x0 * san + cc * eps + sg * z
    return img.reshape(shape)


def test_ddim2d_sample_runs(device, unet2d):
    """sample() with sampling_timesteps < timesteps: the DDIM chain (NotImplementedError before it was built)."""
    d = _diff(unet2d, device, sampling_timesteps=250)
    out = d.sample(batch_size=2, num_boundaries=2)
    assert out.shape == (2, 2, 21, 64, 64)
    assert bool(torch.isfinite(out).all())
    assert torch.equal(out[:, 0, :-3], out[:, 1, :-3])


@pytest.mark.parametrize("obj,avg,etas", [("pred_noise", True, (0.0, 0.5)), ("pred_noise", False, (0.0, 0.5)),
                                          ("pred_x0", True, (0.5,)), ("pred_v", True, (0.5,))])
def test_ddim2d_single_steps_vs_oracle(device, unet2d, obj, avg, etas):
    """One DDIM step (the first two pairs, a middle pair and the last pair, t_next = -1) from a given state, with tape noise."""
    sd = unet2d[1]
    od = O.Diffusion2D(sd, image_size=64, frames=6, objective=obj, use_average_share=avg)
    g = torch.Generator().manual_seed(31)
    x = torch.randn(SHAPE, generator=g)
    x[:, 1, :-3] = x[:, 0, :-3]                  # a state the chain can reach: the state channels shared over the boundaries
    for eta in etas:
        d = _diff(unet2d, device, objective=obj, use_average_share=avg, ddim_sampling_eta=eta)
        tape = _tape(7, S)
        pairs = O.ddim_time_pairs(1000, S)
        for i in (1, S // 2, S - 1, 0):
            ref = _oracle(od, x, i, i + 1, tape, eta)
            out = d.ddim_sample(SHAPE, noise=tape, init_img=x.to(device), step_range=(i, i + 1))
            # the first pair (t = 999): an unclamped x_start entry carries the U-Net's error times sqrt_recipm1[999] = 1.8e3 into
            # x0 * sqrt(alpha_next) (as the x_start tolerance of tests/test_gpu_parity_2d.py::test_step2d_golden)
            t, tn = pairs[i]
            amp = max(1.0, float(d.sqrt_recipm1_alphas_cumprod[t] * d.alphas_cumprod[tn].sqrt())) if i == 0 and obj == "pred_noise" else 1.0
            assert rel(out, ref) < TOL_STEP * amp, (obj, avg, eta, i)


def test_ddim2d_teacher_forced_segments(device, unet2d):
    """Segments of the S = 50 chain against the oracle loop: the first 5 steps from the tape's x_T (eta = 0) and the last 3 from
    a given state (eta = 0.5, tape noise)."""
    od = O.Diffusion2D(unet2d[1], image_size=64, frames=6)
    tape = _tape(11, S)
    x_T = O.sample_noise_2d(*tape.init)
    out = _diff(unet2d, device).ddim_sample(SHAPE, noise=tape, step_range=(0, 5))
    assert rel(out, _oracle(od, x_T, 0, 5, tape, 0.0)) < TOL_CHAIN
    x = torch.randn(SHAPE, generator=torch.Generator().manual_seed(12)) * 0.6
    x[:, 1, :-3] = x[:, 0, :-3]
    out = _diff(unet2d, device, ddim_sampling_eta=0.5).ddim_sample(SHAPE, noise=tape, init_img=x.to(device), step_range=(S - 3, S))
    assert rel(out, _oracle(od, x, S - 3, S, tape, 0.5)) < TOL_CHAIN


@pytest.fixture(scope="module")
def ddim_eta(device, unet2d):
    return _diff(unet2d, device, ddim_sampling_eta=0.5)


def test_ddim2d_graph_equals_plain(ddim_eta):
    a = ddim_eta.sample(batch_size=2, num_boundaries=2, seed=21)
    b = ddim_eta.sample(batch_size=2, num_boundaries=2, seed=21, use_graph=False)
    assert torch.equal(a, b)


def test_ddim2d_seed_repeatable(ddim_eta):
    a = ddim_eta.sample(batch_size=2, num_boundaries=2, seed=5)
    assert torch.equal(a, ddim_eta.sample(batch_size=2, num_boundaries=2, seed=5))
    assert not torch.equal(a, ddim_eta.sample(batch_size=2, num_boundaries=2, seed=6))


def test_ddim2d_batch_partition_invariance(ddim_eta):
    """Designs are independent: designs [0, 4) in one run equal [0, 2) and [2, 4) with sample_offset (x_T and the sigma > 0 draws)."""
    full = ddim_eta.sample(batch_size=4, num_boundaries=2, seed=3)
    lo = ddim_eta.sample(batch_size=2, num_boundaries=2, seed=3, sample_offset=0)
    hi = ddim_eta.sample(batch_size=2, num_boundaries=2, seed=3, sample_offset=2)
    assert torch.equal(full[:2], lo) and torch.equal(full[2:], hi)


@pytest.mark.parametrize("avg", [True, False], ids=["mean", "sum"])
def test_ddim2d_states_shared_over_boundaries(device, unet2d, avg):
    """After a full chain the state channels of all boundary copies of a design are identical; the boundary channels are not."""
    d = _diff(unet2d, device, ddim_sampling_eta=0.5, use_average_share=avg)
    out = d.sample(batch_size=2, num_boundaries=3, seed=9)
    assert bool(torch.isfinite(out).all())
    assert torch.equal(out[:, 0, :-3], out[:, 1, :-3]) and torch.equal(out[:, 0, :-3], out[:, 2, :-3])
    assert not torch.equal(out[:, 0, -3:], out[:, 1, -3:])


def test_ddim2d_refusals_on_device(device, unet2d):
    d = _diff(unet2d, device)
    with pytest.raises(NotImplementedError):
        d.sample(batch_size=1, num_boundaries=2, design_fn=lambda x: torch.zeros_like(x))
    with pytest.raises(NotImplementedError):
        d.sample(batch_size=1, num_boundaries=2, return_all_timesteps=True)
    with pytest.raises(NotImplementedError):
        _diff(unet2d, device, share_noise=False).sample(batch_size=1, num_boundaries=2)
