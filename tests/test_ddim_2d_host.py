"""The 2-D DDIM sampler's host side (no GPU): the schedule, the refusals and the CPU refusal of sampling."""
import pytest
import torch

import cindm_amd
import cindm_oracle as O


def _diffusion(**kw):
    sd = O.synth_state_dict_2d(O.unet2d_param_shapes(64, (1, 2), 21), 0)
    m = cindm_amd.Unet(dim=64, dim_mults=(1, 2), channels=21)
    m.load_state_dict(sd, strict=True)
    return cindm_amd.GaussianDiffusion(m, image_size=64, frames=6, timesteps=1000, **kw)


@pytest.mark.parametrize("S,eta", [(250, 0.0), (100, 0.5), (7, 1.0)])
def test_ddim2d_schedule(S, eta):
    d = _diffusion(sampling_timesteps=S, ddim_sampling_eta=eta)
    assert d.is_ddim_sampling
    times, coefs = d.ddim_schedule()
    assert len(times) == S + 1 and times[-1] == -1 and times[0] == 999
    assert all(a > b for a, b in zip(times[:-1], times[1:]))
    assert list(zip(times[:-1], times[1:])) == O.ddim_time_pairs(1000, S)
    assert coefs.shape == (S, 3) and coefs.dtype == torch.float32 and bool(torch.isfinite(coefs).all())
    od = O.Diffusion2D(O.synth_state_dict_2d(O.unet2d_param_shapes(64, (1, 2), 21), 0), image_size=64, frames=6)
    for i, (t, tn) in enumerate(zip(times[:-2], times[1:-1])):        # (the last pair's coefficients are not used)
        ref = torch.stack(O.ddim_coefs(od, t, tn, eta))
        assert torch.equal(coefs[i], ref), (i, t, tn)


def test_ddim2d_sample_on_cpu_raises_cindm_error():
    d = _diffusion(sampling_timesteps=250)
    with pytest.raises(cindm_amd.CindmError):
        d.sample(batch_size=2, num_boundaries=2)


def test_ddim2d_refusals():
    d = _diffusion(sampling_timesteps=50)
    with pytest.raises(NotImplementedError, match="design_fn"):
        d.sample(batch_size=1, num_boundaries=2, design_fn=lambda x: torch.zeros_like(x))
    with pytest.raises(NotImplementedError, match="return_all_timesteps"):
        d.sample(batch_size=1, num_boundaries=2, return_all_timesteps=True)
    with pytest.raises(NotImplementedError, match="share_noise"):
        _diffusion(sampling_timesteps=50, share_noise=False).sample(batch_size=1, num_boundaries=2)
