"""The autoregressive time composition's host side (no GPU): the refusals, the segment count, the segment-seed rule, and a CPU
restatement of the rollout on cindm_oracle.ddim_sample pinned against the reference's own output
(tests/golden/autoregress_1d.npz, tests/manual/make_golden_autoregress.py)."""
import os

import numpy as np
import pytest
import torch

import cindm_amd
import cindm_oracle as O
from cindm_amd.diffusion1d import autoregress_segment_seeds, autoregress_segments

# tag: (horizon, Lc, R, n_composed, single_step, prediction_steps, S, eta, B) -- tests/manual/make_golden_autoregress.py
CASES = {"a": (24, 4, 20, 2, False, 40, 8, 0.0, 2), "b": (24, 4, 20, 1, False, 40, 8, 0.5, 2), "c": (8, 4, 4, 0, True, 12, 8, 0.0, 2)}


def _diffusion(hz=24, Lc=4, R=20, **kw):
    m = cindm_amd.TemporalUnet1D(hz, 8, False, attention=True)
    return cindm_amd.GaussianDiffusion1D(m, image_size=R, conditioned_steps=Lc, timesteps=1000, loss_type="l1", **kw)


def test_segment_count():
    assert autoregress_segments(4, 20, 0) == 1
    assert autoregress_segments(4, 20, 1) == 2
    assert autoregress_segments(4, 20, 5) == 6
    # single-step: ceil(P / Lc) segments, the default script shape (horizon 8, Lc = R = 4, P = 40) gives 10
    assert autoregress_segments(4, 4, 1, True, 40) == 10
    assert autoregress_segments(4, 4, 7, True, 12) == 3
    assert autoregress_segments(2, 2, 0, True, 6) == 3


def test_refusals_carry_the_reason():
    with pytest.raises(NotImplementedError, match="conditioned_steps == 0"):
        autoregress_segments(0, 24, 1)
    with pytest.raises(NotImplementedError, match="rollout_steps .* < conditioned_steps"):
        autoregress_segments(4, 2, 1)
    with pytest.raises(ValueError, match="slice assignment"):
        autoregress_segments(4, 20, 1, True, 40)          # ceil(40 / 4) * 20 != 40
    with pytest.raises(ValueError, match="slice assignment"):
        autoregress_segments(4, 4, 1, True, 10)           # ceil(10 / 4) * 4 = 12 != 10
    with pytest.raises(ValueError, match="n_composed"):
        autoregress_segments(4, 20, -1)


def test_method_refuses_before_any_device_check():
    """Every refusal comes from the CPU-resident object, ahead of the CindmError of the missing device."""
    d0 = _diffusion(Lc=0, R=24)
    with pytest.raises(NotImplementedError, match="conditioned_steps == 0"):
        d0.autoregress_time_compose_sample(2, torch.zeros(2, 0, 8), 1)
    d = _diffusion()
    with pytest.raises(ValueError, match="conditioned_steps = 4"):
        d.autoregress_time_compose_sample(2, torch.zeros(2, 3, 8), 1)
    with pytest.raises(ValueError, match="slice assignment"):
        d.autoregress_time_compose_sample(2, torch.zeros(2, 4, 8), 1, is_single_step_prediction=True, prediction_steps=40)
    d_short = _diffusion(hz=6, Lc=4, R=2)
    with pytest.raises(NotImplementedError, match="rollout_steps"):
        d_short.autoregress_time_compose_sample(2, torch.zeros(2, 4, 8), 1)


def test_cpu_tensors_raise_cindm_error():
    d = _diffusion(sampling_timesteps=8)
    with pytest.raises(cindm_amd.CindmError):
        d.autoregress_time_compose_sample(2, torch.zeros(2, 4, 8), 1, seed=0)


def test_segment_seed_rule():
    for seed in (0, 1, 12345, 2 ** 62 - 1, 2 ** 64 - 1):
        s = autoregress_segment_seeds(seed, 12)
        assert s[0] == seed % 2 ** 64
        assert len(set(s)) == 12
        assert all(0 <= v < 2 ** 64 for v in s)
        assert s == [(seed + k * 0x9E3779B97F4A7C15) % 2 ** 64 for k in range(12)]
    assert autoregress_segment_seeds(7, 1) == [7]


def _restated_rollout(od, cond, init, step, S, eta):
    """Segment k = cindm_oracle.ddim_sample on the segment's tape, conditioned on cond (k = 0) or on the previous segment's tail."""
    segs, c = [], cond
    for k in range(init.shape[0]):
        img = O.ddim_sample(od, tuple(init[k].shape), c, {"init": init[k], "step": step[k]}, sampling_timesteps=S, eta=eta)
        segs.append(img)
        c = img[:, -od.conditioned_steps:]
    return torch.stack(segs), torch.cat(segs, dim=1)


@pytest.mark.parametrize("tag", sorted(CASES))
def test_restatement_reproduces_reference_golden(gold_dir, tag):
    g = np.load(os.path.join(gold_dir, "autoregress_1d.npz"))
    hz, Lc, R, n_composed, single, P, S, eta, B = CASES[tag]
    K = autoregress_segments(Lc, R, n_composed, single, P)
    init, step = torch.from_numpy(g[f"{tag}.init"]), torch.from_numpy(g[f"{tag}.step"])
    assert tuple(init.shape) == (K, B, R, 8) and tuple(step.shape) == (K, S, B, R, 8)
    assert tuple(g[f"{tag}.out"].shape) == (B, K * R, 8)
    sd = O.synth_state_dict(O.unet1d_param_shapes(hz, 8), seed=0)
    od = O.Diffusion1D(sd, image_size=R, conditioned_steps=Lc)
    seg, out = _restated_rollout(od, torch.from_numpy(g[f"{tag}.cond"]), init, step, S, eta)
    ref_seg, ref_out = torch.from_numpy(g[f"{tag}.seg"]), torch.from_numpy(g[f"{tag}.out"])
    scale = float(ref_out.abs().max())
    assert float((seg - ref_seg).abs().max()) <= 2e-6 * scale, tag
    assert float((out - ref_out).abs().max()) <= 2e-6 * scale, tag
