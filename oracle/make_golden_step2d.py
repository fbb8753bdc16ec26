"""TEST INFRASTRUCTURE ONLY.  Golden vectors of the 2-D reverse step alone -- from the model's output to (model_mean, x_start,
pred_noise) and the next state -- over every option combination the 2-D update kernel serves; runs ONLY in the build container
(imports the reference through oracle/ref_import.py, like oracle/make_golden_2d.py).

The reference's own ``GaussianDiffusion`` (model/diffusion_2d.py) runs on ``step2d_cases.toy_model`` in place of its U-Net, at the
records of ``step2d_cases.golden_records()``:

  * p_mean_variance (:757-773) and p_sample (:788-808) under objective x share_noise x use_average_share x clip_denoised x
    t in {0, 1, 500, 999}: ``step.mean``, ``step.x_start`` (p_mean_variance's; p_sample's is asserted to be the same bits) and
    ``step.state`` (p_sample with the draws of ``step2d_cases.make_noise``)
  * model_predictions (:727-754) under objective x share_noise x use_average_share x clip_x_start x rederive_pred_noise x t:
    ``predict.pred_noise``, ``predict.x_start``

each at the five (B, nb) of the grid, on 1 x 1 images (why: step2d_cases.GOLDEN_SIZE).  Inputs are not stored: the states and
draws are seeded (``make_state``, ``make_noise``) and the toy model gives the same bits on every machine.  The five arrays are the
records' tensors flattened and laid end to end in record order.  Every record asserts oracle == reference (the pin).  The archive is
written with fixed member dates: a second run gives the same bytes.

    python oracle/make_golden_step2d.py          # seconds
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tests"))
import cindm_oracle as O                                    # noqa: E402
import ref_import                                           # noqa: E402
import step2d_cases as S                                    # noqa: E402
from make_golden import GOLD, patched_randn, relerr         # noqa: E402
from make_golden_compose import save_npz                    # noqa: E402


class ToyUnet(torch.nn.Module):
    """What the reference's GaussianDiffusion asks of its model, around the pixel-wise toy."""
    channels = out_dim = S.CHANNELS
    self_condition = False
    random_or_learned_sinusoidal_cond = False

    def forward(self, x, t, x_self_cond=None):
        return S.toy_model(x, t)


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    _, d2 = ref_import.import_reference()
    C, H = S.CHANNELS, S.GOLDEN_SIZE
    frames = (C - 3) // 3
    parts = {k: [] for k in ("step.mean", "step.x_start", "step.state", "predict.pred_noise", "predict.x_start")}
    worst = 0.0
    diffs = {}
    for name, entry, obj, share, avg, clip, red, t, B, nb in S.golden_records():
        key = (obj, share, avg)
        if key not in diffs:
            gd = d2.GaussianDiffusion(ToyUnet(), image_size=H, frames=frames, cond_frames=2, timesteps=1000, sampling_timesteps=1000,
                                      loss_type="l2", objective=obj, beta_schedule=S.BETA_SCHEDULE, share_noise=share, use_average_share=avg)
            od = O.Diffusion2D({"final_conv.weight": torch.zeros(C, 1)}, image_size=H, frames=frames, beta_schedule=S.BETA_SCHEDULE,
                               objective=obj, share_noise=share, use_average_share=avg)
            od.model = S.toy_model
            for k in O.SCHEDULE_BUFFERS:
                assert torch.equal(getattr(gd, k), od.tab[k]), k
            diffs[key] = (gd, od)
        gd, od = diffs[key]
        shape = (B, nb, C, H, H)
        x = S.make_state(C, B, nb, t, False, H)
        tt = torch.full((B * nb,), t, dtype=torch.long)
        with torch.no_grad():
            if entry == "model_predictions":
                pr = gd.model_predictions(shape, x.clone(), tt, None, clip_x_start=clip, rederive_pred_noise=red, share_noise=share)
                o_eps, o_x0 = O.model_predictions_2d(od, shape, x.clone(), t, clip_x_start=clip, rederive_pred_noise=red, share_noise=share)
                worst = max(worst, relerr(o_eps, pr.pred_noise), relerr(o_x0, pr.pred_x_start))
                parts["predict.pred_noise"].append(pr.pred_noise.numpy().ravel())
                parts["predict.x_start"].append(pr.pred_x_start.numpy().ravel())
                continue
            mean, _, _, x0 = gd.p_mean_variance(shape, x.clone(), tt, None, clip_denoised=clip)
            zs, zb = S.make_noise(C, B, nb, t, H)
            draws = [zs, zb] if t > 0 else []
            with patched_randn(draws) as tp:
                state, x0s = gd.p_sample(shape, x.clone(), t, None, clip_denoised=clip)
                assert tp.i == len(draws)
            assert torch.equal(x0s, x0), name
            if t == 0:
                assert torch.equal(state, mean), name
            nz = None if t == 0 else O.sample_noise_2d(zs, zb).reshape(B * nb, C, H, H)
            o_state, o_x0 = O.p_sample_2d(od, shape, x.clone(), t, nz, clip_denoised=clip)
            worst = max(worst, relerr(o_state, state), relerr(o_x0, x0))
            for k, v in (("step.mean", mean), ("step.x_start", x0), ("step.state", state)):
                parts[k].append(v.numpy().ravel())
    out = {k: np.concatenate(v).astype(np.float32) for k, v in parts.items()}
    path = os.path.join(GOLD, "step2d_grid.npz")
    save_npz(path, out)
    print("records", len(S.golden_records()), "oracle vs reference", worst, "bytes", os.path.getsize(path), flush=True)
    assert worst <= 2e-6, worst
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()
