"""TEST INFRASTRUCTURE ONLY.  Golden vectors for the autoregressive time composition
(GaussianDiffusion1D.autoregress_time_compose_sample, model/diffusion_1d.py:2240-2327), captured from the reference on the
CPU with synthetic generator-defined weights (cindm_oracle.synth_state_dict); needs the reference tree (oracle/ref_import.py).
    python tests/manual/make_golden_autoregress.py        # a few seconds
Writes tests/golden/autoregress_1d.npz and tests/golden/PINNING_REPORT_AUTOREGRESS.json.

Per case <tag>: cond [B, Lc, F]; the noise tape in the reference's draw order -- composed [B, K R, F] (the output buffer's own
randn, :2253 / :2294, overwritten), init [K, B, R, F] (each segment's x_T, :2264 / :2299), step [K, S, B, R, F] (the randn_like of
every DDIM step, :2280 / :2315, drawn even when sigma == 0); seg [K, B, R, F] (each segment's final state) and out [B, K R, F]."""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import cindm_oracle as O          # noqa: E402
import ref_import                 # noqa: E402
from make_golden import build_ref_unet, patched_randn, relerr          # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")

# tag: (horizon, Lc, R, n_composed, single_step, prediction_steps, S, eta, B, seed)
CASES = {
    "a": (24, 4, 20, 2, False, 40, 8, 0.0, 2, 4101),
    "b": (24, 4, 20, 1, False, 40, 8, 0.5, 2, 4102),
    "c": (8, 4, 4, 0, True, 12, 8, 0.0, 2, 4103),
}


def n_segments(Lc, n_composed, single_step, prediction_steps):
    return -(-prediction_steps // Lc) if single_step else n_composed + 1


def oracle_rollout(od, cond, init, step, S, eta):
    """The rollout restated on cindm_oracle.ddim_sample: segment k = ddim_sample on (init[k], step[k]) conditioned on cond
    (k = 0) or on the last Lc rows of segment k-1.  Returns (seg [K, B, R, F], out [B, K R, F])."""
    segs, c = [], cond
    for k in range(init.shape[0]):
        img = O.ddim_sample(od, tuple(init[k].shape), c, {"init": init[k], "step": step[k]}, sampling_timesteps=S, eta=eta)
        segs.append(img)
        c = img[:, -od.conditioned_steps:]
    return torch.stack(segs), torch.cat(segs, dim=1)


def main():
    torch.set_num_threads(8)
    d1, _ = ref_import.import_reference()
    t0 = time.time()
    report, out = {}, {}
    for tag, (hz, Lc, R, n_composed, single, P, S, eta, B, seed) in CASES.items():
        m, sd, _ = build_ref_unet(d1, hz, 8)
        gd = d1.GaussianDiffusion1D(m, image_size=R, conditioned_steps=Lc, timesteps=1000, sampling_timesteps=S, loss_type="l1",
                                    ddim_sampling_eta=eta)
        K = n_segments(Lc, n_composed, single, P)
        g = torch.Generator().manual_seed(seed)
        cond = torch.rand((B, Lc, 8), generator=g) - 0.5
        composed = torch.randn((B, K * R, 8), generator=g)
        init = torch.randn((K, B, R, 8), generator=g)
        step = torch.randn((K, S, B, R, 8), generator=g)
        draws = [composed]
        for k in range(K):
            draws.append(init[k])
            draws.extend(step[k, i] for i in range(S))
        with patched_randn(draws) as tp:
            ref = gd.autoregress_time_compose_sample(batch_size=B, cond=cond, n_composed=n_composed, is_single_step_prediction=single,
                                                     prediction_steps=P)
            assert tp.i == len(draws), (tag, tp.i, len(draws))
        assert tuple(ref.shape) == (B, K * R, 8), (tag, tuple(ref.shape))
        seg = ref.reshape(B, K, R, 8).permute(1, 0, 2, 3).contiguous()
        od = O.Diffusion1D(sd, image_size=R, conditioned_steps=Lc)
        seg_o, out_o = oracle_rollout(od, cond, init, step, S, eta)
        report["autoregress." + tag] = max(relerr(out_o, ref), relerr(seg_o, seg))
        for name, v in (("cond", cond), ("composed", composed), ("init", init), ("step", step), ("seg", seg), ("out", ref)):
            out[f"{tag}.{name}"] = v.numpy().astype(np.float32)
        print("autoregress", tag, report["autoregress." + tag], round(time.time() - t0, 1), flush=True)
    np.savez_compressed(os.path.join(GOLD, "autoregress_1d.npz"), **out)
    report["seconds"] = time.time() - t0
    with open(os.path.join(GOLD, "PINNING_REPORT_AUTOREGRESS.json"), "w") as f:
        json.dump(report, f, indent=1)
    print(json.dumps(report, indent=1))
    bad = {k: v for k, v in report.items() if k != "seconds" and v > 2e-6}
    assert not bad, bad


if __name__ == "__main__":
    main()
