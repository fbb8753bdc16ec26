"""Wall time of the autoregressive time composition (GaussianDiffusion1D.autoregress_time_compose_sample) in the shapes of
inference/inference_1d_composing_time_steps.py's autoregress path, synthetic generator-defined weights:
  default      B designs, Lc 4, R 20, F 8, n_composed 1 (2 segments), S DDIM steps, eta 0 (horizon-24 U-Net);
  single_step  B designs, horizon-8 U-Net, Lc = R = 4, prediction_steps 40 (10 segments x S steps);
  composed     the default rollout written as a Python loop of ddim_sample calls with the tail hand-over in torch -- run
               alternately with the one-call rollout in this process (best of REPS rounds each after one warm-up).
    python3 tools/bench_autoregress.py [--batch 1000] [--steps 1000] [--reps 3]"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import cindm_amd                                               # noqa: E402
from cindm_amd.diffusion1d import autoregress_segment_seeds   # noqa: E402
from cindm_amd.synthetic import synthetic_init_                # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1000)
    ap.add_argument("--steps", type=int, default=1000, help="DDIM steps S per segment (sampling_timesteps)")
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_autoregress.py needs a ROCm device")
    dev = torch.device("cuda:0")
    B, S = args.batch, args.steps

    def diffusion(hz, Lc, R):
        m = synthetic_init_(cindm_amd.TemporalUnet1D(hz, 8, False, attention=True), 0).to(dev)
        return cindm_amd.GaussianDiffusion1D(m, image_size=R, conditioned_steps=Lc, timesteps=1000, sampling_timesteps=S,
                                             loss_type="l1", ddim_sampling_eta=0.0).to(dev)

    d24, d8 = diffusion(24, 4, 20), diffusion(8, 4, 4)
    cond = (torch.rand((B, 4, 8), generator=torch.Generator().manual_seed(0)) - 0.5).to(dev)

    def composed():
        segs, c = [], cond
        for s in autoregress_segment_seeds(1, 2):
            img = d24.ddim_sample((B, 20, 8), c, seed=s)
            segs.append(img)
            c = img[:, -4:]
        return torch.cat(segs, dim=1)

    runs = {"default": (lambda: d24.autoregress_time_compose_sample(B, cond, 1, seed=1), 2),
            "single_step": (lambda: d8.autoregress_time_compose_sample(B, cond, 1, is_single_step_prediction=True, prediction_steps=40,
                                                                        seed=1), 10),
            "composed": (composed, 2)}
    outs = {}

    def timed(name):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = runs[name][0]()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        assert bool(torch.isfinite(out).all()), name
        outs[name] = out
        return dt

    for name in runs:
        timed(name)
    best = {name: float("inf") for name in runs}
    for _ in range(args.reps):
        for name in ("default", "composed"):          # alternate the two ways of running the same rollout
            best[name] = min(best[name], timed(name))
    for _ in range(args.reps):
        best["single_step"] = min(best["single_step"], timed("single_step"))
    same = bool(torch.equal(outs["default"], outs["composed"]))
    for name, (_, K) in runs.items():
        dt = best[name]
        rec = {"config": name, "batch": B, "segments": K, "ddim_steps": S, "s_per_rollout": round(dt, 4),
               "us_per_ddim_step": round(1e6 * dt / (K * S), 1), "designs_per_s": round(B / dt, 1)}
        if name == "composed":
            rec["one_call_vs_composed"] = round(best["default"] / dt, 4)
            rec["bitwise_equal_to_one_call"] = same
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
