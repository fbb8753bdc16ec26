"""Wall time of the 2-D airfoil chain at 64 designs x 2 boundaries (BASELINE config 5's shape): the 1000-step DDPM chain against
DDIM chains of S = 250 and S = 100 steps (GaussianDiffusion(..., sampling_timesteps=S)), in one process, one warm-up chain each,
then REPS rounds that alternate the three chains; the best round of each is reported.  Synthetic generator-defined weights.
    python3 tools/bench_ddim2d.py [--reps 3] [--batch 64] [--boundaries 2]"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import cindm_amd                                   # noqa: E402
from cindm_amd.synthetic import synthetic_init_    # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--boundaries", type=int, default=2)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ddim2d.py needs a ROCm device")
    dev = torch.device("cuda:0")
    u = synthetic_init_(cindm_amd.Unet(dim=64, dim_mults=(1, 2), channels=21, image_size=64), 0).to(dev)
    chains = {S: cindm_amd.GaussianDiffusion(u, image_size=64, frames=6, timesteps=1000, sampling_timesteps=S).to(dev)
              for S in (1000, 250, 100)}

    def run(S):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = chains[S].sample(batch_size=args.batch, num_boundaries=args.boundaries, seed=1)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(out).all())
        return time.perf_counter() - t0

    for S in chains:
        run(S)
    best = {S: float("inf") for S in chains}
    for _ in range(args.reps):
        for S in chains:
            best[S] = min(best[S], run(S))
    ddpm = best[1000]
    for S, dt in best.items():
        print(json.dumps({"sampler": "ddpm" if S == 1000 else "ddim", "steps": S, "batch": args.batch, "boundaries": args.boundaries,
                          "s_per_chain": round(dt, 4), "ms_per_step": round(1e3 * dt / S, 4), "designs_per_s": round(args.batch / dt, 2),
                          "wall_vs_ddpm": round(dt / ddpm, 4)}))


if __name__ == "__main__":
    main()
