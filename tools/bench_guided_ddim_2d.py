"""Guided airfoil design on the 2-D path (BASELINE config 5 under the ForceUnet objective, "standard-alpha"): the guided DDIM
chain of S steps (GaussianDiffusion(..., sampling_timesteps=S); cindm_ddpm2d_sample_ddim_force) against the 1000-step guided DDPM
chain of the same tree (cindm_ddpm2d_sample_force) -- same models, objective, seed, 64 designs x 2 boundaries.

    python tools/bench_guided_ddim_2d.py [B=64] [sampling_timesteps=250] [--boundaries 2] [--reps 2] [--ddpm-steps 1000] [--out FILE]

The two chains run in one process, alternating, ``--reps`` times each after one warm-up of both; every timing is a host clock
around a call that ends in a device synchronise (both entries synchronise before they return).  ``--ddpm-steps N`` stops the DDPM
chain after N of its 1000 steps (its time per step does not depend on t) and reports the 1000-step time as extrapolated.
Synthetic generator-defined weights.  The last line is JSON; ``--out`` also writes it to a file."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import cindm_amd                                   # noqa: E402
from cindm_amd.synthetic import synthetic_init_    # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("B", nargs="?", type=int, default=64)
ap.add_argument("steps", nargs="?", type=int, default=250, help="sampling_timesteps (DDIM steps)")
ap.add_argument("--boundaries", type=int, default=2)
ap.add_argument("--reps", type=int, default=2)
ap.add_argument("--ddpm-steps", type=int, default=1000)
ap.add_argument("--out", default=None)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_guided_ddim_2d: no ROCm device (there is no CPU timing)")
B, nb, S, N = args.B, args.boundaries, args.steps, args.ddpm_steps
dev = torch.device("cuda:0")
u = synthetic_init_(cindm_amd.Unet(dim=64, dim_mults=(1, 2), channels=21, image_size=64), 0).to(dev)
force = synthetic_init_(cindm_amd.ForceUnet(dim=64, dim_mults=(1, 2, 4, 8), channels=4), seed=7).to(dev)
fn = cindm_amd.ForceObjective(force, B, nb, 6, p_min=-37.7, p_max=57.6)
ddim = cindm_amd.GaussianDiffusion(u, image_size=64, frames=6, timesteps=1000, sampling_timesteps=S).to(dev)
ddpm = cindm_amd.GaussianDiffusion(u, image_size=64, frames=6, timesteps=1000, sampling_timesteps=1000).to(dev)
kw = dict(batch_size=B, num_boundaries=nb, design_fn=fn, design_guidance="standard-alpha", seed=1)
routes = {
    # name -> (callable, steps it runs, label)
    "ddim": (lambda: ddim.sample(**kw), S, f"guided DDIM, S = {S}: one library chain"),
    "ddpm": (lambda: ddpm.sample(t_stop=1000 - N, **kw), N, f"guided DDPM, {N} of 1000 steps: one library chain"),
}
times = {n: [] for n in routes}
for n in routes:                                   # warm-up: code objects, graph capture, workspaces
    assert bool(torch.isfinite(routes[n][0]()).all())
torch.cuda.synchronize()
for _ in range(args.reps):
    for n in routes:
        t0 = time.perf_counter()
        routes[n][0]()
        torch.cuda.synchronize()
        times[n].append(time.perf_counter() - t0)
res = {"B": B, "boundaries": nb, "sampling_timesteps": S, "ddpm_steps_run": N, "reps": args.reps, "recovered_chains": force.recovered,
       "device": torch.cuda.get_device_name(0)}
for n, (_, steps, label) in routes.items():
    med, lo, hi = statistics.median(times[n]), min(times[n]), max(times[n])
    chain = med if n == "ddim" else med * 1000 / N
    res[n] = {"ms_per_step": med / steps * 1e3, "s_per_chain": chain, "designs_per_s": B / chain, "spread": (hi - lo) / med,
              "extrapolated": n == "ddpm" and N != 1000, "runs_s": [round(t, 4) for t in times[n]]}
    print(f"{label}: B={B} nb={nb}: {med / steps * 1e3:.3f} ms/step, {chain:.2f} s/chain, {B / chain:.2f} designs/s "
          f"(median of {args.reps}, spread {100 * (hi - lo) / med:.1f} %)", flush=True)
res["ddim_over_ddpm_per_step"] = res["ddim"]["ms_per_step"] / res["ddpm"]["ms_per_step"]
res["designs_per_s_gain"] = res["ddim"]["designs_per_s"] / res["ddpm"]["designs_per_s"]
print(f"DDIM / DDPM time per step: {res['ddim_over_ddpm_per_step']:.4f}; designs/s gain: {res['designs_per_s_gain']:.2f}x")
line = json.dumps(res)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
print(line)
