"""Guided DDIM (sampling_timesteps < timesteps, point objective, "-recurrence-N" guidance): the built-in objective's library
chain (cindm_ddpm1d_sample_ddim_guided) against the generic-callable route (autograd between library calls) and, per relaxation
iteration, against the guided DDPM chain (cindm_ddpm1d_sample_guided) -- same model, objective and guidance as
tools/bench_guided.py, n_composed = 0.

    python tools/bench_guided_ddim.py [B=256] [sampling_timesteps=250] [--recurrence 10] [--reps 3] [--only a,b] [--root TREE]

The routes run in one process, alternating, ``--reps`` times each after one warm-up of every shape; every timing is a host clock
around a call that ends in a device synchronise.  ``--root`` imports the package from another tree (a checkout of an older commit:
there ``design_fn=PointObjective`` is the Python loop, which is the baseline the built-in route replaces).  The last line is JSON."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ap = argparse.ArgumentParser()
ap.add_argument("B", nargs="?", type=int, default=256)
ap.add_argument("steps", nargs="?", type=int, default=250, help="sampling_timesteps (DDIM steps)")
ap.add_argument("--recurrence", type=int, default=10)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--only", default="builtin,generic,ddpm")
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.root))
import cindm_amd                                   # noqa: E402
from cindm_amd import _ffi                         # noqa: E402
from cindm_amd.synthetic import synthetic_init_    # noqa: E402

if not torch.cuda.is_available():
    sys.exit("bench_guided_ddim: no ROCm device (there is no CPU timing)")
B, S, R = args.B, args.steps, args.recurrence
dev = torch.device("cuda:0")
m = synthetic_init_(cindm_amd.TemporalUnet1D(24, 8, False, attention=True), 0).to(dev)
ddim = cindm_amd.GaussianDiffusion1D(m, image_size=24, conditioned_steps=0, timesteps=1000, sampling_timesteps=S).to(dev)
ddpm = cindm_amd.GaussianDiffusion1D(m, image_size=24, conditioned_steps=0, timesteps=1000, sampling_timesteps=1000).to(dev)
obj = cindm_amd.PointObjective([0.25, -0.5], 1, coef=100, design_fn_mode="L2")
kw = dict(batch_size=B, n_composed=0, compose_mode="mean-inside", design_guidance=f"standard-recurrence-{R}", seed=1)
has_entry = "cindm_ddpm1d_sample_ddim_guided" in _ffi.SIGNATURES
routes = {
    # name -> (callable running S steps of R iterations, label)
    "builtin": (lambda: ddim.sample(design_fn=obj, **kw),
                "DDIM, PointObjective: " + ("one library chain" if has_entry else "Python loop (this tree has no built-in DDIM route)")),
    "generic": (lambda: ddim.sample(design_fn=lambda x: obj(x), **kw), "DDIM, generic callable: autograd between library calls"),
    "ddpm": (lambda: ddpm.sample(design_fn=obj, t_stop=1000 - S, **kw), "DDPM, PointObjective: guided library chain, the same number of steps"),
}
names = [n for n in args.only.split(",") if n]
times = {n: [] for n in names}
for n in names:                                    # warm-up: code objects, graph capture, workspace
    routes[n][0]()
torch.cuda.synchronize()
for _ in range(args.reps):
    for n in names:
        t0 = time.perf_counter()
        routes[n][0]()
        torch.cuda.synchronize()
        times[n].append(time.perf_counter() - t0)
res = {"B": B, "sampling_timesteps": S, "recurrence": R, "reps": args.reps, "root": os.path.abspath(args.root), "builtin_is_library_chain": has_entry}
for n in names:
    med, lo, hi = statistics.median(times[n]), min(times[n]), max(times[n])
    res[n] = {"ms_per_step": med / S * 1e3, "us_per_iteration": med / (S * R) * 1e6, "designs_per_s": B / med,
              "spread": (hi - lo) / med, "chain_s": [round(t, 4) for t in times[n]]}
    print(f"{routes[n][1]}: B={B} S={S} R={R}: {med / S * 1e3:.3f} ms/step, {med / (S * R) * 1e6:.1f} us/iteration, "
          f"{B / med:.2f} designs/s (median of {args.reps}, spread {100 * (hi - lo) / med:.1f} %)", flush=True)
if "builtin" in res and "generic" in res:
    res["generic_over_builtin"] = res["generic"]["ms_per_step"] / res["builtin"]["ms_per_step"]
    print(f"generic / built-in time per step: {res['generic_over_builtin']:.3f}")
if "builtin" in res and "ddpm" in res:
    res["ddim_over_ddpm_per_iteration"] = res["builtin"]["us_per_iteration"] / res["ddpm"]["us_per_iteration"]
    print(f"DDIM / DDPM time per relaxation iteration: {res['ddim_over_ddpm_per_iteration']:.4f}")
print(json.dumps(res))
