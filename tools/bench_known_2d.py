"""What the known region (``cond=``) adds to a step of the cfg5 chain: 64 designs x 2 boundaries, unguided DDPM.

    python tools/bench_known_2d.py [--steps 300] [--rounds 3] [--reps 2] [--out profiles/known_2d.json]
    python tools/bench_known_2d.py --one plain|known [--steps 300] [--reps 2]       (what the driver runs per process)

Two variants, ``plain`` (nothing armed) and ``known`` (``cond=``: the first 3 * cond_frames = 6 channels of every image held on
their forward-diffusion trajectory by known2d_kernel, one launch more per step).  The driver runs them in alternating fresh
processes on this tree's library, ``--rounds`` times; a process warms up once (code objects, workspace, graph capture) and times
``--reps`` chains of the first ``--steps`` reverse steps (t = 999 .. 1000 - steps; every step costs the same), a host clock around
a call that ends in a device synchronise.  Reported: the median microseconds per step of each variant over all its chains, their
ratio, the difference in microseconds, and what two runs of one variant differ by (max / min of the per-process medians).  The last
line is JSON; ``--out`` also writes it to a file."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--one", choices=["plain", "known"])
ap.add_argument("--steps", type=int, default=300)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--reps", type=int, default=2)
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--out")
args = ap.parse_args()

if args.one is None:
    variants = ("plain", "known")
    runs = {v: [] for v in variants}
    for _ in range(args.rounds):
        for v in variants:                       # one fresh process per run, the two variants alternating
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", v, "--steps", str(args.steps), "--reps", str(args.reps),
                                  "--batch", str(args.batch)], check=True, capture_output=True, text=True, timeout=900).stdout
            runs[v].append(json.loads(out.strip().splitlines()[-1]))
            print(f"{v}: {runs[v][-1]['us_per_step']:.1f} us/step", flush=True)
    res = {"workload": f"cfg5 shape: {args.batch} designs x 2 boundaries, unguided DDPM, first {args.steps} steps", "steps": args.steps,
           "rounds": args.rounds, "reps": args.reps, "device": runs["plain"][0]["device"]}
    for v in variants:
        chains = [t for r in runs[v] for t in r["chain_s"]]
        meds = [r["us_per_step"] for r in runs[v]]
        res[v] = {"us_per_step": statistics.median(chains) / args.steps * 1e6, "per_process_us_per_step": [round(m, 2) for m in meds],
                  "run_to_run": max(meds) / min(meds)}
    res["known_over_plain"] = res["known"]["us_per_step"] / res["plain"]["us_per_step"]
    res["known_minus_plain_us_per_step"] = res["known"]["us_per_step"] - res["plain"]["us_per_step"]
    res["known_bytes_per_step"] = runs["known"][0]["known_bytes_per_step"]
    res["region_held_exactly"] = all(r["region_held"] for r in runs["known"])
    print(f"known / plain: {res['known_over_plain']:.4f} ({res['known_minus_plain_us_per_step']:+.1f} us per step; run to run: plain "
          f"{res['plain']['run_to_run']:.4f}, known {res['known']['run_to_run']:.4f})")
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))
    sys.exit(0)

import torch                                       # noqa: E402

sys.path.insert(0, HERE)
import cindm_amd                                   # noqa: E402
from cindm_amd.synthetic import synthetic_init_    # noqa: E402

if not torch.cuda.is_available():
    sys.exit("bench_known_2d: no ROCm device (there is no CPU timing)")
dev = torch.device("cuda:0")
B, NB, S = args.batch, 2, args.steps
model = synthetic_init_(cindm_amd.Unet(dim=64, dim_mults=(1, 2), channels=21, image_size=64), seed=0).to(dev)
d = cindm_amd.GaussianDiffusion(model, image_size=64, frames=6, cond_frames=2, timesteps=1000, sampling_timesteps=1000).to(dev)
kw = dict(batch_size=B, num_boundaries=NB, seed=1, t_stop=1000 - S)
cond = None
if args.one == "known":
    cond = (torch.rand((B, 6, 64, 64), generator=torch.Generator().manual_seed(0)) * 2 - 1).to(dev)
    kw["cond"] = cond
d.sample(**dict(kw, t_stop=990))                   # warm-up
torch.cuda.synchronize()
chains = []
for _ in range(args.reps):
    t0 = time.perf_counter()
    out = d.sample(**kw)
    torch.cuda.synchronize()
    chains.append(time.perf_counter() - t0)
held = True
if cond is not None:
    # (a truncated chain ends at level t_stop - 1: the exact return is checked on the last two steps of a 2-step diffusion instead)
    d2 = cindm_amd.GaussianDiffusion(model, image_size=64, frames=6, cond_frames=2, timesteps=2, sampling_timesteps=2).to(dev)
    o2 = d2.sample(batch_size=B, num_boundaries=NB, seed=1, cond=cond)
    held = bool(torch.equal(o2[:, 0, :6], cond) and torch.equal(o2[:, 1, :6], cond))
# what the node moves per step with cond=, per image and pixel: 6 mask bytes; channel group 0 (known whole) 16 bytes of values
# read and 16 of state written; group 1 (half known) the state read as well
res = {"variant": args.one, "us_per_step": statistics.median(chains) / S * 1e6, "chain_s": [round(t, 4) for t in chains],
       "known_bytes_per_step": B * NB * 64 * 64 * (6 + 32 + 48) if cond is not None else 0, "region_held": held,
       "device": torch.cuda.get_device_name(0)}
print(json.dumps(res))
