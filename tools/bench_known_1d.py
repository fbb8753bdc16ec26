"""What a known region (``known=`` / ``known_mask=``) adds to a step of the cfg2 chain: 256 designs, plain DDPM.

    python tools/bench_known_1d.py [--rounds 3] [--reps 2] [--out profiles/known_1d.json]
    python tools/bench_known_1d.py --one plain|known|bodies [--reps 2]       (what the driver runs per process)

Three variants: ``plain`` (nothing armed), ``known`` (the first and the last two rows of every design held on their forward-diffusion
trajectory by known1d_kernel: a sparse region, shared by all designs) and ``bodies`` (one of the two bodies on every row: half the
state).  A region costs one launch more per step.  The driver runs the variants in alternating fresh processes on this tree's
library, ``--rounds`` times; a process warms up with one whole chain (code objects, workspace, graph capture) and times ``--reps``
whole chains of 1000 reverse steps, a host clock around a call that ends in a device synchronise.  Reported: the median
microseconds per step of each variant over all its chains, the ratios to ``plain``, the differences in microseconds, and what two
runs of one variant differ by (max / min of the per-process medians).  The last line is JSON; ``--out`` also writes it to a file."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIANTS = ("plain", "known", "bodies")
ap = argparse.ArgumentParser()
ap.add_argument("--one", choices=VARIANTS)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--reps", type=int, default=2)
ap.add_argument("--batch", type=int, default=256)
ap.add_argument("--out")
args = ap.parse_args()
STEPS = 1000

if args.one is None:
    runs = {v: [] for v in VARIANTS}
    for _ in range(args.rounds):
        for v in VARIANTS:                       # one fresh process per run, the variants alternating
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", v, "--reps", str(args.reps), "--batch", str(args.batch)],
                                 check=True, capture_output=True, text=True, timeout=600).stdout
            runs[v].append(json.loads(out.strip().splitlines()[-1]))
            print(f"{v}: {runs[v][-1]['us_per_step']:.1f} us/step", flush=True)
    res = {"workload": f"cfg2 shape: {args.batch} designs of 24 rows x 2 bodies, plain DDPM, {STEPS} steps per chain", "steps": STEPS,
           "rounds": args.rounds, "reps": args.reps, "device": runs["plain"][0]["device"]}
    for v in VARIANTS:
        chains = [t for r in runs[v] for t in r["chain_s"]]
        meds = [r["us_per_step"] for r in runs[v]]
        res[v] = {"us_per_step": statistics.median(chains) / STEPS * 1e6, "per_process_us_per_step": [round(m, 2) for m in meds],
                  "run_to_run": max(meds) / min(meds), "launches_per_step": runs[v][0]["launches_per_step"],
                  "update_fused": runs[v][0]["update_fused"], "known_fraction": runs[v][0]["known_fraction"]}
    for v in VARIANTS[1:]:
        res[f"{v}_over_plain"] = res[v]["us_per_step"] / res["plain"]["us_per_step"]
        res[f"{v}_minus_plain_us_per_step"] = res[v]["us_per_step"] - res["plain"]["us_per_step"]
    res["region_held_exactly"] = all(r["region_held"] for v in VARIANTS[1:] for r in runs[v])
    print(f"known / plain: {res['known_over_plain']:.4f} ({res['known_minus_plain_us_per_step']:+.1f} us per step), bodies / plain: "
          f"{res['bodies_over_plain']:.4f} ({res['bodies_minus_plain_us_per_step']:+.1f} us per step); run to run: "
          + ", ".join(f"{v} {res[v]['run_to_run']:.4f}" for v in VARIANTS))
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
    sys.exit("bench_known_1d: no ROCm device (there is no CPU timing)")
dev = torch.device("cuda:0")
B, L, F = args.batch, 24, 8
pair = synthetic_init_(cindm_amd.TemporalUnet1D(horizon=L, transition_dim=F, cond_dim=False, dim=64, dim_mults=(1, 2, 4, 8), attention=True),
                       seed=0).to(dev)
d = cindm_amd.GaussianDiffusion1D(pair, image_size=L, conditioned_steps=0, timesteps=STEPS, sampling_timesteps=STEPS, loss_type="l1").to(dev)
kw = dict(batch_size=B, cond=None, n_composed=0, compose_n_bodies=2)
mask = None
if args.one != "plain":
    known = (torch.rand((L, F), generator=torch.Generator().manual_seed(0)) * 2 - 1).to(dev)
    mask = torch.zeros((L, F), dtype=torch.bool, device=dev)
    if args.one == "known":
        mask[0] = mask[-2:] = True
    else:
        mask[:, :4] = True
    kw.update(known=known, known_mask=mask)
d.sample(seed=1, **kw)                             # warm-up: one whole chain
torch.cuda.synchronize()
chains = []
for i in range(args.reps):
    t0 = time.perf_counter()
    out = d.sample(seed=2 + i, **kw)
    torch.cuda.synchronize()
    chains.append(time.perf_counter() - t0)
launches, fused = d.last_step_info()
held = mask is None or bool(torch.equal(out[:, mask], known[mask].expand(B, -1)))
res = {"variant": args.one, "us_per_step": statistics.median(chains) / STEPS * 1e6, "chain_s": [round(t, 4) for t in chains],
       "launches_per_step": launches, "update_fused": fused, "known_fraction": 0.0 if mask is None else float(mask.float().mean()),
       "region_held": held, "device": torch.cuda.get_device_name(0)}
print(json.dumps(res))
