"""The waypoint objective (table form, cindm_ddpm1d_set_design_tables) against the point objective on the guided DDPM library chain,
and the library chain against the Python loop a generic callable takes (autograd between library calls).

    python tools/bench_waypoint.py [B=256] [steps=50] [--recurrence 10] [--reps 5] [--only a,b,...]

Shape: n_composed = 2, compose_start_step = 10 (L_tot = 44, three windows), "standard-recurrence-N", the first ``steps``
reverse steps of the DDPM chain (t = 999 .. 1000 - steps; every step costs the same).  Routes, run alternating in one process, each
after one warm-up, ``--reps`` times; every timing is a host clock around a call that ends in a device synchronise:
    point             PointObjective, library chain
    point2            the same again: what two runs of one route differ by in this process
    table             WaypointObjective.from_point of it, library chain (tables shared by every design)
    table_per_design  a target and a weight per design (a sweep in one batch), library chain
    generic           lambda x: obj(x) of the table objective: the Python loop
The last line is JSON."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ap = argparse.ArgumentParser()
ap.add_argument("B", nargs="?", type=int, default=256)
ap.add_argument("steps", nargs="?", type=int, default=50, help="reverse steps per chain")
ap.add_argument("--recurrence", type=int, default=10)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--only", default="point,point2,table,table_per_design,generic")
args = ap.parse_args()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cindm_amd                                   # noqa: E402
from cindm_amd.synthetic import synthetic_init_    # noqa: E402

if not torch.cuda.is_available():
    sys.exit("bench_waypoint: no ROCm device (there is no CPU timing)")
B, S, R = args.B, args.steps, args.recurrence
HZ, NC, CS, NB = 24, 2, 10, 2
L = HZ + NC * CS
dev = torch.device("cuda:0")
m = synthetic_init_(cindm_amd.TemporalUnet1D(HZ, 8, False, attention=True), 0).to(dev)
d = cindm_amd.GaussianDiffusion1D(m, image_size=HZ, conditioned_steps=0, timesteps=1000, sampling_timesteps=1000).to(dev)
okw = dict(coef=100, time_consistency_coef=0.5, design_fn_mode="L2")
point = cindm_amd.PointObjective([0.25, -0.5], 2, **okw)
table = cindm_amd.WaypointObjective.from_point([0.25, -0.5], 2, L, NB, **okw)
g = torch.Generator().manual_seed(0)
sweep = cindm_amd.WaypointObjective(torch.rand((B, L, NB, 2), generator=g) * 1.2 - 0.6,
                                    torch.rand((B, L, NB), generator=g) * (torch.rand((B, L, NB), generator=g) > 0.8), **okw)
kw = dict(batch_size=B, n_composed=NC, compose_start_step=CS, compose_mode="mean-inside", design_guidance=f"standard-recurrence-{R}",
          seed=1, t_stop=1000 - S)
routes = {
    "point": (lambda: d.sample(design_fn=point, **kw), "PointObjective, library chain"),
    "point2": (lambda: d.sample(design_fn=point, **kw), "PointObjective, library chain (again)"),
    "table": (lambda: d.sample(design_fn=table, **kw), "WaypointObjective.from_point, library chain"),
    "table_per_design": (lambda: d.sample(design_fn=sweep, **kw), "WaypointObjective, target and weight per design, library chain"),
    "generic": (lambda: d.sample(design_fn=lambda x: table(x), **kw), "generic callable of the table objective: Python loop, autograd"),
}
names = [n for n in args.only.split(",") if n]
times = {n: [] for n in names}
outs = {}
for n in names:                                    # warm-up: code objects, graph capture, workspace, device tables
    outs[n] = routes[n][0]().clone()
torch.cuda.synchronize()
for _ in range(args.reps):
    for n in names:
        t0 = time.perf_counter()
        routes[n][0]()
        torch.cuda.synchronize()
        times[n].append(time.perf_counter() - t0)
res = {"B": B, "steps": S, "recurrence": R, "L_tot": L, "n_composed": NC, "compose_start_step": CS, "reps": args.reps,
       "device": torch.cuda.get_device_name(0), "recovered_chains": int(m.recovered)}
for n in names:
    med, lo, hi = statistics.median(times[n]), min(times[n]), max(times[n])
    res[n] = {"ms_per_step": med / S * 1e3, "us_per_iteration": med / (S * R) * 1e6, "designs_per_s": B / med,
              "spread": (hi - lo) / med, "chain_s": [round(t, 4) for t in times[n]]}
    print(f"{routes[n][1]}: B={B} steps={S} R={R}: {med / S * 1e3:.3f} ms/step, {med / (S * R) * 1e6:.1f} us/iteration "
          f"(median of {args.reps}, spread {100 * (hi - lo) / med:.1f} %)", flush=True)
if "point" in outs and "table" in outs:
    res["table_equals_point_bitwise"] = bool(torch.equal(outs["point"], outs["table"]))
if "point" in res:
    for n in ("point2", "table", "table_per_design"):
        if n in res:
            res[f"{n}_over_point"] = res[n]["us_per_iteration"] / res["point"]["us_per_iteration"]
            print(f"{n} / point time per relaxation iteration: {res[f'{n}_over_point']:.4f}")
if "generic" in res and "table" in res:
    res["generic_over_table"] = res["generic"]["us_per_iteration"] / res["table"]["us_per_iteration"]
    print(f"generic / table time per relaxation iteration: {res['generic_over_table']:.3f}")
print(json.dumps(res))
