"""The pair-distance objective (cindm_ddpm1d_set_design_pairdist, compose_update_pair_kernel) on the guided DDPM library chain, against
the waypoint objective at the same shapes and against the Python loop the same objective takes as a generic callable (autograd between
library calls).

    python tools/bench_pairdist.py [B=256] [steps=50] [--recurrence 10] [--reps 5] [--only a,b,...] [--out profiles/pair_distance_objective.json]

Shape: n_composed = 2, compose_start_step = 16 (L_tot = 56, three windows), F = 8, "standard-recurrence-N", the first ``steps``
reverse steps of the DDPM chain (t = 999 .. 1000 - steps; every step costs the same).  Routes, run alternating in one process, each
after one warm-up, ``--reps`` times; every timing is a host clock around a call that ends in a device synchronise:
    pairdist              PairDistanceObjective, library chain (tables shared by every design)
    pairdist_per_design   band and weight per design, library chain
    waypoint              WaypointObjective at the same shapes, library chain
    waypoint2             the same again: what two runs of the waypoint route differ by in this process
    generic               lambda x: obj(x) of the pair-distance objective: the Python loop
The objective: the two bodies stay at least 0.3 apart on every row, come within 1.0 at row L // 2 and meet at distance 0.5 on the
last row (weights 0.05 .. 0.2: "standard" guidance takes the raw gradient and the unclamped DDPM state has to stay of order 1 over the
run; the JSON carries max |x| of every route's result).  The per-design route sweeps the three distances over the designs.
The claim the numbers are for: the pair-distance route is within the waypoint route's own same-process spread -- the larger of what
``waypoint`` and ``waypoint2`` differ by and the spread of their repeats.  The last line is JSON, also written to ``--out``."""
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
ap.add_argument("--only", default="pairdist,pairdist_per_design,waypoint,waypoint2,generic")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pair_distance_objective.json"))
args = ap.parse_args()
sys.path.insert(0, ROOT)
import cindm_amd                                   # noqa: E402
from cindm_amd.synthetic import synthetic_init_    # noqa: E402

if not torch.cuda.is_available():
    sys.exit("bench_pairdist: no ROCm device (there is no CPU timing)")
B, S, R = args.B, args.steps, args.recurrence
HZ, NC, CS, NB = 24, 2, 16, 2
L, F = HZ + NC * CS, 4 * NB
dev = torch.device("cuda:0")
m = synthetic_init_(cindm_amd.TemporalUnet1D(HZ, F, False, attention=True), 0).to(dev)
d = cindm_amd.GaussianDiffusion1D(m, image_size=HZ, conditioned_steps=0, timesteps=1000, sampling_timesteps=1000).to(dev)


def tables(apart, within, at):
    """(lo, hi, weight) [.., L, 1] of the objective in the module docstring; apart, within, at: [...] distances."""
    lead = tuple(apart.shape)
    lo = apart[..., None, None].expand(lead + (L, 1)).clone()
    hi = torch.full(lead + (L, 1), float("inf"))
    w = torch.full((L, 1), 0.05)
    hi[..., L // 2, 0] = within
    lo[..., L - 1, 0], hi[..., L - 1, 0] = at, at
    w[L // 2, 0], w[L - 1, 0] = 0.1, 0.2
    return lo, hi, w


g = torch.Generator().manual_seed(0)
tc = 0.5
pair = cindm_amd.PairDistanceObjective(*tables(torch.tensor(0.3), torch.tensor(1.0), torch.tensor(0.5)), time_consistency_coef=tc)
lo, hi, w = tables(torch.rand((B,), generator=g) * 0.2 + 0.2, torch.rand((B,), generator=g) * 0.4 + 0.8, torch.rand((B,), generator=g) * 0.2 + 0.4)
sweep = cindm_amd.PairDistanceObjective(lo, hi, w.expand(B, -1, -1).contiguous(), time_consistency_coef=tc)
assert pair.per_design is None and sweep.per_design == B and sweep.tables("cpu")[0].dim() == 4 and sweep.tables("cpu")[1].dim() == 3
way = cindm_amd.WaypointObjective.from_point([0.25, -0.5], 2, L, NB, coef=100, time_consistency_coef=tc, design_fn_mode="L2")
kw = dict(batch_size=B, n_composed=NC, compose_start_step=CS, compose_mode="mean-inside", design_guidance=f"standard-recurrence-{R}",
          seed=1, t_stop=1000 - S)
routes = {
    "pairdist": (lambda: d.sample(design_fn=pair, **kw), "PairDistanceObjective, library chain"),
    "pairdist_per_design": (lambda: d.sample(design_fn=sweep, **kw), "PairDistanceObjective, band and weight per design, library chain"),
    "waypoint": (lambda: d.sample(design_fn=way, **kw), "WaypointObjective, library chain"),
    "waypoint2": (lambda: d.sample(design_fn=way, **kw), "WaypointObjective, library chain (again)"),
    "generic": (lambda: d.sample(design_fn=lambda x: pair(x), **kw), "generic callable of the pair-distance objective: Python loop, autograd"),
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
res = {"B": B, "steps": S, "recurrence": R, "L_tot": L, "F": F, "n_composed": NC, "compose_start_step": CS, "reps": args.reps,
       "device": torch.cuda.get_device_name(0), "recovered_chains": int(m.recovered)}
for n in names:
    med, lo_, hi_ = statistics.median(times[n]), min(times[n]), max(times[n])
    res[n] = {"ms_per_step": med / S * 1e3, "us_per_iteration": med / (S * R) * 1e6, "designs_per_s": B / med,
              "spread": (hi_ - lo_) / med, "chain_s": [round(t, 4) for t in times[n]],
              "result_finite": bool(torch.isfinite(outs[n]).all()), "result_max_abs": float(outs[n].abs().max())}
    print(f"{routes[n][1]}: B={B} steps={S} R={R}: {med / S * 1e3:.3f} ms/step, {med / (S * R) * 1e6:.1f} us/iteration "
          f"(median of {args.reps}, spread {100 * (hi_ - lo_) / med:.1f} %)", flush=True)
# (the Python loop draws with torch's generator where the library chain draws counter-based: other designs, the same work per iteration;
#  tests/test_gpu_pairdist.py compares the two routes on a tape)
if "waypoint" in res:
    if "waypoint2" in res:
        a, b = res["waypoint"], res["waypoint2"]
        res["waypoint_same_process_spread"] = max(abs(a["us_per_iteration"] - b["us_per_iteration"]) / a["us_per_iteration"], a["spread"], b["spread"])
        print(f"waypoint route, same-process spread: {100 * res['waypoint_same_process_spread']:.2f} %")
    for n in ("pairdist", "pairdist_per_design"):
        if n in res:
            res[f"{n}_over_waypoint"] = res[n]["us_per_iteration"] / res["waypoint"]["us_per_iteration"]
            print(f"{n} / waypoint time per relaxation iteration: {res[f'{n}_over_waypoint']:.4f}")
            if "waypoint_same_process_spread" in res:
                res[f"{n}_within_waypoint_spread"] = bool(res[f"{n}_over_waypoint"] - 1.0 <= res["waypoint_same_process_spread"])
if "generic" in res and "pairdist" in res:
    res["generic_over_pairdist"] = res["generic"]["us_per_iteration"] / res["pairdist"]["us_per_iteration"]
    print(f"generic / pairdist time per relaxation iteration: {res['generic_over_pairdist']:.3f}")
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
print(json.dumps(res))
