"""The sum of built-in objectives (cindm_amd.SumObjective, descriptor mode 7, compose_update_sum_kernel) on the guided DDPM library
chain, against the pair-distance objective alone at the same shapes -- the costliest built-in update before it -- and against the
Python loop the same sum takes as a generic callable (autograd between library calls).

    python tools/bench_sum_objective.py [B=256] [steps=50] [--recurrence 10] [--reps 5] [--only a,b,...] [--out profiles/sum_objective.json]

Shape: n_composed = 2, compose_start_step = 16 (L_tot = 56, three windows), F = 8, "standard-recurrence-N", the first ``steps``
reverse steps of the DDPM chain (t = 999 .. 1000 - steps; every step costs the same).  Routes, run alternating in one process, each
after one warm-up, ``--reps`` times; every timing is a host clock around a call that ends in a device synchronise:
    sum        quadratic + waypoint + pair-distance, library chain (the quadratic and the pair tables per design)
    pairdist   the sum's pair-distance term alone, library chain
    pairdist2  the same again: what two runs of the pair-distance route differ by in this process
    generic    lambda x: sum(x): the Python loop
The objective: reach the waypoints of the last two rows ("L2square"), arrive with zero velocity (a quadratic on the velocities of the
last row) and stay at least 0.3 apart on every row; weights small enough that the unclamped DDPM state stays of order 1 over the run
(the JSON carries max |x| of every route's result).
The claim the numbers are for: sum / pairdist per relaxation iteration is within 1 + 3 x the pair-distance route's own same-process
spread -- the larger of what ``pairdist`` and ``pairdist2`` differ by and the spread of their repeats -- and below generic / pairdist.
The last line is JSON, also written to ``--out``."""
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
ap.add_argument("--only", default="sum,pairdist,pairdist2,generic")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sum_objective.json"))
args = ap.parse_args()
sys.path.insert(0, ROOT)
import cindm_amd                                   # noqa: E402
from cindm_amd.synthetic import synthetic_init_    # noqa: E402

if not torch.cuda.is_available():
    sys.exit("bench_sum_objective: no ROCm device (there is no CPU timing)")
B, S, R = args.B, args.steps, args.recurrence
HZ, NC, CS, NB = 24, 2, 16, 2
L, F = HZ + NC * CS, 4 * NB
dev = torch.device("cuda:0")
m = synthetic_init_(cindm_amd.TemporalUnet1D(HZ, F, False, attention=True), 0).to(dev)
d = cindm_amd.GaussianDiffusion1D(m, image_size=HZ, conditioned_steps=0, timesteps=1000, sampling_timesteps=1000).to(dev)

g = torch.Generator().manual_seed(0)
tc = 0.5
# pair-distance, band and weight per design: at least (0.2 .. 0.4) apart on every row
lo = (torch.rand((B, 1, 1), generator=g) * 0.2 + 0.2).expand(B, L, 1).contiguous()
pair = cindm_amd.PairDistanceObjective(lo, torch.full((B, L, 1), float("inf")), torch.full((B, L, 1), 0.05), time_consistency_coef=tc)
# waypoint, shared: both bodies at their targets on the last two rows
target = torch.zeros((L, NB, 2))
target[:, 0], target[:, 1] = torch.tensor([0.25, -0.5]), torch.tensor([-0.25, 0.5])
weight = torch.zeros((L, NB))
weight[L - 2:] = 0.2
way = cindm_amd.WaypointObjective(target, weight, design_fn_mode="L2square")
# quadratic, S per design: zero velocity on the last row, with a weight swept over the designs
S_tab = torch.zeros((B, L, F, F))
for f in (2, 3, 6, 7):
    S_tab[:, L - 1, f, f] = torch.rand((B,), generator=g) * 0.2 + 0.1
quad = cindm_amd.QuadraticObjective(S_tab, torch.zeros((L, F)))
total = quad + way + pair
assert isinstance(total, cindm_amd.SumObjective) and total.per_design == B and total.time_consistency_coef == tc
kw = dict(batch_size=B, n_composed=NC, compose_start_step=CS, compose_mode="mean-inside", design_guidance=f"standard-recurrence-{R}",
          seed=1, t_stop=1000 - S)
routes = {
    "sum": (lambda: d.sample(design_fn=total, **kw), "SumObjective (quadratic + waypoint + pair-distance), library chain"),
    "pairdist": (lambda: d.sample(design_fn=pair, **kw), "PairDistanceObjective alone, library chain"),
    "pairdist2": (lambda: d.sample(design_fn=pair, **kw), "PairDistanceObjective alone, library chain (again)"),
    "generic": (lambda: d.sample(design_fn=lambda x: total(x), **kw), "generic callable of the sum: Python loop, autograd"),
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
#  tests/test_gpu_sum_objective.py compares the two routes on a tape)
if "pairdist" in res and "pairdist2" in res:
    a, b = res["pairdist"], res["pairdist2"]
    res["pairdist_same_process_spread"] = max(abs(a["us_per_iteration"] - b["us_per_iteration"]) / a["us_per_iteration"], a["spread"], b["spread"])
    print(f"pair-distance route, same-process spread: {100 * res['pairdist_same_process_spread']:.2f} %")
if "sum" in res and "pairdist" in res:
    res["sum_over_pairdist"] = res["sum"]["us_per_iteration"] / res["pairdist"]["us_per_iteration"]
    print(f"sum / pairdist time per relaxation iteration: {res['sum_over_pairdist']:.4f}")
    if "pairdist_same_process_spread" in res:
        res["sum_within_1_plus_3_spreads"] = bool(res["sum_over_pairdist"] <= 1.0 + 3.0 * res["pairdist_same_process_spread"])
if "generic" in res and "sum" in res:
    res["generic_over_sum"] = res["generic"]["us_per_iteration"] / res["sum"]["us_per_iteration"]
    res["sum_below_generic"] = bool(res["sum"]["us_per_iteration"] < res["generic"]["us_per_iteration"])
    print(f"generic / sum time per relaxation iteration: {res['generic_over_sum']:.3f}")
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
print(json.dumps(res))
