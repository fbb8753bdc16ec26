"""The quadratic objective (cindm_ddpm1d_set_design_quadratic, compose_update_quad_kernel) on the guided DDPM library chain, against
the waypoint objective at the same shapes and against the Python loop the same objective takes as a generic callable (autograd between
library calls).

    python tools/bench_quadratic.py [B=256] [steps=50] [--recurrence 10] [--reps 5] [--only a,b,...] [--out profiles/quadratic_objective.json]

Shape: n_composed = 2, compose_start_step = 16 (L_tot = 56, three windows), F = 8, "standard-recurrence-N", the first ``steps``
reverse steps of the DDPM chain (t = 999 .. 1000 - steps; every step costs the same).  Routes, run alternating in one process, each
after one warm-up, ``--reps`` times; every timing is a host clock around a call that ends in a device synchronise:
    quadratic             QuadraticObjective, library chain (tables shared by every design)
    quadratic2            the same again: what two runs of one route differ by in this process
    quadratic_per_design  S and h per design, library chain
    waypoint              WaypointObjective at the same shapes, library chain
    generic               lambda x: obj(x) of the quadratic objective: the Python loop
The objective: both bodies arrive at a point and stop (positions and velocities of the last row), the bodies meet at row L // 2, the
centre of mass passes a point at row L // 3 -- all weights positive (S is positive semi-definite with eigenvalues below 1, so the
unclamped DDPM state stays of order 1 over the run; the JSON carries max |x| of every route's result).
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
ap.add_argument("--only", default="quadratic,quadratic2,quadratic_per_design,waypoint,generic")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "quadratic_objective.json"))
args = ap.parse_args()
sys.path.insert(0, ROOT)
import cindm_amd                                   # noqa: E402
from cindm_amd.synthetic import synthetic_init_    # noqa: E402

if not torch.cuda.is_available():
    sys.exit("bench_quadratic: no ROCm device (there is no CPU timing)")
B, S, R = args.B, args.steps, args.recurrence
HZ, NC, CS, NB = 24, 2, 16, 2
L, F = HZ + NC * CS, 4 * NB
dev = torch.device("cuda:0")
m = synthetic_init_(cindm_amd.TemporalUnet1D(HZ, F, False, attention=True), 0).to(dev)
d = cindm_amd.GaussianDiffusion1D(m, image_size=HZ, conditioned_steps=0, timesteps=1000, sampling_timesteps=1000).to(dev)


def residuals(target, meet, com):
    """(rows, A, r, weight) of the objective in the module docstring; target, meet, com: [..., 2]."""
    rows, A, r, w = [], [], [], []

    def add(row, coefs, value, weight):
        a = torch.zeros(F, dtype=torch.float64)
        for f, c in coefs:
            a[f] = c
        rows.append(row); A.append(a); r.append(value); w.append(weight)
    z = torch.zeros_like(target[..., 0])
    for j in range(NB):
        for c in range(2):
            add(L - 1, [(4 * j + c, 1.0)], target[..., c], 0.4)                       # arrive ...
            add(L - 1, [(4 * j + 2 + c, 1.0)], z, 0.4)                                # ... and stop
    for c in range(2):
        add(L // 2, [(c, 1.0), (4 + c, -1.0)], z + meet[..., c], 0.2)                 # the two bodies a given offset apart (0: they meet)
        add(L // 3, [(c, 0.5), (4 + c, 0.5)], com[..., c], 0.3)                       # the centre of mass
    r = torch.stack([v.double() for v in r], dim=-1)
    return torch.tensor(rows), torch.stack(A), r, torch.tensor(w, dtype=torch.float64)


g = torch.Generator().manual_seed(0)
tc = 0.5
quad = cindm_amd.QuadraticObjective.from_residuals(*residuals(torch.tensor([0.25, -0.5]), torch.zeros(2), torch.tensor([0.1, 0.2])),
                                                   L, F, time_consistency_coef=tc)
sweep = cindm_amd.QuadraticObjective.from_residuals(*residuals(torch.rand((B, 2), generator=g) * 1.2 - 0.6, torch.zeros((B, 2)),
                                                               torch.rand((B, 2), generator=g) * 0.6 - 0.3), L, F, time_consistency_coef=tc)
assert quad.per_design is None and sweep.per_design == B and sweep.S.dim() == 3 and sweep.h.dim() == 3
# (a sweep of targets moves h only: S per design as well, materialised, so that the route reads a matrix per design)
sweep = cindm_amd.QuadraticObjective(sweep.S.expand(B, -1, -1, -1).contiguous(), sweep.h, time_consistency_coef=tc)
way = cindm_amd.WaypointObjective.from_point([0.25, -0.5], 2, L, NB, coef=100, time_consistency_coef=tc, design_fn_mode="L2")
kw = dict(batch_size=B, n_composed=NC, compose_start_step=CS, compose_mode="mean-inside", design_guidance=f"standard-recurrence-{R}",
          seed=1, t_stop=1000 - S)
routes = {
    "quadratic": (lambda: d.sample(design_fn=quad, **kw), "QuadraticObjective, library chain"),
    "quadratic2": (lambda: d.sample(design_fn=quad, **kw), "QuadraticObjective, library chain (again)"),
    "quadratic_per_design": (lambda: d.sample(design_fn=sweep, **kw), "QuadraticObjective, S and h per design, library chain"),
    "waypoint": (lambda: d.sample(design_fn=way, **kw), "WaypointObjective, library chain"),
    "generic": (lambda: d.sample(design_fn=lambda x: quad(x), **kw), "generic callable of the quadratic objective: Python loop, autograd"),
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
    med, lo, hi = statistics.median(times[n]), min(times[n]), max(times[n])
    res[n] = {"ms_per_step": med / S * 1e3, "us_per_iteration": med / (S * R) * 1e6, "designs_per_s": B / med,
              "spread": (hi - lo) / med, "chain_s": [round(t, 4) for t in times[n]],
              "result_finite": bool(torch.isfinite(outs[n]).all()), "result_max_abs": float(outs[n].abs().max())}
    print(f"{routes[n][1]}: B={B} steps={S} R={R}: {med / S * 1e3:.3f} ms/step, {med / (S * R) * 1e6:.1f} us/iteration "
          f"(median of {args.reps}, spread {100 * (hi - lo) / med:.1f} %)", flush=True)
# (the Python loop draws with torch's generator where the library chain draws counter-based: other designs, the same work per iteration;
#  tests/test_gpu_quadratic.py compares the two routes on a tape)
if "waypoint" in res:
    for n in ("quadratic", "quadratic2", "quadratic_per_design"):
        if n in res:
            res[f"{n}_over_waypoint"] = res[n]["us_per_iteration"] / res["waypoint"]["us_per_iteration"]
            print(f"{n} / waypoint time per relaxation iteration: {res[f'{n}_over_waypoint']:.4f}")
if "generic" in res and "quadratic" in res:
    res["generic_over_quadratic"] = res["generic"]["us_per_iteration"] / res["quadratic"]["us_per_iteration"]
    print(f"generic / quadratic time per relaxation iteration: {res['generic_over_quadratic']:.3f}")
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
print(json.dumps(res))
