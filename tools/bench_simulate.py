"""cindm_amd.simulation (cindm_nbody_simulate, nbody_simulate_kernel) at the size the reference's 1-D script re-simulates:
1000 designs x {2, 4, 8} bodies x 92 frames.

    python tools/bench_simulate.py [B=1000] [n_steps=92] [--bodies 2,4,8] [--reps 50] [--burst 200] [--out profiles/nbody_simulate.json]

Designs: the generator of tests/nbody_cases.py (separated placements in the box, velocities U(-100, 100) px/s, fp32).  Per body count,
after five warm-up calls: ``ms_per_call`` = median over ``--reps`` calls, each between two device events (input already float64 on the
device: the launch alone, with its three output allocations); ``ms_per_call_burst`` = a host clock around ``--burst`` back-to-back calls
that ends in a device synchronise, over the count (a single call is far shorter than a timer's noise).  ``events_per_design``: contacts
resolved.  ``max_deviation_px``: largest |kernel - host statement| over every output, the statement being tests/nbody_cases.py run
on the host for all designs; ``max_deviation_over_s_case``: the largest ratio of a design's deviation to its s_case (the statement's own
deviation under a +-2^-52 perturbation of the inputs) -- the quantity tests/test_gpu_nbody_sim.py bounds by 64 (events + n_steps).
``reference_cap``: what the reference's simulator cannot beat, DERIVED from its code, not measured (pymunk / pygame are not installed
where this ran): run_simulation calls clock.tick(60) once per step (utils.py:1065), so a design of n_steps frames takes at least
n_steps / 60 s of wall time and the loop over designs is serial.  The last line is JSON, also written to ``--out``."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ap = argparse.ArgumentParser()
ap.add_argument("B", nargs="?", type=int, default=1000)
ap.add_argument("n_steps", nargs="?", type=int, default=92)
ap.add_argument("--bodies", default="2,4,8")
ap.add_argument("--reps", type=int, default=50)
ap.add_argument("--burst", type=int, default=200)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nbody_simulate.json"))
args = ap.parse_args()
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import cindm_amd               # noqa: E402
import nbody_cases as N        # noqa: E402

if not torch.cuda.is_available():
    sys.exit("bench_simulate: no ROCm device (there is no CPU timing)")
B, T = args.B, args.n_steps
dev = torch.device("cuda:0")
res = {"B": B, "n_steps": T, "reps": args.reps, "burst": args.burst, "device": torch.cuda.get_device_name(0),
       "reference_cap": {"steps_per_s": 60, "s_per_design": T / 60.0, "s_per_call": B * T / 60.0,
                         "source": "derived from clock.tick(60) in run_simulation (utils.py:1065) and the serial loop over designs "
                                   "(utils.py:1089); NOT measured"}}
for nb in (int(v) for v in args.bodies.split(",")):
    feats = N.generator_cases(nb, B)
    x = torch.tensor(np.array(feats)).to(dev).double()
    for _ in range(5):
        out, (status, events) = cindm_amd.simulation(x, T, return_status=True)
    torch.cuda.synchronize()
    ms = []
    for _ in range(args.reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        cindm_amd.simulation(x, T)
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    t0 = time.perf_counter()
    for _ in range(args.burst):
        cindm_amd.simulation(x, T)
    torch.cuda.synchronize()
    burst = (time.perf_counter() - t0) / args.burst * 1e3
    want, st, ev, _ = N.simulate(feats, T)
    got = out.cpu().numpy()
    dev_px = np.abs(got - want).reshape(B, -1).max(1)
    s = np.array([N.sensitivity(feats[i], T, base=want[i]) for i in range(B)])
    r = {"ms_per_call": statistics.median(ms), "ms_per_call_min": min(ms), "ms_per_call_max": max(ms), "ms_per_call_burst": burst,
         "designs_per_s": B / (statistics.median(ms) * 1e-3), "events_per_design_mean": float(ev.mean()), "events_per_design_max": int(ev.max()),
         "status_nonzero": int((status.cpu().numpy() != 0).sum()), "status_and_events_equal_host": bool(
             np.array_equal(status.cpu().numpy(), st) and np.array_equal(events.cpu().numpy(), ev)),
         "max_deviation_px": float(dev_px.max()), "s_case_max_px": float(s.max()),
         "max_deviation_over_s_case": float((dev_px / np.maximum(s, 1e-300)).max()),
         "speedup_over_reference_cap": (B * T / 60.0) / (statistics.median(ms) * 1e-3)}
    res[f"bodies_{nb}"] = r
    print(f"{nb} bodies: {r['ms_per_call']:.3f} ms per call of {B} designs x {T} frames (median of {args.reps}; burst {burst:.3f} ms), "
          f"{r['events_per_design_mean']:.1f} events per design, deviation {r['max_deviation_px']:.2e} px = {r['max_deviation_over_s_case']:.3g} s_case",
          flush=True)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
print(json.dumps(res))
