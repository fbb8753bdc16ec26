"""The second-order multistep solver (``solver="dpmpp-2m"``) against the DDIM chain of the same tree: time per step
at four shapes, and designs/s at S = 25 and S = 50 beside DDIM at S = 250.

    python tools/bench_multistep.py [--reps 5] [--only a,b,...] [--ddim-only] [--out profiles/multistep.json]

Every pair (the DDIM chain, the multistep chain) runs in one process, alternating, ``--reps`` times each after one warm-up of
both; every timing is a host clock around a call that ends in a device synchronise; the median is reported with the spread
(max - min) / median of the runs.  Shapes:
    cfg2-ddim250     256 designs, TemporalUnet1D(dim=64, horizon=24), unguided, S = 250 (bench.py's cfg2-ddim250).  The DDIM step
                     runs its update inside the U-Net's last kernel; the multistep step launches it: one launch more.
    three-windows    256 designs, three 24-row windows (compose_start_step 16, 56 rows), PointObjective under
                     "standard-recurrence-1", S = 50.  ddim_sample's state is one window, so both chains are issued through
                     _run_guided_ddim on a three-window descriptor.
    2d               64 designs x 2 boundaries, unguided, the first 40 steps of S = 250
    2d-force         64 designs x 2 boundaries, ForceObjective under "standard-alpha", the first 40 steps of S = 250
    designs-per-s    whole chains: 1-D (256 designs) and 2-D (64 x 2, unguided), multistep at S = 25 and S = 50, DDIM at S = 250
``--ddim-only`` times the DDIM chains alone (a tree without the solver can run it: the parent's side of an A/B over processes).
Synthetic generator-defined weights: the figures are costs, not design quality.  The last line is JSON, also written to ``--out``."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--only", default="cfg2-ddim250,three-windows,2d,2d-force,designs-per-s")
ap.add_argument("--ddim-only", action="store_true")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multistep.json"))
args = ap.parse_args()
sys.path.insert(0, ROOT)
import cindm_amd                                   # noqa: E402
from cindm_amd.synthetic import synthetic_init_    # noqa: E402

if not torch.cuda.is_available():
    sys.exit("bench_multistep: no ROCm device (there is no CPU timing)")
dev = torch.device("cuda:0")
only = set(args.only.split(","))
SOLVERS = ("ddim",) if args.ddim_only else ("ddim", "dpmpp-2m")
HZ = 24


def timed(routes):
    """routes: name -> callable returning a tensor (or a tuple that starts with one).  -> name -> list of seconds."""
    def run(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        out = out[0] if isinstance(out, tuple) else out
        assert bool(torch.isfinite(out).all())
        return dt
    for fn in routes.values():                     # warm-up: code objects, graph capture, workspaces
        run(fn)
    times = {n: [] for n in routes}
    for _ in range(args.reps):
        for n, fn in routes.items():
            times[n].append(run(fn))
    return times


def summary(ts, steps, designs):
    med = statistics.median(ts)
    return {"ms_per_step": med / steps * 1e3, "s_per_chain": med, "designs_per_s": designs / med, "steps": steps,
            "spread": (max(ts) - min(ts)) / med, "runs_s": [round(t, 5) for t in ts]}


def kw_of(solver):
    return {} if solver == "ddim" else {"solver": solver}      # (a tree without the keyword runs --ddim-only)


def pair(name, make, steps, designs):
    ts = timed({s: make(s) for s in SOLVERS})
    out = {s: summary(ts[s], steps, designs) for s in SOLVERS}
    if len(SOLVERS) == 2:
        out["multistep_over_ddim_per_step"] = out["dpmpp-2m"]["ms_per_step"] / out["ddim"]["ms_per_step"]
        out["extra_us_per_step"] = (out["dpmpp-2m"]["ms_per_step"] - out["ddim"]["ms_per_step"]) * 1e3
    for s in SOLVERS:
        print(f"{name} {s}: {out[s]['ms_per_step']:.4f} ms/step (median of {args.reps}, spread {100 * out[s]['spread']:.1f} %)", flush=True)
    return out


res = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "solvers": list(SOLVERS)}
m1 = synthetic_init_(cindm_amd.TemporalUnet1D(HZ, 8, False, dim=64, attention=True), 0).to(dev)


def diff1(S):
    return cindm_amd.GaussianDiffusion1D(m1, image_size=HZ, conditioned_steps=0, timesteps=1000, sampling_timesteps=S).to(dev)


if "cfg2-ddim250" in only:
    d = diff1(250)
    res["cfg2-ddim250"] = pair("cfg2-ddim250", lambda s: (lambda: d.sample(batch_size=256, seed=1, **kw_of(s))), 250, 256)
    launches = {}
    for s in SOLVERS:
        d.sample(batch_size=256, seed=1, **kw_of(s))
        launches[s] = d.last_step_info()[0]
    res["cfg2-ddim250"]["launches_per_step"] = launches

if "three-windows" in only:
    S, B, L = 50, 256, HZ + 2 * 16
    d = diff1(S)
    obj = cindm_amd.PointObjective([0.25, -0.5], 2, coef=2.0)
    guid = "standard-recurrence-1"
    desc = d._desc_for((B, L, 8), "mean-inside", 2, 16, HZ, 2, clip=True)
    dz, _ = d._builtin(obj, guid, B, L, 2)
    times, coefs = d.ddim_schedule()
    x_T = d._init_state((B, L, 8), dev, None, 1, 0, 1000)

    def chain(s):
        def run():
            img = x_T.clone()
            ms = None if s == "ddim" else d._multistep(True, 0, S, None, img)
            extra = {} if ms is None else {"ms": ms}
            return d._run_guided_ddim(img, None, desc, dz, times, coefs, noise=None, seed=1, sample_offset=0, inpaint_cond=None,
                                      initial_state_overwrite=None, **extra)
        return run
    res["three-windows"] = pair("three-windows", chain, S, B)

u = force = None
if only & {"2d", "2d-force", "designs-per-s"}:
    u = synthetic_init_(cindm_amd.Unet(dim=64, dim_mults=(1, 2), channels=21, image_size=64), 0).to(dev)


def diff2(S):
    return cindm_amd.GaussianDiffusion(u, image_size=64, frames=6, timesteps=1000, sampling_timesteps=S).to(dev)


SHAPE2, SEG = (64, 2, 21, 64, 64), 40
if "2d" in only:
    d = diff2(250)
    res["2d"] = pair("2d", lambda s: (lambda: d.ddim_sample(SHAPE2, seed=1, step_range=(0, SEG), **kw_of(s))), SEG, 64)

if "2d-force" in only:
    d = diff2(250)
    force = synthetic_init_(cindm_amd.ForceUnet(dim=64, dim_mults=(1, 2, 4, 8), channels=4), seed=7).to(dev)
    fn = cindm_amd.ForceObjective(force, 64, 2, 6, p_min=-37.7, p_max=57.6)
    res["2d-force"] = pair("2d-force", lambda s: (lambda: d.ddim_sample(SHAPE2, design_fn=fn, design_guidance="standard-alpha", seed=1,
                                                                        step_range=(0, SEG), **kw_of(s))), SEG, 64)
    res["2d-force"]["recovered_chains"] = force.recovered

if "designs-per-s" in only:
    rows = {}
    for label, mk, designs, call in (("1d", diff1, 256, lambda d, s: d.sample(batch_size=256, seed=1, **kw_of(s))),
                                     ("2d", diff2, 64, lambda d, s: d.sample(batch_size=64, num_boundaries=2, seed=1, **kw_of(s)))):
        routes, meta = {}, {}
        cases = [("ddim", 250)] + ([] if args.ddim_only else [("dpmpp-2m", 25), ("dpmpp-2m", 50)])
        for s, S in cases:
            d = mk(S)
            routes[f"{s}@{S}"] = (lambda d=d, s=s: call(d, s))
            meta[f"{s}@{S}"] = S
        ts = timed(routes)
        rows[label] = {n: summary(ts[n], meta[n], designs) for n in routes}
        for n in routes:
            print(f"designs/s {label} {n}: {rows[label][n]['designs_per_s']:.2f} ({rows[label][n]['s_per_chain']:.3f} s/chain)", flush=True)
    res["designs-per-s"] = rows

line = json.dumps(res)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
print(line)
