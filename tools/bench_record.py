"""The chain recorder (return_trajectory_every=): what it costs when it is on, and that nothing changed when it is off.

    python tools/bench_record.py on  [--steps2d 50] [--reps 3] [--out FILE]
    python tools/bench_record.py off --parent TREE [--rounds 3] [--steps2d 50] [--out FILE]
    python tools/bench_record.py store [--steps2d 50] [--reps 9] [--out FILE]
    python tools/bench_record.py one [--root TREE] ...          (what `off` runs per process; prints one JSON line)

Two chains: the cfg2 shape (1-D, 256 designs, 1000 DDPM steps) and the cfg5 shape (2-D, 64 designs x 2 boundaries, --steps2d DDPM
steps).  Every timing is a host clock around a call that ends in a device synchronise, after one warm-up of every variant.

``on``: in one process, alternating, recorder off against every in {n, 50, 1} for ``x`` alone and for ``x`` + ``x0``; reports the
microseconds per step each variant adds and the microseconds per record (its added time over the records it wrote).
``store``: the 2-D ``every = 1`` chain alone, recorder off and the three store flavours of chain_record_kernel alternating
(CINDM_RECORD_STORE = 0 plain, 1 nt, 2 sc1); a 50 MB copy is about 1 % of a 2-D step, hence the repetitions.  Only the PROFILING build
of the library (CINDM_LIB_VARIANT=prof, ``python -m cindm_amd.build --prof``) has the switch -- the production kernel stores nt -- so
this mode refuses to run on any other.
``off``: this tree against a checkout of the parent commit (``--parent``, built), one fresh process per run, the two alternating
``--rounds`` times.  Reports this / parent per chain, the spread parent-against-parent shows (max / min over the parent's own
runs) and whether the designs are bit-identical (sha256).  The last line is JSON; ``--out`` also writes it to a file."""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("mode", choices=["on", "off", "one", "store"])
ap.add_argument("--root", default=HERE)
ap.add_argument("--parent")
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--steps1d", type=int, default=1000)
ap.add_argument("--steps2d", type=int, default=50)
ap.add_argument("--out")
args = ap.parse_args()


def finish(res):
    line = json.dumps(res)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    print(line)


if args.mode == "off":
    if not args.parent:
        sys.exit("bench_record off: --parent TREE (a built checkout of the parent commit)")
    trees = {"this": HERE, "parent": os.path.abspath(args.parent)}
    runs = {k: [] for k in trees}
    for _ in range(args.rounds):
        for k, root in trees.items():           # one fresh process per run, the two trees alternating
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "one", "--root", root, "--reps", str(args.reps),
                                  "--steps1d", str(args.steps1d), "--steps2d", str(args.steps2d)],
                                 check=True, capture_output=True, text=True, timeout=600).stdout
            runs[k].append(json.loads(out.strip().splitlines()[-1]))
            print(k, runs[k][-1], flush=True)
    res = {"mode": "off", "rounds": args.rounds, "steps1d": args.steps1d, "steps2d": args.steps2d}
    for chain in ("cfg2", "cfg5"):
        us = {k: [r[chain]["us_per_step"] for r in runs[k]] for k in trees}
        sha = {k: sorted({r[chain]["sha256"] for r in runs[k]}) for k in trees}
        res[chain] = {"this_us_per_step": us["this"], "parent_us_per_step": us["parent"],
                      "this_over_parent": statistics.median(us["this"]) / statistics.median(us["parent"]),
                      "parent_spread_max_over_min": max(us["parent"]) / min(us["parent"]),
                      "this_spread_max_over_min": max(us["this"]) / min(us["this"]),
                      "bit_identical": sha["this"] == sha["parent"] and len(sha["this"]) == 1}
        r = res[chain]
        r["inside_parent_spread"] = 1.0 / r["parent_spread_max_over_min"] <= r["this_over_parent"] <= r["parent_spread_max_over_min"]
        print(f"{chain}: this / parent {r['this_over_parent']:.4f}, parent spread x{r['parent_spread_max_over_min']:.4f}, "
              f"bit-identical {r['bit_identical']}", flush=True)
    finish(res)
    sys.exit(0)

sys.path.insert(0, os.path.abspath(args.root))
import torch                                       # noqa: E402
import cindm_amd                                   # noqa: E402
from cindm_amd.synthetic import synthetic_init_    # noqa: E402

if not torch.cuda.is_available():
    sys.exit("bench_record: no ROCm device (there is no CPU timing)")
dev = torch.device("cuda:0")
m1 = synthetic_init_(cindm_amd.TemporalUnet1D(24, 8, False, attention=True), 0).to(dev)
d1 = cindm_amd.GaussianDiffusion1D(m1, image_size=24, conditioned_steps=0, timesteps=1000, sampling_timesteps=1000).to(dev)
m2 = synthetic_init_(cindm_amd.Unet(dim=64, dim_mults=(1, 2), channels=21), 0).to(dev)
d2 = cindm_amd.GaussianDiffusion(m2, image_size=64, frames=6, timesteps=1000).to(dev)
N1, N2 = args.steps1d, args.steps2d
chains = {
    "cfg2": (N1, lambda **kw: d1.sample(batch_size=256, n_composed=0, compose_n_bodies=2, seed=1, t_stop=1000 - N1, **kw)),
    "cfg5": (N2, lambda **kw: d2.sample(batch_size=64, num_boundaries=2, seed=1, t_stop=1000 - N2, **kw)),
}


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


if args.mode == "one":
    res = {"root": os.path.abspath(args.root)}
    for name, (n, run) in chains.items():
        run()
        torch.cuda.synchronize()
        ts, out = [], None
        for _ in range(args.reps):
            dt, out = timed(run)
            ts.append(dt)
        res[name] = {"us_per_step": statistics.median(ts) / n * 1e6,
                     "sha256": hashlib.sha256(out.detach().cpu().numpy().tobytes()).hexdigest()}
    finish(res)
    sys.exit(0)

if args.mode == "store":
    if os.environ.get("CINDM_LIB_VARIANT") != "prof":
        sys.exit("bench_record store: run with CINDM_LIB_VARIANT=prof (only the profiling build can switch the store flavour)")
    n, run = chains["cfg5"]
    pols = {"off": None, "plain": "0", "nt": "1", "sc1": "2"}

    def go(k):
        if pols[k] is None:
            os.environ.pop("CINDM_RECORD_STORE", None)
            return run()
        os.environ["CINDM_RECORD_STORE"] = pols[k]
        return run(return_trajectory_every=1)
    times = {k: [] for k in pols}
    for k in pols:
        go(k)
        torch.cuda.synchronize()
    for _ in range(args.reps):
        for k in pols:
            times[k].append(timed(lambda: go(k))[0])
    os.environ.pop("CINDM_RECORD_STORE", None)
    res = {"mode": "store", "reps": args.reps, "steps2d": n, "record_bytes": 64 * 2 * 64 * 64 * m2.padded_channels * 4}
    for k in pols:
        res[k] = {"us_per_step_median": statistics.median(times[k]) / n * 1e6, "us_per_step_min": min(times[k]) / n * 1e6,
                  "us_per_step_max": max(times[k]) / n * 1e6}
    for k in ("plain", "nt", "sc1"):
        res[k]["us_per_record_median"] = res[k]["us_per_step_median"] - res["off"]["us_per_step_median"]
        res[k]["us_per_record_min"] = res[k]["us_per_step_min"] - res["off"]["us_per_step_min"]
    for k in pols:
        print(k, ", ".join(f"{a} {b:.2f}" for a, b in res[k].items()), flush=True)
    finish(res)
    sys.exit(0)

# mode "on"
res = {"mode": "on", "reps": args.reps, "steps1d": N1, "steps2d": N2}
for name, (n, run) in chains.items():
    variants = {"off": {}}
    for every in (n, 50, 1):
        for traj in (("x",), ("x", "x0")):
            variants[f"every={every} {'+'.join(traj)}"] = dict(return_trajectory_every=every, trajectory=traj)

    def go(key):
        return run(**variants[key])
    times = {k: [] for k in variants}
    base = None
    for k in variants:                              # warm-up: graph capture, record buffers' first touch
        out = go(k)
        out = out[0] if isinstance(out, tuple) else out
        torch.cuda.synchronize()
        base = out if base is None else base
        assert torch.equal(out, base), f"{name} {k}: the recorded chain's designs differ from the unrecorded chain's"
    for _ in range(args.reps):
        for k in variants:
            times[k].append(timed(lambda: go(k))[0])
    off = statistics.median(times["off"])
    rows = {}
    for k in variants:
        med = statistics.median(times[k])
        row = {"us_per_step": med / n * 1e6, "spread": (max(times[k]) - min(times[k])) / med}
        if k != "off":
            every = variants[k]["return_trajectory_every"]
            n_rec = -(-n // every) * len(variants[k]["trajectory"])
            row["added_us_per_step"] = (med - off) / n * 1e6
            row["us_per_record"] = (med - off) / n_rec * 1e6
            row["records"] = n_rec
        rows[k] = row
        print(f"{name} {k}: " + ", ".join(f"{a} {b:.3f}" if isinstance(b, float) else f"{a} {b}" for a, b in row.items()), flush=True)
    res[name] = rows
finish(res)
