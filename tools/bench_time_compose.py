"""Wall time of the two time-composition samplers at the same (B, K, S), synthetic generator-defined weights, horizon-24 U-Net
(Lc 4, R 20, F 8), eta 0:
  parallel        GaussianDiffusion1D.composing_time_sample: ONE DDIM chain of S steps on K * B rows;
  autoregressive  GaussianDiffusion1D.autoregress_time_compose_sample: K DDIM chains of S steps on B rows, one after the other.
The two are different algorithms with different results; what is compared is the time a K-segment rollout of B designs takes.
They run alternately in this process, each call ending in a device synchronise: one warm-up call each, then the median and the
spread (min .. max) of --reps calls.  Launches per step are what the library emitted for the last captured step
(cindm_ddpm1d_last_step_info), not a model of it.
    python3 tools/bench_time_compose.py [--batches 16,64,256] [--segments 3] [--steps 250] [--reps 5] [--out profiles/time_compose_parallel.json]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import cindm_amd                                               # noqa: E402
from cindm_amd.synthetic import synthetic_init_                # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="16,64,256")
    ap.add_argument("--segments", type=int, default=3)
    ap.add_argument("--steps", type=int, default=250, help="DDIM steps S (sampling_timesteps)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "time_compose_parallel.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_time_compose.py needs a ROCm device")
    dev = torch.device("cuda:0")
    K, S = args.segments, args.steps
    m = synthetic_init_(cindm_amd.TemporalUnet1D(24, 8, False, attention=True), 0).to(dev)
    d = cindm_amd.GaussianDiffusion1D(m, image_size=20, conditioned_steps=4, timesteps=1000, sampling_timesteps=S, loss_type="l1",
                                      ddim_sampling_eta=0.0).to(dev)
    rows = []
    for B in (int(b) for b in args.batches.split(",")):
        cond = (torch.rand((B, 4, 8), generator=torch.Generator().manual_seed(B)) - 0.5).to(dev)
        runs = {"parallel": lambda: torch.cat(d.composing_time_sample((B, 20, 8), cond, n_composed=K - 1, seed=1), dim=1),
                "autoregressive": lambda: d.autoregress_time_compose_sample(B, cond, K - 1, seed=1)}
        times, launches = {n: [] for n in runs}, {}

        def timed(name):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = runs[name]()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            assert tuple(out.shape) == (B, K * 20, 8) and bool(torch.isfinite(out).all()), name
            launches[name] = d.last_step_info()[0]
            return dt

        for name in runs:
            timed(name)
        for _ in range(args.reps):
            for name in runs:                         # alternate the two samplers
                times[name].append(timed(name))
        for name, seq in (("parallel", S), ("autoregressive", K * S)):
            med = statistics.median(times[name])
            rows.append({"sampler": name, "batch": B, "segments": K, "ddim_steps": S, "rows_per_step": K * B if name == "parallel" else B,
                         "sequential_steps": seq, "reps": args.reps, "s_per_rollout_median": round(med, 5),
                         "s_per_rollout_min": round(min(times[name]), 5), "s_per_rollout_max": round(max(times[name]), 5),
                         "us_per_step": round(1e6 * med / seq, 1), "designs_per_s": round(B / med, 1), "launches_per_step": launches[name]})
        par, aut = rows[-2], rows[-1]
        par["rollout_time_vs_autoregressive"] = round(par["s_per_rollout_median"] / aut["s_per_rollout_median"], 4)
        for r in rows[-2:]:
            print(json.dumps(r), flush=True)
    result = {"tool": "tools/bench_time_compose.py", "device": torch.cuda.get_device_name(0), "shape": {"Lc": 4, "R": 20, "F": 8, "horizon": 24, "eta": 0.0},
              "timing": "host clock around one call ending in a device synchronise; median of reps, the two samplers alternating", "rows": rows}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
