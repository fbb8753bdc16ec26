"""Cost of the Langevin (ULA) phase of GaussianDiffusion1D.sample_compose_multibodies against the DDPM step of the same
composition, in one process on the same handles, synthetic generator-defined weights (4 bodies, horizon 24 = 4 + 20):
  (i)   us per Langevin iteration: the Langevin chain alone over t = N-1 .. 401 with L iterations per timestep
        (sample_compose_multibodies(N, L, t_stop=401): one cindm_ddpm1d_sample_ula call);
  (ii)  us per DDPM step of sample_compose_multibodies(N = 400, L = 0): 400 cfg4 steps (cindm_ddpm1d_sample);
  (iii) the whole two-phase sampler sample_compose_multibodies(N, L): designs / s.
The two chains are run alternately, REPS times each after one warm-up; medians and ranges are reported, and the ratio
(i) / (ii) of the medians.
    python3 tools/bench_ula.py [--batch 128] [--N 1000] [--L 2] [--reps 7]"""
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
from cindm_amd.schedule import beta_schedule                   # noqa: E402
from cindm_amd.synthetic import synthetic_init_                # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--N", type=int, default=1000)
    ap.add_argument("--L", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ula.py needs a ROCm device")
    dev = torch.device("cuda:0")
    B, N, L = args.batch, args.N, args.L
    m8 = synthetic_init_(cindm_amd.TemporalUnet1D(24, 8, False, attention=True), 0).to(dev)
    m4 = synthetic_init_(cindm_amd.TemporalUnet1D(24, 4, False, attention=True), 1).to(dev)
    d = cindm_amd.GaussianDiffusion1D(m8, image_size=20, conditioned_steps=4, timesteps=1000, sampling_timesteps=1000, loss_type="l1",
                                      betas_inference=beta_schedule("linear", N)).to(dev)
    d.model_unconditioned = m4
    cond = torch.rand((B, 4, 16), generator=torch.Generator().manual_seed(0)).to(dev)
    n_it = (N - 401) * L
    runs = {"langevin": (lambda: d.sample_compose_multibodies(cond, N, L, 4, seed=1, t_stop=401), n_it),
            "ddpm": (lambda: d.sample_compose_multibodies(cond, 400, 0, 4, seed=1), 400),
            "two_phase": (lambda: d.sample_compose_multibodies(cond, N, L, 4, seed=1), n_it + 401)}

    def timed(name):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = runs[name][0]()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        assert bool(torch.isfinite(out).all()), name
        return dt

    for name in runs:                      # warm-up: weight packing, workspace, graph capture
        timed(name)
    t = {name: [] for name in runs}
    for _ in range(args.reps):
        for name in ("langevin", "ddpm"):  # alternate the two chains whose ratio is reported
            t[name].append(timed(name))
    for _ in range(max(3, args.reps // 2)):
        t["two_phase"].append(timed("two_phase"))
    info = d.last_chain_info()
    us = {}
    for name, (_, n) in runs.items():
        per = [1e6 * v / n for v in t[name]]
        us[name] = statistics.median(per)
        print(json.dumps({"config": name, "batch": B, "N": N, "L": L, "steps": n, "reps": len(per),
                          "us_per_step_median": round(us[name], 2), "us_per_step_min": round(min(per), 2),
                          "us_per_step_max": round(max(per), 2), "s_per_chain_median": round(statistics.median(t[name]), 4),
                          "designs_per_s": round(B / statistics.median(t[name]), 1)}), flush=True)
    print(json.dumps({"langevin_iteration_over_ddpm_step": round(us["langevin"] / us["ddpm"], 4), "recovered": info["recovered"],
                      "exchange_free_up_front": info["exchange_free_up_front"]}), flush=True)


if __name__ == "__main__":
    main()
