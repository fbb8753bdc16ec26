"""TemporalUnet1D at dim = 96 (the generic tier: three launches per residual block and per attention site, GroupNorm statistics per
segment -- DESIGN 4.14) on the plain DDPM library chain, against the same model on the fp32-MFMA kernels and against the dim-64
model at the same horizon (fused level kernels, dconv, attention sites).

    python tools/bench_dim96.py [B=256] [steps=200] [--reps 5] [--merge key=file.json ...] [--out profiles/unet_dim96.json]

Shape: horizon 44, F = 8, dim_mults (1, 2, 4, 8), attention; n_composed = 0; the first ``steps`` reverse steps of the graph-captured
DDPM chain (every step costs the same), counter-based noise.  Routes, run alternating in one process, each after one warm-up,
``--reps`` times; every timing is a host clock around a call that ends in a device synchronise:
    dim96          dim 96, default plan (split-fp16 convolutions)
    dim96_f32      dim 96, set_option("mfma_f32", 1)
    dim64          dim 64 at the same horizon
Also recorded: launches per forward of each, profile() per kernel kind of dim96, the algorithmic FLOPs per row of dim96 and dim64
computed from the layer shapes, and for dim96 the executed-over-algorithmic ratio of the split-fp16 convolutions that comes from
padding every source's Cin to whole 128-channel K stages.  ``--merge key=file.json`` copies other measurements of the same session
(the dim-64 bit comparison of tools/dump_eps_dim64.py, an A/B of bench.py against the parent commit) into the record under ``key``.
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
ap.add_argument("steps", nargs="?", type=int, default=200, help="reverse steps per chain")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--merge", action="append", default=[], metavar="KEY=FILE")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "unet_dim96.json"))
args = ap.parse_args()
sys.path.insert(0, ROOT)
import cindm_amd                                   # noqa: E402
from cindm_amd.synthetic import synthetic_init_    # noqa: E402

HZ, F, MULTS = 44, 8, (1, 2, 4, 8)


def layers(hz, F, dim, mults, attention=True):
    """The GEMM layers of one forward in order: (name, kind, L_out, (Cin of every concatenated source), Cout, algorithmic taps)."""
    dims = [F] + [dim * m for m in mults]
    nres = len(mults)
    n_plain = 1 if hz % 8 == 0 else 2 if hz % 4 == 0 else 3
    out, L = [], hz

    def rtb(p, L, cins, co):
        out.append((p + ".blocks.0", "conv5", L, cins, co, 5.0))
        out.append((p + ".blocks.1", "conv5", L, (co,), co, 5.0))
        if sum(cins) != co:
            out.append((p + ".residual_conv", "res1x1", L, cins, co, 1.0))

    def attn(p, L, c):
        if attention:
            out.append((p + ".to_qkv", "1x1", L, (c,), 384, 1.0))
            out.append((p + ".core", "attention", L, (), 0, 0.0))
            out.append((p + ".to_out", "1x1", L, (128,), c, 1.0))
    for ind in range(nres):
        ci, co = dims[ind], dims[ind + 1]
        rtb(f"downs.{ind}.0", L, (ci,), co); rtb(f"downs.{ind}.1", L, (co,), co); attn(f"downs.{ind}.2", L, co)
        if ind < nres - n_plain:
            L //= 2
            out.append((f"downs.{ind}.3", "conv3", L, (co,), co, 3.0))
    mid = dims[nres]
    rtb("mid_block1", L, (mid,), mid); attn("mid_attn", L, mid); rtb("mid_block2", L, (mid,), mid)
    for ind in range(nres - 1):
        ci, co = dims[nres - 1 - ind], dims[nres - ind]
        rtb(f"ups.{ind}.0", L, (co, co), co); rtb(f"ups.{ind}.1", L, (co,), ci); attn(f"ups.{ind}.2", L, ci)
        if ind >= n_plain - 1:
            L *= 2
            out.append((f"ups.{ind}.3", "convT4", L, (ci,), ci, 2.0))          # 2 of the 4 taps hit every output position
    out.append(("final_conv.0", "conv5", L, (dim,), dim, 5.0))
    out.append(("final_conv.1", "1x1", L, (dim,), F, 1.0))
    return out


def flops_per_row(ls):
    """Algorithmic FLOPs of one sample; and, over the layers the split-fp16 convolution kernel runs (k = 5 and the 1x1 residual_conv that
    rides on it, k = 3, k = 4), algorithmic and executed with every source's Cin padded to whole 128-channel stages."""
    alg = h3_alg = h3_exe = 0.0
    for _, kind, L, cins, co, taps in ls:
        if kind == "attention":
            alg += 4 * (2.0 * 32 * 32 * L * 2)
            continue
        f = 2.0 * L * co * sum(cins) * taps
        alg += f
        if kind in ("conv5", "res1x1", "conv3", "convT4"):
            h3_alg += f
            h3_exe += 2.0 * L * co * sum(-(-c // 128) * 128 for c in cins) * taps
    return alg, h3_alg, h3_exe


if not torch.cuda.is_available():
    sys.exit("bench_dim96: no ROCm device (there is no CPU timing)")
B, S = args.B, args.steps
dev = torch.device("cuda:0")


def build(dim, **opts):
    m = synthetic_init_(cindm_amd.TemporalUnet1D(HZ, F, False, dim=dim, dim_mults=MULTS, attention=True), 0)
    for k, v in opts.items():
        m.set_option(k, v)
    m = m.to(dev)
    return m, cindm_amd.GaussianDiffusion1D(m, image_size=HZ, conditioned_steps=0, timesteps=1000, sampling_timesteps=1000).to(dev)


models = {"dim96": build(96), "dim96_f32": build(96, mfma_f32=1), "dim64": build(64)}
text = {"dim96": "dim 96, default plan", "dim96_f32": "dim 96, mfma_f32 = 1", "dim64": "dim 64, default plan"}
kw = dict(batch_size=B, n_composed=0, compose_n_bodies=2, seed=1, t_stop=1000 - S)
times = {n: [] for n in models}
outs = {}
for n, (m, d) in models.items():                   # warm-up: code objects, finalize, graph capture, workspace
    outs[n] = d.sample(**kw).clone()
torch.cuda.synchronize()
for _ in range(args.reps):
    for n, (m, d) in models.items():
        t0 = time.perf_counter()
        d.sample(**kw)
        torch.cuda.synchronize()
        times[n].append(time.perf_counter() - t0)
res = {"B": B, "steps": S, "horizon": HZ, "F": F, "dim_mults": list(MULTS), "reps": args.reps, "device": torch.cuda.get_device_name(0)}
for n, (m, d) in models.items():
    med, lo, hi = statistics.median(times[n]), min(times[n]), max(times[n])
    res[n] = {"us_per_reverse_step": med / S * 1e6, "designs_per_s_1000_steps": B / (med / S * 1000), "spread": (hi - lo) / med,
              "chain_s": [round(t, 4) for t in times[n]], "launches_per_forward": int(m.launches_per_forward),
              "range_fallback": int(m.get_option("range_fallback")), "recovered_chains": int(m.recovered),
              "result_finite": bool(torch.isfinite(outs[n]).all())}
    print(f"{text[n]}: B={B} steps={S}: {med / S * 1e6:.1f} us per reverse step, {res[n]['launches_per_forward']} launches per forward "
          f"(median of {args.reps}, spread {100 * (hi - lo) / med:.1f} %)", flush=True)
# per kernel kind, one instrumented forward of the default dim-96 plan (events around every launch: sums exclude the gaps between launches)
x = torch.randn((B, HZ, F), generator=torch.Generator().manual_seed(3)).to(dev)
for n in ("dim96", "dim96_f32"):
    prof = models[n][0].profile(x, 500)
    res[n]["profile"] = {k: {"launches": c, "us": ms * 1e3, "algorithmic_gflop": fl * 1e-9} for k, (c, ms, fl) in prof.items() if c}
    res[n]["profile_sum_us"] = sum(v["us"] for v in res[n]["profile"].values())
for n, dim in (("dim96", 96), ("dim64", 64)):
    alg, h3a, h3e = flops_per_row(layers(HZ, F, dim, MULTS))
    res[n]["algorithmic_mflop_per_row"] = alg * 1e-6
    res[n]["conv_h3_algorithmic_mflop_per_row"] = h3a * 1e-6
    res[n]["conv_h3_executed_over_algorithmic_cin_padding"] = h3e / h3a
res["dim96"]["profile_algorithmic_mflop_per_row"] = sum(v["algorithmic_gflop"] for v in res["dim96"]["profile"].values()) * 1e3 / B
res["time_dim96_over_dim64"] = res["dim96"]["us_per_reverse_step"] / res["dim64"]["us_per_reverse_step"]
res["flop_dim96_over_dim64"] = res["dim96"]["algorithmic_mflop_per_row"] / res["dim64"]["algorithmic_mflop_per_row"]
res["time_dim96_over_dim96_f32"] = res["dim96"]["us_per_reverse_step"] / res["dim96_f32"]["us_per_reverse_step"]
print(f"dim96 / dim64: time {res['time_dim96_over_dim64']:.3f}, algorithmic FLOPs {res['flop_dim96_over_dim64']:.3f};  "
      f"dim96 split-fp16 / fp32-MFMA time: {res['time_dim96_over_dim96_f32']:.3f};  Cin padding of the split-fp16 convolutions: "
      f"x {res['dim96']['conv_h3_executed_over_algorithmic_cin_padding']:.3f} executed over algorithmic")
for item in args.merge:
    key, path = item.split("=", 1)
    with open(path) as f:
        res[key] = json.load(f)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
print(json.dumps(res))
