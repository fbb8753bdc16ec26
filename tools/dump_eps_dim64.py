"""eps of the dim-64 model on seeded inputs, for a bit comparison of two source trees (a change that must leave the kernels of the
power-of-two widths as they were: the dim-96 work).

    python tools/dump_eps_dim64.py --tree <tree with its built library> --out <dir>      # one process per tree
    python tools/dump_eps_dim64.py --compare <dir A> <dir B> [--json out.json]

Model (24, 8, 64, (1, 2, 4, 8), attention), synthetic weights (cindm_amd.synthetic, seed 0), t = 77; inputs seeded 4100 + B.  Cases: the
default plan at B = 17, 64, 321 and mfma_f32 = 1 at B = 17.  --tree imports cindm_amd from that tree."""
import argparse
import json
import os
import sys

import numpy as np
import torch

CASES = [("default", 17), ("default", 64), ("default", 321), ("mfma_f32", 17)]

ap = argparse.ArgumentParser()
ap.add_argument("--tree")
ap.add_argument("--out")
ap.add_argument("--compare", nargs=2, metavar="DIR")
ap.add_argument("--json")
args = ap.parse_args()

if args.compare:
    a, b = args.compare
    res = {}
    for plan, B in CASES:
        name = f"eps_{plan}_{B}.npy"
        x, y = np.load(os.path.join(a, name)), np.load(os.path.join(b, name))
        res[f"{plan}-{B}"] = {"bit_equal": bool(x.shape == y.shape and np.array_equal(x.view(np.uint32), y.view(np.uint32))),
                              "finite": bool(np.isfinite(x).all() and np.isfinite(y).all()), "max_abs": float(np.abs(x).max())}
    res["all_bit_equal"] = all(v["bit_equal"] for v in res.values())
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    print(json.dumps(res))
    sys.exit(0 if res["all_bit_equal"] else 1)

tree = os.path.abspath(args.tree)
sys.path.insert(0, tree)
import cindm_amd                                   # noqa: E402
from cindm_amd.synthetic import synthetic_init_    # noqa: E402

assert os.path.abspath(cindm_amd.__file__).startswith(tree + os.sep), cindm_amd.__file__
dev = torch.device("cuda:0")
os.makedirs(args.out, exist_ok=True)
for plan in ("default", "mfma_f32"):
    m = synthetic_init_(cindm_amd.TemporalUnet1D(24, 8, False, dim=64, dim_mults=(1, 2, 4, 8), attention=True), 0)
    if plan == "mfma_f32":
        m.set_option("mfma_f32", 1)
    m = m.to(dev)
    for p, B in CASES:
        if p != plan:
            continue
        x = torch.randn((B, 24, 8), generator=torch.Generator().manual_seed(4100 + B)).to(dev)
        eps = m(x, torch.full((B,), 77, device=dev))
        np.save(os.path.join(args.out, f"eps_{plan}_{B}.npy"), eps.cpu().numpy())
        print(f"{tree}: {plan} B={B} launches per forward {m.launches_per_forward} max|eps| {float(eps.abs().max()):.4f}", flush=True)
