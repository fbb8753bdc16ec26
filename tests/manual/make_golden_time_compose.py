"""TEST INFRASTRUCTURE ONLY.  Golden vectors for the parallel time composition (GaussianDiffusion1D.composing_time_sample,
model/diffusion_1d.py:1807-1854), captured from the reference's own method on the CPU with the synthetic generator-defined
weights (cindm_oracle.synth_state_dict); needs the reference tree (oracle/ref_import.py, read-only).
    python tests/manual/make_golden_time_compose.py [parallel] [objectives]        # well under a minute; default: both files
Writes tests/golden/time_compose_parallel.npz (the pred_noise cases) and tests/golden/time_compose_objectives.npz (the pred_x0 /
pred_v cases, with ``<tag>.clamp_share_min``), compressed.

Per case <tag>: cond [B, Lc, F]; the tapes -- init [K, B, R, F] (the reference's SECOND torch.randn, img_infered's x_T, :1815) and
step [S, K, B, R, F] (the randn_like of every DDIM step, :1837, drawn even when sigma == 0 and on the last step); img [B, R, F] and
img_infered [B, (K - 1) min(20, R), F] (what the method returns); states [S, K, B, R, F], the state after EVERY step (unclamped
between steps: what the next step's hand-over reads; taken from the argument of the next step's randn_like, the last one from
the returned tensors, which hold every row for R <= 20).  The reference's other four randn draws (img, cond_infered's rows,
x_start_infered, pred_noise_infered, img_temp) are never read -- the rows of cond_infered for k >= 1 are overwritten before
their first use -- and are arbitrary here.

A case is written only if (1) the reference stays within TOL_CHAIN / 4 of a float64 restatement of the same loop at every step and
(2) fewer than half of the returned elements sit on the clamp (|x| = 1) and, for the pred_x0 / pred_v cases, (3) at every step with
time_next >= 0 at least 0.5 % of the float64 x_start lies on the clamp -- there the noise re-derived from the clamped x_start
(:1018-1027) differs from the unclamped one's.  If a case fails (1) or (2), change its S or its cond scale, never a tolerance; if
it fails (3), change its seed, within four tries, never the condition."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import cindm_oracle as O          # noqa: E402
import ref_import                 # noqa: E402
from make_golden import build_ref_unet, relerr          # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
TOL_CHAIN = 1e-4                  # tests/test_gpu_parity.py
F, B = 8, 5

# tag: (horizon, Lc, R, K, S, eta, cond scale, seed, objective)
CASES = {
    "default": (24, 4, 20, 3, 6, 0.0, 1.0, 5201, "pred_noise"),
    "stochastic": (24, 4, 20, 3, 6, 0.5, 1.0, 5202, "pred_noise"),
    "whole_state": (8, 4, 4, 4, 6, 0.0, 1.0, 5203, "pred_noise"),
    "two_segment": (24, 4, 20, 2, 4, 0.0, 1.0, 5204, "pred_noise"),
    "pred_x0_eta0.0": (24, 4, 20, 3, 6, 0.0, 1.0, 5301, "pred_x0"),
    "pred_x0_eta0.5": (24, 4, 20, 3, 6, 0.5, 1.0, 5301, "pred_x0"),
    "pred_v_eta0.0": (24, 4, 20, 3, 6, 0.0, 1.0, 5301, "pred_v"),
    "pred_v_eta0.5": (24, 4, 20, 3, 6, 0.5, 1.0, 5301, "pred_v"),
}
FILES = {"parallel": "time_compose_parallel.npz", "objectives": "time_compose_objectives.npz"}
MIN_CLAMP_SHARE = 0.005


def restated(od, cond, init, step, S, eta, shares=None):
    """The loop of :1823-1846 on cindm_oracle.model_predictions / ddim_coefs, in the dtype of its arguments.  Returns the state
    after every step [S, K * B, R, F]; ``shares`` receives the share of x_start on the clamp at every step with time_next >= 0."""
    K, Bn = init.shape[0], init.shape[1]
    x = init.reshape((K * Bn,) + tuple(init.shape[2:])).clone()
    c = torch.zeros((K * Bn, cond.shape[1], cond.shape[2]), dtype=x.dtype)
    c[:Bn] = cond
    states = []
    for i, (time, time_next) in enumerate(O.ddim_time_pairs(od.num_timesteps, S)):
        c[Bn:] = x[:(K - 1) * Bn, -od.conditioned_steps:]
        pred_noise, x_start = O.model_predictions(od, x, c, time, clip_x_start=True)
        san, cc, sigma = O.ddim_coefs(od, time, time_next, eta)
        x = x_start if time_next < 0 else x_start * san + cc * pred_noise + sigma * step[i].reshape(x.shape)
        states.append(x.clone())
        if shares is not None and time_next >= 0:
            shares.append(float((x_start.abs() == 1.0).double().mean()))
    return torch.stack(states)


def run_reference(gd, cond, init, step, K, R):
    """The reference's method with torch.randn / randn_like replaced inside its module: returns (img, img_infered, states)."""
    seen, n_randn = [], [0]
    filler = torch.Generator().manual_seed(99)

    def randn(*size, **kw):
        size = tuple(size[0]) if len(size) == 1 and isinstance(size[0], (tuple, list, torch.Size)) else tuple(size)
        n_randn[0] += 1
        if n_randn[0] == 2:
            assert size == (K * B, R, F), size
            return init.reshape(size).clone()
        return torch.randn(size, generator=filler)

    def randn_like(x, **kw):
        seen.append(x.detach().clone())
        return step[len(seen) - 1].reshape(x.shape).clone()

    import types
    d1 = sys.modules[type(gd).__module__]
    shim = types.SimpleNamespace(**{k: getattr(torch, k) for k in dir(torch) if not k.startswith("__")})
    shim.randn, shim.randn_like = randn, randn_like
    keep = d1.torch
    d1.torch = shim
    try:
        img, inf = gd.composing_time_sample((B, R, F), cond, n_composed=K - 1)
    finally:
        d1.torch = keep
    assert n_randn[0] == 6 and len(seen) == step.shape[0], (n_randn[0], len(seen))
    last = torch.cat([img] + [inf[:, (k - 1) * R:k * R] for k in range(1, K)], dim=0)      # R <= 20: every row is returned
    return img, inf, torch.stack(seen[1:] + [last])


def main():
    torch.set_num_threads(8)
    d1, _ = ref_import.import_reference()
    which = [a for a in sys.argv[1:] if a in FILES] or list(FILES)
    out = {k: {} for k in which}
    for tag, (hz, Lc, R, K, S, eta, scale, seed, objective) in CASES.items():
        name = "parallel" if objective == "pred_noise" else "objectives"
        if name not in which:
            continue
        assert R <= 20
        m, sd, _ = build_ref_unet(d1, hz, F)
        gd = d1.GaussianDiffusion1D(m, image_size=R, conditioned_steps=Lc, timesteps=1000, sampling_timesteps=S, loss_type="l1",
                                    ddim_sampling_eta=eta, objective=objective)
        g = torch.Generator().manual_seed(seed)
        cond = (torch.rand((B, Lc, F), generator=g) - 0.5) * scale
        init = torch.randn((K, B, R, F), generator=g)
        step = torch.randn((S, K, B, R, F), generator=g)
        img, inf, states = run_reference(gd, cond, init, step, K, R)
        assert tuple(img.shape) == (B, R, F) and tuple(inf.shape) == (B, (K - 1) * min(20, R), F), (tuple(img.shape), tuple(inf.shape))
        od = O.Diffusion1D(sd, image_size=R, conditioned_steps=Lc, objective=objective)
        r32 = restated(od, cond, init, step, S, eta)
        od64 = O.Diffusion1D({k: v.double() for k, v in sd.items()}, image_size=R, conditioned_steps=Lc, objective=objective)
        od64.tab = {k: v.double() for k, v in od.tab.items()}
        shares = []
        r64 = restated(od64, cond.double(), init.double(), step.double(), S, eta, shares)
        e_oracle = max(relerr(r32[i], states[i]) for i in range(S))
        e64 = max(relerr(states[i].double(), r64[i]) for i in range(S))
        clamped = float(((torch.cat([img.flatten(), inf.flatten()])).abs() == 1.0).float().mean())
        print(f"{tag}: restatement vs reference {e_oracle:.2e}, reference vs float64 {e64:.2e} (bound {TOL_CHAIN / 4:.1e}), "
              f"on the clamp {clamped:.3f}", flush=True)
        assert e64 <= TOL_CHAIN / 4, f"{tag}: the fp32 reference leaves the float64 run: change S or the cond scale"
        assert clamped < 0.5, f"{tag}: half of the returned elements sit on the clamp: change S or the cond scale"
        assert e_oracle <= 2e-6, tag
        if objective != "pred_noise":
            print(f"{tag}: x_start on the clamp per step {[round(v, 4) for v in shares]}", flush=True)
            assert len(shares) == S - 1 and min(shares) >= MIN_CLAMP_SHARE, f"{tag}: under 0.5 % of x_start on the clamp at a step: change the seed"
            out[name][f"{tag}.clamp_share_min"] = np.float32(min(shares))
        for key, v in (("cond", cond), ("init", init), ("step", step), ("img", img), ("img_infered", inf),
                        ("states", states.reshape(S, K, B, R, F))):
            out[name][f"{tag}.{key}"] = v.numpy().astype(np.float32)
    for name in which:
        path = os.path.join(GOLD, FILES[name])
        np.savez_compressed(path, **out[name])
        print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
