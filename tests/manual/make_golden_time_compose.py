"""TEST INFRASTRUCTURE ONLY.  Golden vectors for the parallel time composition (GaussianDiffusion1D.composing_time_sample,
model/diffusion_1d.py:1807-1854), captured from the reference's own method on the CPU with the synthetic generator-defined
weights (cindm_oracle.synth_state_dict); needs the reference tree (oracle/ref_import.py, read-only).
    python tests/manual/make_golden_time_compose.py        # well under a minute
Writes tests/golden/time_compose_parallel.npz (compressed).

Per case <tag>: cond [B, Lc, F]; the tapes -- init [K, B, R, F] (the reference's SECOND torch.randn, img_infered's x_T, :1815) and
step [S, K, B, R, F] (the randn_like of every DDIM step, :1837, drawn even when sigma == 0 and on the last step); img [B, R, F] and
img_infered [B, (K - 1) min(20, R), F] (what the method returns); states [S, K, B, R, F], the state after EVERY step (unclamped
between steps: what the next step's hand-over reads; taken from the argument of the next step's randn_like, the last one from
the returned tensors, which hold every row for R <= 20).  The reference's other four randn draws (img, cond_infered's rows,
x_start_infered, pred_noise_infered, img_temp) are never read -- the rows of cond_infered for k >= 1 are overwritten before
their first use -- and are arbitrary here.

A case is written only if (1) the reference stays within TOL_CHAIN / 4 of a float64 restatement of the same loop at every step and
(2) fewer than half of the returned elements sit on the clamp (|x| = 1).  If a case fails, change its S or its cond scale, never
a tolerance."""
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

# tag: (horizon, Lc, R, K, S, eta, cond scale, seed)
CASES = {
    "default": (24, 4, 20, 3, 6, 0.0, 1.0, 5201),
    "stochastic": (24, 4, 20, 3, 6, 0.5, 1.0, 5202),
    "whole_state": (8, 4, 4, 4, 6, 0.0, 1.0, 5203),
    "two_segment": (24, 4, 20, 2, 4, 0.0, 1.0, 5204),
}


def restated(od, cond, init, step, S, eta):
    """The loop of :1823-1846 on cindm_oracle.model_predictions / ddim_coefs, in the dtype of its arguments.  Returns the state
    after every step [S, K * B, R, F]."""
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
    out = {}
    for tag, (hz, Lc, R, K, S, eta, scale, seed) in CASES.items():
        assert R <= 20
        m, sd, _ = build_ref_unet(d1, hz, F)
        gd = d1.GaussianDiffusion1D(m, image_size=R, conditioned_steps=Lc, timesteps=1000, sampling_timesteps=S, loss_type="l1",
                                    ddim_sampling_eta=eta)
        g = torch.Generator().manual_seed(seed)
        cond = (torch.rand((B, Lc, F), generator=g) - 0.5) * scale
        init = torch.randn((K, B, R, F), generator=g)
        step = torch.randn((S, K, B, R, F), generator=g)
        img, inf, states = run_reference(gd, cond, init, step, K, R)
        assert tuple(img.shape) == (B, R, F) and tuple(inf.shape) == (B, (K - 1) * min(20, R), F), (tuple(img.shape), tuple(inf.shape))
        od = O.Diffusion1D(sd, image_size=R, conditioned_steps=Lc)
        r32 = restated(od, cond, init, step, S, eta)
        od64 = O.Diffusion1D({k: v.double() for k, v in sd.items()}, image_size=R, conditioned_steps=Lc)
        od64.tab = {k: v.double() for k, v in od.tab.items()}
        r64 = restated(od64, cond.double(), init.double(), step.double(), S, eta)
        e_oracle = max(relerr(r32[i], states[i]) for i in range(S))
        e64 = max(relerr(states[i].double(), r64[i]) for i in range(S))
        clamped = float(((torch.cat([img.flatten(), inf.flatten()])).abs() == 1.0).float().mean())
        print(f"{tag}: restatement vs reference {e_oracle:.2e}, reference vs float64 {e64:.2e} (bound {TOL_CHAIN / 4:.1e}), "
              f"on the clamp {clamped:.3f}", flush=True)
        assert e64 <= TOL_CHAIN / 4, f"{tag}: the fp32 reference leaves the float64 run: change S or the cond scale"
        assert clamped < 0.5, f"{tag}: half of the returned elements sit on the clamp: change S or the cond scale"
        assert e_oracle <= 2e-6, tag
        for name, v in (("cond", cond), ("init", init), ("step", step), ("img", img), ("img_infered", inf),
                        ("states", states.reshape(S, K, B, R, F))):
            out[f"{tag}.{name}"] = v.numpy().astype(np.float32)
    path = os.path.join(GOLD, "time_compose_parallel.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
