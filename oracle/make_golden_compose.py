"""TEST INFRASTRUCTURE ONLY.  Golden vectors of the composition alone -- from the pair model's outputs to (model_mean, x_start,
pred_noise) -- at descriptors no earlier fixture reaches; runs ONLY in the build container (imports the reference through
oracle/ref_import.py, like oracle/make_golden.py).  The descriptors are ``compose_cases.GOLDEN`` (tests/compose_cases.py):

  * sum-inside, 3 bodies, 3 windows, stride 16      (model/diffusion_1d.py:997-999: the divisor mask.mean(0), an odd pair count)
  * noise_sum, 4 bodies, 2 windows, stride 10       (:1453-1463)
  * outside mean, 3 bodies, 2 abutting windows      (:1447-1452)
  * mean-inside, 2 windows, conditioned_steps = 4   (:956-957, :1028-1030: windows on cat(cond, x), outputs on x)
  * outside mean, 2 windows, conditioned_steps = 4  -- THE REFERENCE RAISES: p_sample_compose_outside hands the whole ``cond`` to
    p_mean_variance of every 24-row window (:1428-1430), model_predictions prepends it (:957) and the pair model is given 28 rows, which
    its skip connections cannot join (with more than two bodies torch.cat already fails on the feature width).  The message is
    recorded under "<name>.raises"; what the library does there (it refuses the descriptor) is the project's own definition.

Per descriptor, at batch 2, t = 500, pred_noise, clip on: ``x``, ``cond``, ``t``, the rows the pair model was called on and what it
returned, per (window, pair) in call order (``pair_in`` [W * P * B, 24, 8] as ``f64_reference.compose_rows`` orders them, ``pair_eps``
[W, P, B, 24, 8]), and the reference's ``mean``, ``x_start`` and -- inside modes -- ``pred_noise``.  The outside modes go through
p_sample_compose_outside with a zero noise draw, which returns (model_mean, x_start) and no pred_noise.  Every item asserts
oracle == reference (the pin).  The archive is written with fixed member dates: a second run gives the same bytes.

    python oracle/make_golden_compose.py          # seconds
"""
import io
import os
import sys
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tests"))
import cindm_oracle as O                                    # noqa: E402
import f64_reference as R                                   # noqa: E402
import ref_import                                           # noqa: E402
import compose_cases as C                                   # noqa: E402
from make_golden import GOLD, build_ref_unet, patched_randn, relerr      # noqa: E402


def save_npz(path, arrays):
    """np.savez_compressed with every member dated 1980-01-01: the same arrays give the same file."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    d1, _ = ref_import.import_reference()
    m8, sd8, _ = build_ref_unet(d1, 24, 8)
    calls = []
    m8.register_forward_hook(lambda mod, args, out: calls.append((args[0].detach().clone(), out.detach().clone())))
    out, report = {}, {}
    t, B = C.GOLDEN_T, C.GOLDEN_B
    for name, d in C.GOLDEN.items():
        mode, nb, W, cs, k = d
        desc = R.ComposeCase(mode, nb, W, cs, C.WINDOW, k)
        gd = d1.GaussianDiffusion1D(m8, image_size=C.WINDOW, conditioned_steps=k, timesteps=1000, sampling_timesteps=1000, loss_type="l1")
        od = O.Diffusion1D(sd8, image_size=C.WINDOW, conditioned_steps=k)
        x, cond = C.make_state(d, t, B)
        kw = dict(compose_mode=mode, n_composed=W - 1, compose_start_step=cs, single_model_step=C.WINDOW, compose_n_bodies=nb)
        del calls[:]
        try:
            with torch.no_grad():
                if mode in C.OUTSIDE:
                    with patched_randn([torch.zeros_like(x)]):
                        mean, x0 = gd.p_sample_compose_outside(x.clone(), cond, t, **kw)
                    eps = None
                    o_mean, _, o_x0 = O._outside_aggregate(od, x.clone(), cond, t, clip_denoised=True, **kw)
                else:
                    mean, _, _, x0, eps = gd.p_mean_variance(x.clone(), cond, torch.full((B,), t, dtype=torch.long), clip_denoised=True, **kw)
                    o_mean, _, o_x0, _ = O.p_mean_variance(od, x.clone(), cond, t, True, **kw)
        except RuntimeError as e:
            out[name + ".raises"] = np.array(f"{type(e).__name__}: {e}".splitlines()[0])
            print(name, "raises:", out[name + ".raises"], flush=True)
            continue
        report[name] = max(relerr(o_mean, mean), relerr(o_x0, x0))
        P = nb * (nb - 1) // 2
        assert len(calls) == W * P, (name, len(calls))
        out[name + ".x"], out[name + ".t"] = x.numpy(), np.array(t)
        if cond is not None:
            out[name + ".cond"] = cond.numpy()
        out[name + ".pair_in"] = torch.cat([c[0] for c in calls], dim=0).numpy()
        out[name + ".pair_eps"] = torch.stack([c[1] for c in calls]).view(W, P, B, C.WINDOW, 8).numpy()
        assert torch.equal(torch.from_numpy(out[name + ".pair_in"]), R.compose_rows(desc, x, cond)[0]), name
        out[name + ".mean"], out[name + ".x_start"] = mean.numpy(), x0.numpy()
        if eps is not None:
            out[name + ".pred_noise"] = eps.numpy()
        print(name, "oracle vs reference", report[name], flush=True)
    save_npz(os.path.join(GOLD, "compose_grid.npz"), out)
    bad = {k: v for k, v in report.items() if v > 2e-6}
    assert not bad, bad
    assert [k for k in out if k.endswith(".raises")] == ["mean-nb2-w2-cs10-cond4.raises"]


if __name__ == "__main__":
    main()
