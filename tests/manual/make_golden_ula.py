"""TEST INFRASTRUCTURE ONLY.  Golden vectors for the Langevin (ULA) phase of GaussianDiffusion1D.sample_compose_multibodies
(model/diffusion_1d.py:1986-2073: sample_step_ULA on gradient()'s composed score above t = 400, then p_sample), captured from the
reference on the CPU with synthetic generator-defined weights; needs the reference tree (oracle/ref_import.py).
    python tests/manual/make_golden_ula.py        # a few minutes
Writes tests/golden/ula_1d.npz and tests/golden/PINNING_REPORT_ULA.json.

Inputs and noise tapes are regenerated from seeds (tests/test_ula_host.py: step_inputs, grad_input, chain_inputs); the fixture holds
the reference's outputs: step.<tag>.out (sample_step_ULA, L = 3), grad.out (gradient(x, t, 4, scalar) at t > 400), and of one
sample_compose_multibodies(cond, N = 404, L = 2, 4) run chain.post (the whole state after the Langevin phase), chain.ckpt_t /
chain.ckpt (x[:, cs:] after the DDPM steps listed) and chain.final.  The reference's randn / randn_like draws are replaced by the
tapes, its plotting calls by a stub.  The report records the restatement of tests/test_ula_host.py against every item."""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import ref_import                 # noqa: E402
from make_golden import build_ref_unet, loop_draws, patched_randn          # noqa: E402
import test_ula_host as U         # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")


class _NoPlot:
    """Stands in for matplotlib.pyplot inside the reference module: every call is accepted and does nothing."""

    def __getattr__(self, name):
        return lambda *a, **k: None


def main():
    torch.set_num_threads(8)
    d1, _ = ref_import.import_reference()
    d1.plt = _NoPlot()
    t0 = time.time()
    m8, _, _ = build_ref_unet(d1, U.HZ, 8)
    m4, _, _ = build_ref_unet(d1, U.HZ, 4)
    g4 = d1.GaussianDiffusion1D(m8, image_size=U.R, conditioned_steps=U.LC, timesteps=1000, sampling_timesteps=1000, loss_type="l1")
    g4.model_unconditioned = m4
    od = U.oracle_diffusion()
    report, out = {}, {}

    # (a) sample_step_ULA at two timesteps
    for tag, (N, t, L, B, _) in U.STEP_CASES.items():
        x, nz = U.step_inputs(tag)
        b = d1.linear_beta_schedule(N)
        assert torch.equal(b, U.linear_beta_schedule(N))
        g4.betas_inference = b
        scalar = torch.sqrt(1 / (1 - torch.cumprod(1. - b, dim=0)))
        with patched_randn([nz[l] for l in range(L)]) as tp:
            ref = g4.sample_step_ULA(x.clone(), torch.tensor([t] * B), L, 4, N, scalar)
            assert tp.i == L
        mine = U.restated_step_ula(od, x, t, L, b, U.scalar_for_gradient(b), nz)
        report["step." + tag] = U.relerr(mine, ref)
        out[f"step.{tag}.out"] = ref.numpy().astype(np.float32)
        print("step", tag, report["step." + tag], round(time.time() - t0, 1), flush=True)

    # (b) gradient() above t = 400
    N, t, B, _ = U.GRAD_CASE
    b = d1.linear_beta_schedule(N)
    scalar = torch.sqrt(1 / (1 - torch.cumprod(1. - b, dim=0)))
    x = U.grad_input()
    ref = g4.gradient(x.clone(), t, 4, scalar)
    report["grad"] = U.relerr(U.restated_gradient(od, x, t, U.scalar_for_gradient(b)), ref)
    out["grad.out"] = ref.numpy().astype(np.float32)

    # (c) the two-phase chain
    N, L, B = U.CHAIN["N"], U.CHAIN["L"], U.CHAIN["B"]
    cond, tape, ula = U.chain_inputs()
    b = d1.linear_beta_schedule(N)
    g4.betas_inference = b
    draws = [tape.init] + [ula[j, l] for j in range(N - 401) for l in range(L)] + loop_draws(tape, 401)[1:]
    rec = {}
    p_sample = g4.p_sample

    def recording_p_sample(x, c, i, *a, **k):
        if i == 400:
            rec["post"] = torch.cat([c, x], dim=1).clone()
        res = p_sample(x, c, i, *a, **k)
        if i in U.CHAIN["ckpt"]:
            rec[i] = res[0].clone()
        return res

    g4.p_sample = recording_p_sample
    with patched_randn(draws) as tp:
        ref = g4.sample_compose_multibodies(cond.clone(), N, L, 4)
        assert tp.i == len(draws), (tp.i, len(draws))
    g4.p_sample = p_sample
    mine_rec = {}
    mine = U.restated_sample(od, cond, N, L, b, tape, ula, record=lambda k, v: mine_rec.__setitem__(k, v.clone()))
    report["chain.post"] = U.relerr(mine_rec["post"], rec["post"])
    for i in U.CHAIN["ckpt"]:
        report[f"chain.t{i}"] = U.relerr(mine_rec[i], rec[i])
    report["chain.final"] = U.relerr(mine, ref)
    assert torch.equal(ref, rec[0])
    out["chain.post"] = rec["post"].numpy().astype(np.float32)
    out["chain.ckpt_t"] = np.array(U.CHAIN["ckpt"], dtype=np.int32)
    out["chain.ckpt"] = np.stack([rec[i].numpy().astype(np.float32) for i in U.CHAIN["ckpt"]])
    out["chain.final"] = ref.numpy().astype(np.float32)
    print("chain", {k: v for k, v in report.items() if k.startswith("chain")}, round(time.time() - t0, 1), flush=True)

    np.savez_compressed(os.path.join(GOLD, "ula_1d.npz"), **out)
    report["seconds"] = time.time() - t0
    report["torch"] = torch.__version__
    with open(os.path.join(GOLD, "PINNING_REPORT_ULA.json"), "w") as f:
        json.dump(report, f, indent=1)
    print(json.dumps(report, indent=1))
    bad = {k: v for k, v in report.items() if isinstance(v, float) and k != "seconds" and v != 0.0}
    assert not bad, bad


if __name__ == "__main__":
    main()
