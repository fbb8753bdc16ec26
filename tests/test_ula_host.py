"""The Langevin (ULA) phase of sample_compose_multibodies, host side (no GPU): the three per-timestep tables against the
reference's formulas bit for bit, a CPU restatement of sample_step_ULA / the two-phase sampler on cindm_oracle pinned against the
reference's own output (tests/golden/ula_1d.npz, tests/manual/make_golden_ula.py), every refusal with its reason, the untouched
N <= 401 path, and the new C entry's export.

Weights and noise tapes are regenerated from seeds (the helpers below are shared with the golden generator and the GPU tests);
the fixture holds inputs and the reference's outputs only."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import cindm_amd
import cindm_oracle as O
from cindm_amd import _ffi
from cindm_amd.schedule import ula_schedule

HZ, LC, R, F = 24, 4, 20, 16                    # horizon = LC + R, four bodies
# sample_step_ULA cases: tag -> (N of linear_beta_schedule(N), timestep, L, B, seed)
STEP_CASES = {"n1000_t999": (1000, 999, 3, 2, 5201), "n404_t402": (404, 402, 3, 2, 5202)}
GRAD_CASE = (1000, 650, 2, 5203)                # (N, t, B, seed): gradient(x, t, 4, scalar) at one t > 400
CHAIN = dict(N=404, L=2, B=2, seed=5204, ckpt=(398, 300, 200, 100, 0))


def linear_beta_schedule(N):
    """model/diffusion_1d.py:464-468 (what the composition script passes as betas_inference)."""
    return O.linear_beta_schedule(N)


def step_inputs(tag):
    N, t, L, B, seed = STEP_CASES[tag]
    g = torch.Generator().manual_seed(seed)
    return torch.randn((B, HZ, F), generator=g), torch.randn((L, B, HZ, F), generator=g)


def grad_input():
    N, t, B, seed = GRAD_CASE
    return torch.randn((B, HZ, F), generator=torch.Generator().manual_seed(seed))


def chain_inputs():
    """(cond [B, LC, F], NoiseTape(init, step [401, ...]), ula [N - 401, L, B, HZ, F] first timestep first)."""
    N, L, B, seed = CHAIN["N"], CHAIN["L"], CHAIN["B"], CHAIN["seed"]
    g = torch.Generator().manual_seed(seed)
    cond = torch.rand((B, LC, F), generator=g)
    ula = torch.randn((N - 401, L, B, HZ, F), generator=g)
    return cond, O.NoiseTape.make(seed + 1, (B, R, F), 401), ula


def oracle_diffusion():
    sd8 = O.synth_state_dict(O.unet1d_param_shapes(HZ, 8), seed=0)
    sd4 = O.synth_state_dict(O.unet1d_param_shapes(HZ, 4), seed=1)
    return O.Diffusion1D(sd8, image_size=R, conditioned_steps=LC, sd_uncond=sd4)


# ------------------------------------------------------------------ the restatement (model/diffusion_1d.py:1986-2073 on cindm_oracle)
def scalar_for_gradient(betas_inference):
    return torch.sqrt(1 / (1 - torch.cumprod(1. - betas_inference, dim=0)))          # :1998-1999


def restated_gradient(od, x, t, scalar):
    eps = O.gradient_4body(od, x, t)
    return -1 * scalar[t] * eps if t > 400 else eps                                   # :1923-1926


def restated_step_ula(od, x, t, L, betas_inference, scalar, noise):
    step_sizes = betas_inference * 0.035                                              # :2050
    for l in range(L):
        ss = step_sizes[t]
        std = (2 * ss) ** .5
        grad = restated_gradient(od, x, t, scalar)
        x = x + grad * ss + noise[l] * std                                            # :2056-2059
    return x


def restated_sample(od, cond, N, L, betas_inference, tape, ula, t_stop=0, record=None):
    cs = od.conditioned_steps
    x = torch.cat([cond, tape.init], dim=1)
    scalar = scalar_for_gradient(betas_inference)
    for j, i in enumerate(range(N - 1, 400, -1)):
        if i < t_stop:
            return x
        x = restated_step_ula(od, x, i, L, betas_inference, scalar, ula[j])
    if record is not None:
        record("post", x)
    for i in reversed(range(t_stop, min(N, 401))):
        new, _ = O.p_sample(od, x[:, cs:], x[:, :cs], i, tape.step[i])
        x = torch.cat([x[:, :cs], new], dim=1)
        if record is not None:
            record(i, x[:, cs:])
    return x[:, cs:]


def relerr(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp(min=1e-30))


# ------------------------------------------------------------------ tables
@pytest.mark.parametrize("N", [404, 1000])
def test_tables_bit_for_bit(N):
    b = linear_beta_schedule(N)
    assert b.dtype == torch.float64
    sc, ss, sd = ula_schedule(b)
    assert sc.dtype == ss.dtype == sd.dtype == torch.float32 and len(sc) == len(ss) == len(sd) == N
    abar = torch.cumprod(1 - b, dim=0)
    want_sc = torch.sqrt(1 / (1 - abar))
    for i in range(N):
        s_i = b[i] * 0.035
        assert ss[i] == s_i.to(torch.float32), i
        assert sd[i] == ((2 * s_i) ** .5).to(torch.float32), i
        assert sc[i] == want_sc[i].to(torch.float32), i
    # what multiplies the U-Net's error in one Langevin update: ss * scalar < 1e-2 above t = 400 (beta <= 0.05, scalar <= 1.2)
    assert float((ss * sc)[401:].max()) < 1e-2
    assert float(b.max()) <= 0.05 and float(sc[401:].max()) <= 1.2


# ------------------------------------------------------------------ restatement against the reference's golden
def test_restatement_reproduces_reference_golden(gold_dir):
    g = np.load(os.path.join(gold_dir, "ula_1d.npz"))
    od = oracle_diffusion()
    for tag, (N, t, L, B, _) in STEP_CASES.items():
        x, nz = step_inputs(tag)
        b = linear_beta_schedule(N)
        out = restated_step_ula(od, x, t, L, b, scalar_for_gradient(b), nz)
        ref = torch.from_numpy(g[f"step.{tag}.out"])
        assert float((out - ref).abs().max()) <= 2e-6 * float(ref.abs().max()), tag
        assert not torch.equal(out[:, :LC], x[:, :LC])                   # the conditioning rows move
    N, t, B, _ = GRAD_CASE
    b = linear_beta_schedule(N)
    out = restated_gradient(od, grad_input(), t, scalar_for_gradient(b))
    ref = torch.from_numpy(g["grad.out"])
    assert float((out - ref).abs().max()) <= 2e-6 * float(ref.abs().max())
    # the chain: the Langevin phase and the hand-over to the DDPM loop (its first steps run on the drifted rows)
    cond, tape, ula = chain_inputs()
    rec = {}
    restated_sample(od, cond, CHAIN["N"], CHAIN["L"], linear_beta_schedule(CHAIN["N"]), tape, ula, t_stop=398,
                    record=lambda k, v: rec.__setitem__(k, v.clone()))
    post = torch.from_numpy(g["chain.post"])
    assert float((rec["post"] - post).abs().max()) <= 2e-6 * float(post.abs().max())
    assert float((post[:, :LC] - cond).abs().max()) > 1e-3                # drifted
    ck = torch.from_numpy(g["chain.ckpt"])[list(g["chain.ckpt_t"]).index(398)]
    assert float((rec[398] - ck).abs().max()) <= 2e-6 * float(ck.abs().max())


def test_pinning_report_is_exact(gold_dir):
    import json
    rep = json.load(open(os.path.join(gold_dir, "PINNING_REPORT_ULA.json")))
    items = {k: v for k, v in rep.items() if k not in ("seconds", "torch")}
    assert len(items) >= 4 + len(CHAIN["ckpt"])
    assert all(v == 0.0 for v in items.values()), items


# ------------------------------------------------------------------ refusals
def _diffusion(betas_inference=None, uncond=True, timesteps=1000, **kw):
    m = cindm_amd.TemporalUnet1D(HZ, 8, False, attention=True)
    d = cindm_amd.GaussianDiffusion1D(m, image_size=R, conditioned_steps=LC, timesteps=timesteps, loss_type="l1",
                                      betas_inference=betas_inference, **kw)
    if uncond:
        d.model_unconditioned = cindm_amd.TemporalUnet1D(HZ, 4, False, attention=True)
    return d


def test_refusals_carry_the_reason():
    cond = torch.zeros((2, LC, F))
    d = _diffusion(linear_beta_schedule(1000))
    with pytest.raises(NotImplementedError, match=r"gradient\(x, t, 4\)"):
        d.sample_compose_multibodies(cond, 1000, 2, 3)
    with pytest.raises(ValueError, match="L .* must be >= 0"):
        d.sample_compose_multibodies(cond, 1000, -1, 4)
    with pytest.raises(ValueError, match="num_timesteps = 1000"):
        d.sample_compose_multibodies(cond, 1001, 2, 4)
    with pytest.raises(ValueError, match="betas_inference .*None"):
        _diffusion(None).sample_compose_multibodies(cond, 1000, 2, 4)
    with pytest.raises(ValueError, match="400 entries, shorter than N = 1000"):
        _diffusion(linear_beta_schedule(400)).sample_compose_multibodies(cond, 1000, 2, 4)
    with pytest.raises(NotImplementedError, match="model_unconditioned"):
        _diffusion(linear_beta_schedule(1000), uncond=False).sample_compose_multibodies(cond, 1000, 2, 4)
    with pytest.raises(NotImplementedError, match="pred_x0"):
        _diffusion(linear_beta_schedule(1000), objective="pred_x0").sample_compose_multibodies(cond, 1000, 2, 4)
    # every argument is fine: what is left is the missing device
    with pytest.raises(cindm_amd.CindmError, match="no CPU execution path"):
        d.sample_compose_multibodies(cond, 1000, 2, 4, seed=0)
    b = linear_beta_schedule(1000)
    with pytest.raises(cindm_amd.CindmError, match="no CPU execution path"):
        d.sample_step_ULA(torch.zeros((2, HZ, F)), torch.tensor([999, 999]), 3, 4, 1000, scalar_for_gradient(b), seed=0)
    with pytest.raises(NotImplementedError, match=r"gradient\(x, t, 4\)"):
        d.sample_step_ULA(torch.zeros((2, HZ, 12)), torch.tensor([999, 999]), 3, 3, 1000, scalar_for_gradient(b))
    with pytest.raises(ValueError, match="scalar_for_gradient must cover"):
        d.sample_step_ULA(torch.zeros((2, HZ, F)), torch.tensor([999, 999]), 3, 4, 1000, scalar_for_gradient(b)[:500])
    # gradient(): t > 400 without the scalar fails as in the reference; with it the refusal is gone (the CPU tensor is what is left)
    with pytest.raises(NotImplementedError, match="scalar_for_gradient"):
        d.gradient(torch.zeros((2, HZ, F)), 650, 4)
    with pytest.raises(cindm_amd.CindmError):
        d.gradient(torch.zeros((2, HZ, F)), 650, 4, scalar_for_gradient(b))


def test_n_le_401_takes_the_old_path(monkeypatch):
    """N <= 401: no Langevin phase, no new refusal -- L, n_bodies and betas_inference are not looked at, the chain starts at N - 1 on
    the caller's cond."""
    d = _diffusion(None)
    seen = {}

    def fake_run_loop(img, cond, desc, t_start, t_end, **kw):
        seen.update(t_start=t_start, t_end=t_end, cond=cond, shape=tuple(img.shape))
        return img

    monkeypatch.setattr(d, "_run_loop", fake_run_loop)
    monkeypatch.setattr(d, "_run_ula", lambda *a, **k: pytest.fail("Langevin phase entered for N <= 401"))
    monkeypatch.setattr(d, "_init_state", lambda shape, *a, **k: torch.zeros(shape))

    class Dev(torch.Tensor):                       # a CPU tensor that claims to be on the device: the host logic is what is tested
        is_cuda = True

    cond = torch.zeros((2, LC, F)).as_subclass(Dev)
    for N in (401, 400, 12):
        out = d.sample_compose_multibodies(cond, N, -5, 7, seed=1, t_stop=3)
        assert seen["t_start"] == N - 1 and seen["t_end"] == 3 and seen["cond"] is cond and seen["shape"] == (2, R, F)
        assert tuple(out.shape) == (2, R, F)


def test_noise_tape_carries_ula():
    t = cindm_amd.NoiseTape(torch.zeros(1), torch.zeros(1))
    assert t.ula is None and t.to("cpu").ula is None
    t = cindm_amd.NoiseTape(torch.zeros(1), torch.zeros(1), ula=torch.ones((1, 2), dtype=torch.float64))
    assert t.to("cpu").ula.dtype == torch.float32 and t.to("cpu").recur is None


def test_symbol_exported_and_bound():
    assert "cindm_ddpm1d_sample_ula" in _ffi.SIGNATURES
    L = _ffi.lib()
    fn = L.cindm_ddpm1d_sample_ula
    assert fn.restype is C.c_int and len(fn.argtypes) == 21
    assert L.cindm_abi_version() == 4
    # argument checks come before any device work: a null handle is refused with the reason
    assert fn(None, None, None, None, None, 1, 0, 1, None, None, None, None, 0, None, 0, 0, 1, None, 0, None, 0) != 0
    assert b"null argument" in L.cindm_last_error()
