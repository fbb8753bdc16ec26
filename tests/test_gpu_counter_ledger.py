"""GPU (MI355X): the counter-based generator against its host model, and the draw ledger on the chains.

Three questions, none of which a moment test or a seeded-against-seeded comparison answers:

  a / b.  Does ``cindm_fill_normal`` / ``cindm_fill_noise2d`` write, on EVERY element, the normal the host model
          (oracle/counter_noise.py: Philox4x32-10 in integers, the kernel's fp32 uniforms, Box-Muller in float64) computes for the
          same (seed, sample, word, element)?  The device's logf / sqrtf / sincosf are not correctly rounded, so the comparison is
          absolute with a measured bound (FILL_MEASURED / FILL_BOUND below); a wrong key, round count, multiplier, truncated
          sample index or dropped seed word changes almost every element by O(1).
  c.      Does every sampling chain draw each of its streams under the key the ledger (counter_noise.STREAMS) states?
          The seeded run (``seed=``, ``sample_offset=``) must equal, bit for bit, the run of the same entry on a tape
          (``noise=``) whose every field was drawn by the two fill entries under the ledger's keys -- the device's own bits, so no
          tolerance: both runs go through the same update kernel and the library is built with -ffp-contract=off.
  d.      Does a seeded chain, as the benchmark times it, agree with the reference on its own draws?  The ledger tape goes to
          the host, the oracle runs on it, and the SEEDED result is held to the chain tolerance.

Shapes: horizon 24, F = 8 (4 and 16 on the DDIM entry), B = 3 or 5 with sample_offset = 2, five DDPM steps (t_stop = T - 5) or
S = 4 DDIM steps with eta = 0.5 (three of which draw; the last pair returns x_start).  2-D: 32 x 32, 2 designs x 2 boundaries, a
DDPM diffusion of 4 timesteps (its whole chain; a 1000-row tape of 2-D states would be 150 MB) and the first 3 DDIM steps of
S = 250; the guided 2-D chains run at 64 x 64, the only size the four-level ForceUnet of the fixture is built for."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import cindm_amd
import cindm_oracle as O
import counter_noise as N
from cindm_amd import _ffi
from cindm_amd.unet2d import from_device_layout
from test_gpu_known_1d import region
from test_gpu_parity import TOL_CHAIN, build_unet, rel
from test_gpu_parity_2d import build_unet2d

pytestmark = pytest.mark.gpu

HZ, T = 24, 1000
SEED, OFF = (0x5eed << 40) + 17, 2          # both key words non-zero; a batch that does not start at sample 0

# Largest |device - model| over every element of every case of test_fill_normal_equals_host_model and
# test_fill_noise2d_equals_host_model, measured on one MI355X: 3.546e-7 (at z = -2.39, seed 2^63 + 12345, offset 2^32 - 2, word 0:
# one and a half fp32 ulps of the result); 2^20 further draws reached 5.7e-7 at |z| = 4.0, inside the 8 x margin.
FILL_MEASURED = 3.55e-7
FILL_BOUND = 8 * FILL_MEASURED
assert FILL_BOUND <= 1e-4


def _say(name, v):
    print(f"[counter-ledger] {name}: {v:.3e}")
    return v


def _i32(word):
    """A 32-bit generator word as the int32 the C entries take (they cast it back to uint32)."""
    word &= N.M32
    return word - (1 << 32) if word >= (1 << 31) else word


# ------------------------------------------------------------------ the two fill entries
def dev_fill(device, B, per, seed, off, word):
    out = torch.empty((B, per), dtype=torch.float32, device=device)
    with torch.cuda.device(device):
        _ffi.check(_ffi.lib().cindm_fill_normal(_ffi.ptr(out), B, per, C.c_uint64(seed & N.M64), off, _i32(word),
                                                _ffi.current_stream(device)))
    return out


def dev_fill2d(device, B, nb, HW, Cc, cp, seed, off, word):
    out = torch.full((B * nb, HW, cp), float("nan"), dtype=torch.float32, device=device)
    with torch.cuda.device(device):
        _ffi.check(_ffi.lib().cindm_fill_noise2d(_ffi.ptr(out), B, nb, HW, Cc, cp, C.c_uint64(seed & N.M64), off, _i32(word),
                                                 _ffi.current_stream(device)))
    return out


FILL_SHAPES = [(3, 192), (5, 50)]                                    # per = 50: not a multiple of 4
FILL_SEEDS = [5, (1 << 63) + 12345, 1 << 32]                         # high key word set; low key word zero
FILL_OFFSETS = [0, 7, (1 << 32) - 2]                                 # the batch crosses the carry into the fourth counter word
FILL_WORDS = [0, 999, 1000, 0x10000 + 17, 0x80000000 + 65536 + 402]


@pytest.mark.parametrize("B,per", FILL_SHAPES)
def test_fill_normal_equals_host_model(device, B, per):
    """cindm_fill_normal against the float64 host model on every element of 45 (seed, offset, word) cases per shape.
    Measured on the MI355X: largest |device - model| = 3.55e-7 at (3, 192) and 3.43e-7 at (5, 50) (one and a half fp32 ulps of a
    |z| in [2, 4)); bound 8 x the larger = 2.84e-6 (<= 1e-4).  A wrong key moves almost every draw by O(1) (asserted on the model)."""
    worst = 0.0
    for seed in FILL_SEEDS:
        for off in FILL_OFFSETS:
            for word in FILL_WORDS:
                got = dev_fill(device, B, per, seed, off, word).cpu().double().numpy()
                want = N.fill_normal(B, per, seed, off, word)
                assert np.isfinite(got).all() and float(np.abs(got).max()) <= N.Z_MAX + FILL_BOUND
                err = float(np.abs(got - want).max())
                worst = max(worst, err)
                assert err <= FILL_BOUND, (hex(seed), off, hex(word), err)
    _say(f"fill_normal B={B} per={per}: max |device - model|", worst)
    # what a wrong key would look like: each single change of the key moves the draws by O(1), far above the bound
    seed, off, word = FILL_SEEDS[1], FILL_OFFSETS[2], FILL_WORDS[4]
    base = N.fill_normal(B, per, seed, off, word)
    assert float(np.abs(N.fill_normal(B, per, seed & N.M32, off, word) - base).max()) > 1.0          # a dropped high seed word
    assert float(np.abs(N.fill_normal(B, per, seed, off, word + 1) - base).max()) > 1.0              # another step word
    # a sample index truncated to 32 bits: samples 2^32, 2^32 + 1, ... (rows 2 .. of this batch) would repeat samples 0, 1, ...
    assert float(np.abs(N.fill_normal(B - 2, per, seed, 0, word) - base[2:]).max()) > 1.0


def test_fill_noise2d_equals_host_model(device):
    """cindm_fill_noise2d (2 designs x 3 boundaries, 4 x 4 pixels, 21 channels in 24 padded) against the host model on every
    element, padding lanes included.  Measured on the MI355X: largest |device - model| = 2.60e-7; the bound is FILL_BOUND = 2.84e-6,
    8 x the larger figure of the two fill tests.  State channels are shared over a design's boundary copies, boundary channels are per
    image under the xor'd seed, padding lanes hold 0 (fill_noise2d_kernel: ``v[j] = (c >= C) ? 0.f : ...``), and the batch of 2
    at sample_offset = 1 is designs 1 and 2 of the batch of 3 at offset 0."""
    B, nb, HW, Cc, cp = 2, 3, 16, 21, 24
    worst = 0.0
    for seed, off, word in ((5, 0, 1000), ((1 << 63) + 12345, 7, 999), (1 << 32, (1 << 32) - 2, 3)):
        got = dev_fill2d(device, B, nb, HW, Cc, cp, seed, off, word).cpu().double().numpy()
        want = N.fill_noise2d(B, nb, HW, Cc, cp, seed, off, word)
        assert np.isfinite(got).all()
        err = float(np.abs(got - want).max())
        worst = max(worst, err)
        assert err <= FILL_BOUND, (hex(seed), off, word, err)
        g = got.reshape(B, nb, HW, cp)
        assert all(np.array_equal(g[:, 0, :, :Cc - 3], g[:, k, :, :Cc - 3]) for k in range(1, nb))
        assert not np.array_equal(g[0, :, :, :Cc - 3], g[1, :, :, :Cc - 3])
        assert all(not np.array_equal(g[:, 0, :, Cc - 3:Cc], g[:, k, :, Cc - 3:Cc]) for k in range(1, nb))
        assert bool((g[..., Cc:] == 0).all())
        # the boundary channels written out once more from the scalar model: keyed by the image, under the xor'd seed
        b, k, pix, c = 1, 2, 5, 19
        z = float(N.counter_normal(seed ^ N.BOUND2D_XOR, (off + b) * nb + k, word, pix * cp + c))
        assert abs(g[b, k, pix, c] - z) <= FILL_BOUND
    _say("fill_noise2d: max |device - model|", worst)
    three = dev_fill2d(device, 3, nb, HW, Cc, cp, 5, 0, 1000)
    assert torch.equal(dev_fill2d(device, 2, nb, HW, Cc, cp, 5, 1, 1000), three[nb:])


# ------------------------------------------------------------------ ledger tapes: every field from the device's own generator
def draw(device, stream, shape, seed, off, t=0, r=0, l=0, Tn=T):
    """One draw of a ledger stream over ``shape`` [B, rows, F], by cindm_fill_normal under the ledger's key."""
    s = N.STREAM[stream]
    return dev_fill(device, shape[0], math.prod(shape[1:]), s["seed_word"](seed), off, s["step_word"](t, r, l, Tn)).view(shape)


def ddpm_rows(ts):
    """(tape row, timestep, level reached) of DDPM steps: rows are indexed by t."""
    return [(t, t, t - 1) for t in ts]


def ddim_rows(d):
    """... of every DDIM step of d's schedule: rows are indexed by the step; the last pair (t_next = -1) draws nothing."""
    times, _ = d.ddim_schedule()
    return [(i, t, tn) for i, (t, tn) in enumerate(zip(times[:-1], times[1:]))]


def ledger_tape(device, shape, rows, n_rows, *, seed=SEED, off=OFF, relax=0, cond_rows=0, known=False, ddim=False):
    """The NoiseTape of a 1-D chain over the state ``shape`` with every field drawn under the ledger's keys.  ``rows`` as
    ddpm_rows / ddim_rows; ``relax``: relaxation records per row (the guidance's N); ``cond_rows``: inpainting rows."""
    B, L, F = shape
    z = lambda *s: torch.zeros(s, dtype=torch.float32, device=device)
    dr = lambda stream, shp=shape, **k: draw(device, stream, shp, seed, off, **k)
    step = z(n_rows, *shape)
    recur = z(n_rows, relax, *shape) if relax else None
    cond = z(n_rows, B, cond_rows, F) if cond_rows else None
    kw = {}
    if known:
        kw = dict(known_init=dr("known-1d-init"), known_step=z(n_rows, *shape), known_recur=z(n_rows, relax, *shape) if relax else None)
    for row, t, level in rows:
        if (t > 0 and not ddim) or (ddim and level >= 0):
            step[row] = dr("step", t=t)
        if cond is not None:
            cond[row] = dr("inpainting", (B, cond_rows, F), t=t)
        for r in range(relax):
            recur[row][r] = dr("relaxation", t=t, r=r)
            if known:
                kw["known_recur"][row][r] = dr("known-1d-relaxation", t=t, r=r)
        if known and level >= 0:
            kw["known_step"][row] = dr("known-1d-step", t=level)
    return cindm_amd.NoiseTape(dr("x_T"), step, recur, cond, **kw)


def same(run, tape, **seeded):
    """The seeded run and the tape run of one entry, bit for bit.  Returns the seeded result."""
    a = run(seed=SEED, sample_offset=OFF, **seeded)
    b = run(noise=tape)
    assert bool(torch.isfinite(a).all()) and float(a.abs().max()) > 0
    assert torch.equal(a, b), f"seeded and ledger-tape runs differ: max |a - b| = {float((a - b).abs().max()):.3e}"
    return a


@pytest.fixture(scope="module")
def unet8(device):
    return build_unet(device)


@pytest.fixture(scope="module")
def unet4(device):
    return build_unet(device, F=4)


def _ddpm(device, m, **kw):
    return cindm_amd.GaussianDiffusion1D(m, image_size=HZ, conditioned_steps=0, timesteps=T, sampling_timesteps=T, loss_type="l1", **kw).to(device)


def _ddim(device, m, S=4, eta=0.5, **kw):
    kw.setdefault("image_size", HZ)
    kw.setdefault("conditioned_steps", 0)
    return cindm_amd.GaussianDiffusion1D(m, timesteps=T, sampling_timesteps=S, loss_type="l1", ddim_sampling_eta=eta, **kw).to(device)


TS = list(range(T - 1, T - 6, -1))          # the five DDPM steps of t_stop = T - 5


# ------------------------------------------------------------------ c. plain DDPM
@pytest.mark.parametrize("fuse,pingpong", [(1, 1), (0, 1), (1, 0), (0, 0)])
def test_plain_ddpm(device, unet8, fuse, pingpong):
    """x_T under (seed, T), the step draws under (seed, t): in ups_last_kernel's fused tail (element (n F + q4) >> 2 as a group of
    four) and in compose_update_kernel (element lx F + f), with the step state in two slots or advanced by the counter kernel."""
    m, _ = unet8
    d = _ddpm(device, m)
    shape = (3, HZ, 8)
    tape = ledger_tape(device, shape, ddpm_rows(TS), T)
    try:
        m.set_option("fuse_update", fuse); m.set_option("pingpong", pingpong)
        same(lambda **kw: d.sample(batch_size=3, n_composed=0, compose_n_bodies=2, t_stop=T - 5, **kw), tape)
        assert d.last_step_info()[1] is bool(fuse)
    finally:
        m.set_option("fuse_update", 1); m.set_option("pingpong", 1)


@pytest.mark.parametrize("objective", ["pred_x0", "pred_v"])
def test_plain_ddpm_other_objectives(device, unet8, objective):
    d = _ddpm(device, unet8[0], objective=objective)
    tape = ledger_tape(device, (5, HZ, 8), ddpm_rows(TS), T)
    same(lambda **kw: d.sample(batch_size=5, n_composed=0, compose_n_bodies=2, t_stop=T - 5, **kw), tape)


@pytest.mark.parametrize("F", [4, 8, 16])
def test_plain_ddim_state_widths(device, F):
    """The DDIM entry (words: the step's TIMESTEP, rows: its index) at the three state widths of the fused tail."""
    m, _ = build_unet(device, F=F, seed=7)
    d = _ddim(device, m)
    shape = (5, HZ, F)
    tape = ledger_tape(device, shape, ddim_rows(d), 4, ddim=True)
    same(lambda **kw: d.ddim_sample(shape, None, **kw), tape)
    assert d.last_step_info()[1] is True


# ------------------------------------------------------------------ c. three composed windows
@pytest.mark.parametrize("mode", ["mean-inside", "noise_sum"])
def test_composed_windows(device, unet8, mode):
    """n_composed = 2, compose_start_step = 16: the state has 56 rows and the element index runs over all of them, not over a window's 24."""
    d = _ddpm(device, unet8[0])
    shape = (3, HZ + 2 * 16, 8)
    tape = ledger_tape(device, shape, ddpm_rows(TS), T)
    out = same(lambda **kw: d.sample(batch_size=3, n_composed=2, compose_start_step=16, compose_mode=mode, t_stop=T - 5, **kw), tape)
    assert tuple(out.shape) == shape


# ------------------------------------------------------------------ c. inpainting rows
@pytest.mark.parametrize("ddim", [False, True], ids=["ddpm", "ddim"])
def test_inpainting_rows(device, unet8, ddim):
    """``cond`` with conditioned_steps == 0: rows 0 .. 3 are overwritten with q_sample(cond, t, z), z under seed ^ 0x5bd1e995 at
    word t, element lx F + f of the state row -- which is the element of the [B, 4, F] tape as well."""
    m, _ = unet8
    shape = (3, HZ, 8)
    cond = (torch.rand((3, 4, 8), generator=torch.Generator().manual_seed(61)) * 2 - 1).to(device)
    if ddim:
        d = _ddim(device, m)
        tape = ledger_tape(device, shape, ddim_rows(d), 4, cond_rows=4, ddim=True)
        run = lambda **kw: d.ddim_sample(shape, cond, **kw)
    else:
        d = _ddpm(device, m)
        tape = ledger_tape(device, shape, ddpm_rows(TS), T, cond_rows=4)
        run = lambda **kw: d.sample(batch_size=3, cond=cond, n_composed=0, t_stop=T - 5, **kw)
    out = same(run, tape)
    if not ddim:          # the chain ended on the overwrite at level T - 5: the rows are the ledger's draw, written out
        z = tape.cond[T - 5]
        assert torch.equal(out[:, :4], d.sqrt_alphas_cumprod[T - 5] * cond + d.sqrt_one_minus_alphas_cumprod[T - 5] * z)


# ------------------------------------------------------------------ c. sample_compose_multibodies
@pytest.fixture(scope="module")
def models_mb(device, unet8, unet4):
    return unet8[0], unet4[0]


def _mb(device, models, N_inf=None):
    kw = {} if N_inf is None else dict(betas_inference=O.linear_beta_schedule(N_inf))
    d = cindm_amd.GaussianDiffusion1D(models[0], image_size=20, conditioned_steps=4, timesteps=T, sampling_timesteps=T, loss_type="l1", **kw).to(device)
    d.model_unconditioned = models[1]
    return d


def test_multibodies_ddpm_phase(device, models_mb):
    """N = 400, four bodies, three designs, four steps: x_T [B, 20, 16] under (seed, T = num_timesteps), steps under (seed, t)."""
    d = _mb(device, models_mb)
    cond = (torch.rand((3, 4, 16), generator=torch.Generator().manual_seed(62)) - 0.5).to(device)
    tape = ledger_tape(device, (3, 20, 16), ddpm_rows(range(399, 395, -1)), 400)
    same(lambda **kw: d.sample_compose_multibodies(cond, 400, 0, 4, t_stop=396, **kw), tape)


def test_multibodies_langevin_phase(device, models_mb):
    """N = 404, L = 2, t_stop = 402: the Langevin draws under (seed, 0x80000000 + 65536 l + t) over the WHOLE state (conditioning
    rows included: 24 rows, not 20), tape row N - 1 - t."""
    Nn, L = 404, 2
    d = _mb(device, models_mb, Nn)
    cond = (torch.rand((3, 4, 16), generator=torch.Generator().manual_seed(63)) - 0.5).to(device)
    full = (3, 24, 16)
    ula = torch.zeros((2, L) + full, dtype=torch.float32, device=device)
    for t in (403, 402):
        for l in range(L):
            ula[Nn - 1 - t][l] = draw(device, "langevin", full, SEED, OFF, t=t, l=l)
    tape = cindm_amd.NoiseTape(draw(device, "x_T", (3, 20, 16), SEED, OFF), None, ula=ula)
    out = same(lambda **kw: d.sample_compose_multibodies(cond, Nn, L, 4, t_stop=402, full_state=True, **kw), tape)
    assert tuple(out.shape) == full and not torch.equal(out[:, :4], cond)


# ------------------------------------------------------------------ c. guided chains (built-in point objective)
# ("-alpha" multiplies the gradient by betas[t] / sqrt(alphas_cumprod[t]) = 2.0e4 at t = 999 on the cosine schedule: with the coef = 2
# of the other guided tests, which run it from lower t or without relaxations, three relaxations at t = 999 .. 995 diverge to NaN in
# the CPU oracle as well.  coef = 2e-4 makes the shift of the order of the state there.)
GUIDED = [("standard-recurrence-2", dict(last_n_step=2, coef=2.0)),
          ("standard-alpha-recurrence-3", dict(last_n_step=3, coef=2e-4, design_fn_mode="L2square"))]


@pytest.mark.parametrize("guid,okw", GUIDED, ids=[g for g, _ in GUIDED])
@pytest.mark.parametrize("ddim", [False, True], ids=["ddpm", "ddim"])
def test_guided_chains(device, unet8, ddim, guid, okw):
    """Relaxation r of the step at t draws under (seed ^ 0x7f4a7c15, 0x10000 (r + 1) + t), the step itself under (seed, t): a
    relaxation that reused the step's draw, or the draw of another iteration, would pass every other test of the suite."""
    m, _ = unet8
    R = int(guid.split("-")[-1])
    obj = cindm_amd.PointObjective([0.25, -0.5], **okw)
    shape = (3, HZ, 8)
    kw0 = dict(n_composed=0, compose_mode="mean-inside", design_fn=obj, design_guidance=guid)
    if ddim:
        d = _ddim(device, m)
        tape = ledger_tape(device, shape, ddim_rows(d), 4, relax=R, ddim=True)
        run = lambda **kw: d.ddim_sample(shape, None, **kw0, **kw)
    else:
        d = _ddpm(device, m)
        tape = ledger_tape(device, shape, ddpm_rows(TS), T, relax=R)
        run = lambda **kw: d.sample(batch_size=3, t_stop=T - 5, **kw0, **kw)
    same(run, tape)


# ------------------------------------------------------------------ c. autoregressive rollout
def test_autoregressive_rollout(device, unet8):
    """Two segments, S = 3: segment k draws x_T and its steps under seed_k = seed + k 0x9E3779B97F4A7C15 (mod 2^64)."""
    d = _ddim(device, unet8[0], S=3, image_size=20, conditioned_steps=4)
    B, K, S, shape = 3, 2, 3, (3, 20, 8)
    cond = (torch.rand((B, 4, 8), generator=torch.Generator().manual_seed(64)) - 0.5).to(device)
    init = torch.zeros((K,) + shape, device=device)
    step = torch.zeros((K, S) + shape, device=device)
    for k in range(K):
        sk = N.segment_seed(SEED, k)
        init[k] = draw(device, "x_T", shape, sk, OFF)
        for i, t, tn in ddim_rows(d):
            if tn >= 0:
                step[k][i] = draw(device, "step", shape, sk, OFF, t=t)
    out = same(lambda **kw: d.autoregress_time_compose_sample(B, cond, K - 1, **kw), cindm_amd.NoiseTape(init, step))
    assert tuple(out.shape) == (B, K * 20, 8)


# ------------------------------------------------------------------ c. a known region
@pytest.mark.parametrize("chain", ["ddpm", "ddim", "ddim_guided"])
def test_known_region(device, unet8, chain):
    """known_init under (seed ^ 0x6b6e6f776e316421, T), known_step at the LEVEL the step reached (DDPM: t - 1, row t; DDIM:
    t_next, row i), known_recur under 0x10000 (r + 1) + t -- the region of tests/test_gpu_known_1d.py (whole, partial and
    per-design bodies)."""
    m, _ = unet8
    shape = (3, HZ, 8)
    k, msk = region(HZ, 8)
    rkw = dict(known=k.to(device), known_mask=msk.to(device))
    if chain == "ddpm":
        d = _ddpm(device, m)
        tape = ledger_tape(device, shape, ddpm_rows(TS), T, known=True)
        run = lambda **kw: d.sample(batch_size=3, n_composed=0, t_stop=T - 5, **rkw, **kw)
    else:
        d = _ddim(device, m)
        guided = chain == "ddim_guided"
        tape = ledger_tape(device, shape, ddim_rows(d), 4, known=True, relax=2 if guided else 0, ddim=True)
        gkw = dict(n_composed=0, compose_mode="mean-inside", design_guidance="standard-recurrence-2",
                   design_fn=cindm_amd.PointObjective([0.25, -0.5], last_n_step=2, coef=2.0)) if guided else {}
        run = lambda **kw: d.ddim_sample(shape, None, **gkw, **rkw, **kw)
    out = same(run, tape)
    if chain == "ddpm":          # the region ended at level T - 6 on the ledger's draw
        lvl = T - 6
        q = d.sqrt_alphas_cumprod[lvl] * rkw["known"] + d.sqrt_one_minus_alphas_cumprod[lvl] * tape.known_step[T - 5]
        assert torch.equal(out[rkw["known_mask"]], q[rkw["known_mask"]])
    else:
        assert torch.equal(out[rkw["known_mask"]], rkw["known"][rkw["known_mask"]])


# ------------------------------------------------------------------ d. one step across to the reference
def test_seeded_ddpm_agrees_with_the_oracle_on_its_own_draws(device, unet8):
    """The seeded plain DDPM chain (five steps) against O.sample on the ledger tape copied to the host."""
    m, sd = unet8
    d = _ddpm(device, m)
    shape = (3, HZ, 8)
    tape = ledger_tape(device, shape, ddpm_rows(TS), T)
    od = O.Diffusion1D(sd, image_size=HZ, conditioned_steps=0)
    ref = O.sample(od, 3, O.NoiseTape(tape.init.cpu(), tape.step.cpu()), n_composed=0, t_stop=T - 5)
    out = d.sample(batch_size=3, n_composed=0, compose_n_bodies=2, seed=SEED, sample_offset=OFF, t_stop=T - 5)
    assert _say("seeded DDPM vs oracle on the ledger tape", rel(out, ref)) < TOL_CHAIN


def test_seeded_guided_ddpm_agrees_with_the_oracle_on_its_own_draws(device, unet8):
    """The seeded guided DDPM chain (standard-recurrence-2, five steps) against the oracle's guided loop on the ledger tape."""
    m, sd = unet8
    d = _ddpm(device, m)
    shape = (3, HZ, 8)
    guid, okw = GUIDED[0]
    obj = cindm_amd.PointObjective([0.25, -0.5], **okw)
    tape = ledger_tape(device, shape, ddpm_rows(TS), T, relax=2)
    od = O.Diffusion1D(sd, image_size=HZ, conditioned_steps=0)
    kw = dict(n_composed=0, compose_mode="mean-inside", design_fn=obj, design_guidance=guid, t_stop=T - 5)
    ref = O.sample(od, 3, O.NoiseTape(tape.init.cpu(), tape.step.cpu(), tape.recur.cpu()), **kw)
    out = d.sample(batch_size=3, seed=SEED, sample_offset=OFF, **kw)
    assert _say("seeded guided DDPM vs oracle on the ledger tape", rel(out, ref)) < TOL_CHAIN


# ------------------------------------------------------------------ c. the 2-D chains
CH, FRAMES = 21, 6
PMIN, PMAX = -37.7, 57.6


def draw2d(device, d, shape, word, seed=SEED, off=OFF):
    """(state [B, 1, C-3, H, W], boundary [B, nb, 3, H, W]) of cindm_fill_noise2d under (seed, word): the 2d-state stream keyed by
    the design, the 2d-boundary stream by the image under the xor'd seed."""
    B, nb, Cc, H, W = shape
    assert N.STREAM["2d-state"]["seed_word"](seed) == seed and N.STREAM["2d-boundary"]["seed_word"](seed) == seed ^ N.BOUND2D_XOR
    x = from_device_layout(dev_fill2d(device, B, nb, H * W, Cc, d.model.padded_channels, seed, off, word), Cc, H, W).reshape(shape)
    return x[:, :1, :-3].contiguous(), x[:, :, -3:].contiguous()


def ledger_tape2d(device, d, shape, rows, n_rows):
    """The NoiseTape2D with x_T under word T and row ``row`` under word t, for (row, t) in rows."""
    B, nb, Cc, H, W = shape
    ss = torch.zeros((n_rows, B, 1, Cc - 3, H, W), device=device)
    sb = torch.zeros((n_rows, B, nb, 3, H, W), device=device)
    for row, t in rows:
        ss[row], sb[row] = draw2d(device, d, shape, N.STREAM["2d-state"]["step_word"](t, 0, 0, d.num_timesteps))
    return cindm_amd.NoiseTape2D(draw2d(device, d, shape, d.num_timesteps), ss, sb)


@pytest.fixture(scope="module")
def unet2d_32(device):
    return build_unet2d(device, image_size=32)


@pytest.fixture(scope="module")
def unet2d_64(device):
    return build_unet2d(device)


@pytest.fixture(scope="module")
def force(device):
    sd = O.synth_state_dict_2d(O.force_unet_param_shapes(), 7)
    m = cindm_amd.ForceUnet(dim=64, dim_mults=(1, 2, 4, 8), channels=4)
    m.load_state_dict(sd, strict=True)
    return m.to(device)


def _diff2d(unet, device, size, S, Tn=1000):
    return cindm_amd.GaussianDiffusion(unet[0], image_size=size, frames=FRAMES, cond_frames=2, timesteps=Tn, loss_type="l2",
                                       sampling_timesteps=S, coeff_ratio=0.05, ddim_sampling_eta=0.5).to(device)


def _run2d(device, unet, size, ddim, fo=None):
    """(run, tape) of one 2-D chain: DDPM = the whole chain of a 4-timestep diffusion, DDIM = the first 3 steps of S = 250."""
    shape = (2, 2, CH, size, size)
    gkw = {} if fo is None else dict(design_fn=fo, design_guidance="standard-alpha")
    if ddim:
        d = _diff2d(unet, device, size, 250)
        times, _ = d.ddim_schedule()
        tape = ledger_tape2d(device, d, shape, [(i, times[i]) for i in range(3)], 3)
        return (lambda **kw: d.ddim_sample(shape, step_range=(0, 3), **gkw, **kw)), tape
    d = _diff2d(unet, device, size, 4, Tn=4)
    tape = ledger_tape2d(device, d, shape, [(t, t) for t in (3, 2, 1)], 4)
    return (lambda **kw: d.p_sample_loop(shape, **gkw, **kw)), tape


@pytest.mark.parametrize("ddim", [False, True], ids=["ddpm", "ddim"])
def test_2d_plain_chains(device, unet2d_32, ddim):
    """32 x 32, 2 designs x 2 boundaries: state channels under (seed, design), boundary channels under (seed ^ 0x9e37..., image),
    x_T at word T, steps at word t, element pix * CP + c."""
    run, tape = _run2d(device, unet2d_32, 32, ddim)
    out = same(run, tape)
    assert all(torch.equal(out[:, 0, :-3], out[:, k, :-3]) for k in range(1, out.shape[1]))


@pytest.mark.parametrize("ddim", [False, True], ids=["ddpm_force", "ddim_force"])
def test_2d_force_guided_chains(device, unet2d_64, force, ddim):
    """The two chains guided by the ForceObjective (64 x 64: the surrogate's only size), same keys as the plain chains."""
    fo = cindm_amd.ForceObjective(force, 2, 2, FRAMES, p_min=PMIN, p_max=PMAX)
    run, tape = _run2d(device, unet2d_64, 64, ddim, fo)
    same(run, tape)
