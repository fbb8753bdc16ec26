"""GPU (MI355X): the chain recorder (``return_trajectory_every=`` / ``trajectory=``; cindm_ddpm1d_set_recorder, chain_record_kernel).

The central check needs no oracle: the noise is a function of (seed, design, step), so record r of a chain must be ``torch.equal`` to
the result of the same call cut at that step with the same seed (``t_stop=`` for the DDPM loops, ``step_range=(0, step)`` for the DDIM
loops).  Two tape-driven chains are also held to the CPU oracle's ``record=`` callbacks, which pins the step <-> record mapping to an
independent implementation.  Every chain is a handful of steps at 1 .. 5 designs (32 where the exchange kernels must run)."""
import ctypes as C

import pytest
import torch

import cindm_amd
import cindm_oracle as O
from cindm_amd import _ffi
from test_gpu_parity import TOL_CHAIN, TOL_STEP, build_unet, rel
from test_gpu_parity_2d import build_unet2d

pytestmark = pytest.mark.gpu

HZ = 24
PMIN, PMAX, FRAMES = -37.7, 57.6, 6


def _say(name, v):
    print(f"[chain-record] {name}: {v:.3e}" if isinstance(v, float) else f"[chain-record] {name}: {v}")
    return v


@pytest.fixture(scope="module")
def unet8(device):
    return build_unet(device)


def _diff(device, m, S=1000, eta=0.0):
    return cindm_amd.GaussianDiffusion1D(m, image_size=HZ, conditioned_steps=0, timesteps=1000, sampling_timesteps=S,
                                         loss_type="l1", ddim_sampling_eta=eta).to(device)


@pytest.fixture(scope="module")
def diff8(device, unet8):
    return _diff(device, unet8[0])


@pytest.fixture(scope="module")
def unet2d32(device):
    return build_unet2d(device, image_size=32)


def _diff2d(device, m, size, S=None, **kw):
    return cindm_amd.GaussianDiffusion(m, image_size=size, frames=FRAMES, cond_frames=2, timesteps=1000, sampling_timesteps=S,
                                       loss_type="l2", **kw).to(device)


PLAIN = dict(batch_size=5, n_composed=0, compose_n_bodies=2, seed=7)          # the chain of tests 1, 2 and 7: t 999 -> 987, 13 steps


def _check_cuts(rec, cut, want_steps):
    """Record r == the same call cut after rec.step[r] steps, bit for bit."""
    assert rec.step == want_steps
    assert rec.x.shape[0] == len(want_steps)
    for r, (s, t) in enumerate(zip(rec.step, rec.t)):
        assert torch.equal(rec.x[r], cut(s, t)), (r, s, t)


# ------------------------------------------------------------------ 1. plain 1-D DDPM: fused update, ping-pong step state, odd count
def test_plain_ddpm_records_equal_cut_chains(diff8):
    d = diff8
    base = d.sample(t_stop=987, **PLAIN)
    n0, fused0 = d.last_step_info()
    out, rec = d.sample(t_stop=987, return_trajectory_every=4, **PLAIN)
    n1, fused1 = d.last_step_info()
    assert isinstance(rec, cindm_amd.ChainRecord) and rec.x0 is None
    assert rec.t == [996, 992, 988, 987] and tuple(rec.x.shape) == (4, 5, HZ, 8)
    assert torch.equal(out, base) and torch.equal(rec.x[-1], out)
    _check_cuts(rec, lambda s, t: d.sample(t_stop=t, **PLAIN), [4, 8, 12, 13])
    _say("launches per step without / with the recorder", (n0, n1))
    assert fused0 and fused1 and n1 == n0 + 1                              # exactly one launch more, the update still fused
    d.sample(t_stop=987, **PLAIN)
    assert d.last_step_info() == (n0, fused0)                              # and the same count as before with no recorder set
    out2, rec2 = d.sample(t_stop=987, return_trajectory_every=4, use_graph=False, **PLAIN)
    assert torch.equal(out2, out) and torch.equal(rec2.x, rec.x) and rec2.step == rec.step
    # an even count (no tail graph) and every > n (one record: the result)
    out3, rec3 = d.sample(t_stop=988, return_trajectory_every=50, **PLAIN)
    assert rec3.step == [12] and rec3.t == [988] and torch.equal(rec3.x[0], out3) and torch.equal(out3, rec.x[2])


def test_every_at_the_top_of_int32_records_the_result_alone(device, diff8):
    """every = 2**31 - 1 ("only the result") on chains of two or more steps: s + every - 1 must not wrap in the kernel's record index.
    The record tensor sits between two guard tensors of the same size, which must stay untouched."""
    d, L, big = diff8, _ffi.lib(), 2 ** 31 - 1
    base = d.sample(t_stop=987, **PLAIN)
    out, rec = d.sample(t_stop=987, return_trajectory_every=big, trajectory=("x", "x0"), **PLAIN)
    assert rec.step == [13] and rec.t == [987] and tuple(rec.x.shape) == (1, 5, HZ, 8)
    assert torch.equal(out, base) and torch.equal(rec.x[0], out)
    _, rec1 = d.sample(t_stop=987, return_trajectory_every=13, trajectory=("x", "x0"), **PLAIN)
    assert torch.equal(rec.x0, rec1.x0)
    # through the C entry, into the middle third of one allocation
    B, fpr = 3, 3 * HZ * 8
    arena = torch.full((3 * fpr,), 7.0, device=device)
    x = d._init_state((B, HZ, 8), device, None, 5, 0, d.num_timesteps)
    desc = d._desc_for((B, HZ, 8), "mean", 0, 4, HZ, 2, outside=True)
    h, un, ws = d._prepare(desc, B, device)
    _ffi.check(L.cindm_ddpm1d_set_recorder(h, C.c_void_p(arena.data_ptr() + 4 * fpr), fpr, big, 1))
    with torch.cuda.device(device):
        _ffi.check(L.cindm_ddpm1d_sample(h, d.model._h, un, C.byref(desc), _ffi.ptr(x), None, None, C.c_uint64(5), 0, None, 0, None,
                                         999, 997, B, _ffi.ptr(ws), ws.numel(), _ffi.current_stream(device), 1))
    torch.cuda.synchronize(device)
    assert torch.equal(arena[fpr:2 * fpr].view(B, HZ, 8), x)
    assert bool((arena[:fpr] == 7.0).all()) and bool((arena[2 * fpr:] == 7.0).all())


# ------------------------------------------------------------------ 2. the x0 stream
def test_x0_stream(device, diff8):
    d = diff8
    base, rec_x = d.sample(t_stop=987, return_trajectory_every=1, **PLAIN)
    out, rec = d.sample(t_stop=987, return_trajectory_every=1, trajectory=("x", "x0"), **PLAIN)
    n, fused = d.last_step_info()
    assert not fused                                                       # x0 comes from the separate update launch
    assert rec.step == list(range(1, 14)) and rec.t == list(range(999, 986, -1))
    assert tuple(rec.x0.shape) == (13, 5, HZ, 8)
    # the separate update launch is bit-identical to the fused one
    assert torch.equal(out, base) and torch.equal(rec.x, rec_x.x) and torch.equal(rec.x[-1], out)
    x_prev = d._init_state((5, HZ, 8), device, None, PLAIN["seed"], 0, d.num_timesteps)          # x_T of that seed
    kw = dict(compose_mode="mean", n_composed=0, single_model_step=HZ, compose_n_bodies=2)
    worst, bit_equal = 0.0, True
    for r, t in enumerate(rec.t):
        x0 = d.p_sample_compose_outside(x_prev, None, t, **kw)[1]          # the library's own single step on the recorded predecessor
        worst = max(worst, rel(rec.x0[r], x0))
        bit_equal = bit_equal and torch.equal(rec.x0[r], x0)
        x_prev = rec.x[r]
    _say("x0 vs single step, max rel", worst)
    _say("x0 vs single step, bit-equal", bit_equal)
    assert worst < TOL_STEP
    assert float(rec.x0.abs().max()) <= 1.0                                # clamped, as the update used it
    # x0 alone
    out1, rec1 = d.sample(t_stop=987, return_trajectory_every=4, trajectory=("x0",), **PLAIN)
    assert rec1.x is None and torch.equal(out1, base) and torch.equal(rec1.x0, rec.x0[[3, 7, 11, 12]])


# ------------------------------------------------------------------ 3. composition over windows
def test_time_composition(diff8):
    d = diff8
    kw = dict(batch_size=3, n_composed=1, compose_start_step=16, compose_mode="mean-inside", seed=21)
    out, rec = d.sample(t_stop=994, return_trajectory_every=2, **kw)
    assert tuple(rec.x.shape) == (3, 3, HZ + 16, 8) and torch.equal(rec.x[-1], out)
    _check_cuts(rec, lambda s, t: d.sample(t_stop=t, **kw), [2, 4, 6])
    assert torch.equal(out, d.sample(t_stop=994, **kw))


# ------------------------------------------------------------------ 4. guided 1-D DDPM: a relaxation iteration is not a step
def test_guided_ddpm(diff8):
    d = diff8
    obj = cindm_amd.PointObjective([0.25, -0.5], 2, coef=2.0)
    kw = dict(batch_size=2, n_composed=0, compose_mode="mean-inside", design_fn=obj, design_guidance="standard-recurrence-2", seed=31)
    out, rec = d.sample(t_stop=995, return_trajectory_every=2, trajectory=("x", "x0"), **kw)
    assert rec.t == [998, 996, 995] and torch.equal(rec.x[-1], out)
    _check_cuts(rec, lambda s, t: d.sample(t_stop=t, **kw), [2, 4, 5])
    assert torch.equal(out, d.sample(t_stop=995, **kw))
    assert tuple(rec.x0.shape) == tuple(rec.x.shape) and float(rec.x0.abs().max()) <= 1.0
    # the generic (autograd) route of the same callable loops in Python and records with the same indexing
    out_g, rec_g = d.sample(t_stop=995, return_trajectory_every=2, **dict(kw, design_fn=lambda x: obj(x)))
    assert rec_g.step == rec.step and rec_g.t == rec.t and tuple(rec_g.x.shape) == tuple(rec.x.shape)
    assert torch.equal(rec_g.x[-1], out_g)


# ------------------------------------------------------------------ 5. 1-D DDIM
def test_ddim(device, unet8):
    d = _diff(device, unet8[0], S=10, eta=0.5)
    shape = (3, HZ, 8)
    out, rec = d.ddim_sample(shape, None, seed=41, return_trajectory_every=3, trajectory=("x", "x0"))
    times, _ = d.ddim_schedule()
    assert rec.t == [times[2], times[5], times[8], times[9]] and torch.equal(rec.x[-1], out)
    _check_cuts(rec, lambda s, t: d.ddim_sample(shape, None, seed=41, step_range=(0, s)), [3, 6, 9, 10])
    assert torch.equal(out, d.ddim_sample(shape, None, seed=41))
    assert torch.equal(rec.x0[-1], out)                                    # the last DDIM step returns its x_start
    out2, rec2 = d.sample(batch_size=3, seed=41, return_trajectory_every=3, use_graph=False)
    assert torch.equal(out2, out) and torch.equal(rec2.x, rec.x)


# ------------------------------------------------------------------ 6. guided 1-D DDIM: the ping-ponged state
@pytest.mark.parametrize("R,S,steps", [(1, 5, [2, 4, 5]), (3, 3, [2, 3])])
def test_guided_ddim(device, unet8, R, S, steps):
    """R = 3, S = 3: nine iterations, an odd count -- the result is copied back to x after the chain, and the odd-count tail graph
    carries a record node of its own."""
    d = _diff(device, unet8[0], S=S, eta=1.0)
    obj = cindm_amd.PointObjective([0.25, -0.5], 2, coef=2.0)
    shape = (2, HZ, 8)
    kw = dict(n_composed=0, compose_mode="mean-inside", design_fn=obj, design_guidance=f"standard-recurrence-{R}", seed=51)
    out, rec = d.ddim_sample(shape, None, return_trajectory_every=2, trajectory=("x", "x0"), **kw)
    assert torch.equal(rec.x[-1], out)
    assert torch.equal(rec.x0[-1], out)                                    # the last DDIM step returns its (last iteration's) x_start
    _check_cuts(rec, lambda s, t: d.ddim_sample(shape, None, step_range=(0, s), **kw), steps)
    assert torch.equal(out, d.ddim_sample(shape, None, **kw))
    out2, rec2 = d.ddim_sample(shape, None, return_trajectory_every=2, use_graph=False, **kw)
    assert torch.equal(out2, out) and torch.equal(rec2.x, rec.x)


# ------------------------------------------------------------------ 7. against the CPU oracle, with a noise tape
def test_1d_records_vs_oracle(device, unet8, diff8):
    _, sd = unet8
    od = O.Diffusion1D(sd, image_size=HZ, conditioned_steps=0)
    tape = O.NoiseTape.make(1234, (5, HZ, 8), 1000)
    states = {}
    O.p_sample_loop(od, (5, HZ, 8), None, tape, n_composed=0, compose_n_bodies=2, t_stop=987,
                    record=lambda t, img: states.__setitem__(int(t), img.clone()))
    out, rec = diff8.sample(batch_size=5, n_composed=0, compose_n_bodies=2, noise=cindm_amd.NoiseTape(tape.init, tape.step),
                            t_stop=987, return_trajectory_every=4)
    assert rec.step == [4, 8, 12, 13]
    for r, t in enumerate(rec.t):
        assert _say(f"1-D record {r} (t = {t}) vs oracle", rel(rec.x[r], states[t])) < TOL_CHAIN


def _tape2d(seed, B, nb, Cc, H, W, t_min):
    g = torch.Generator().manual_seed(seed)
    init = (torch.randn((B, 1, Cc - 3, H, W), generator=g), torch.randn((B, nb, 3, H, W), generator=g))
    ss, sb = torch.zeros((1000, B, 1, Cc - 3, H, W)), torch.zeros((1000, B, nb, 3, H, W))
    for t in range(999, t_min - 1, -1):
        ss[t] = torch.randn((B, 1, Cc - 3, H, W), generator=g)
        sb[t] = torch.randn((B, nb, 3, H, W), generator=g)
    return cindm_amd.NoiseTape2D(init, ss, sb)


def test_2d_records_vs_oracle(device, unet2d32):
    m, sd = unet2d32
    d = _diff2d(device, m, 32)
    shape = (1, 2, 21, 32, 32)
    tape = _tape2d(77, 1, 2, 21, 32, 32, 996)
    od = O.Diffusion2D(sd, image_size=32, frames=FRAMES)
    steps = {t: (tape.step_state[t], tape.step_boundary[t]) for t in range(1, 1000)}
    states = {}
    O.p_sample_loop_2d(od, shape, tape.init, steps, t_stop=996, record=lambda t, img: states.__setitem__(int(t), img.clone()))
    out, rec = d.sample(batch_size=1, num_boundaries=2, noise=tape, t_stop=996, return_trajectory_every=3)
    assert rec.step == [3, 4] and rec.t == [997, 996]
    for r, t in enumerate(rec.t):
        assert _say(f"2-D record {r} (t = {t}) vs oracle", rel(rec.x[r], states[t])) < TOL_CHAIN


# ------------------------------------------------------------------ 8. 2-D DDPM
def test_2d_ddpm(device, unet2d32):
    m, _ = unet2d32
    d = _diff2d(device, m, 32)
    kw = dict(batch_size=1, num_boundaries=2, seed=61)
    out, rec = d.sample(t_stop=996, return_trajectory_every=3, **kw)
    assert tuple(rec.x.shape) == (2, 1, 2, 21, 32, 32) and rec.t == [997, 996] and rec.x0 is None
    assert torch.equal(rec.x[-1], out) and torch.equal(out, d.sample(t_stop=996, **kw))
    _check_cuts(rec, lambda s, t: d.sample(t_stop=t, **kw), [3, 4])
    assert torch.equal(rec.x[:, :, 0, :-3], rec.x[:, :, 1, :-3])           # state channels identical across the boundary axis
    assert not torch.equal(rec.x[:, :, 0, -3:], rec.x[:, :, 1, -3:])
    out2, rec2 = d.sample(t_stop=996, return_trajectory_every=3, use_graph=False, **kw)
    assert torch.equal(out2, out) and torch.equal(rec2.x, rec.x)
    out3, rec3 = d.sample(t_stop=996, return_trajectory_every=2 ** 31 - 1, **kw)
    assert rec3.step == [4] and torch.equal(out3, out) and torch.equal(rec3.x[0], out)
    # x0 works here
    out1, rec1 = d.sample(t_stop=996, return_trajectory_every=1, trajectory=("x", "x0"), **kw)
    assert torch.equal(out1, out) and torch.equal(rec1.x[[2, 3]], rec.x) and tuple(rec1.x0.shape) == (4, 1, 2, 21, 32, 32)
    worst = 0.0
    for r in range(1, 4):
        x0 = d.p_sample((1, 2, 21, 32, 32), rec1.x[r - 1].reshape(2, 21, 32, 32), rec1.t[r])[1]
        worst = max(worst, rel(rec1.x0[r].reshape(2, 21, 32, 32), x0))
    assert _say("2-D x0 vs single step, max rel", worst) < TOL_STEP


# ------------------------------------------------------------------ 9. 2-D DDIM
def test_2d_ddim(device, unet2d32):
    m, _ = unet2d32
    d = _diff2d(device, m, 32, S=4, ddim_sampling_eta=0.5)
    shape = (1, 2, 21, 32, 32)
    out, rec = d.ddim_sample(shape, seed=71, return_trajectory_every=2)
    times, _ = d.ddim_schedule()
    assert rec.t == [times[1], times[3]] and tuple(rec.x.shape) == (2,) + shape and torch.equal(rec.x[-1], out)
    _check_cuts(rec, lambda s, t: d.ddim_sample(shape, seed=71, step_range=(0, s)), [2, 4])
    assert torch.equal(out, d.ddim_sample(shape, seed=71))
    before = torch.cuda.memory_allocated(device)
    with pytest.raises(NotImplementedError, match="x0"):
        d.ddim_sample(shape, seed=71, return_trajectory_every=2, trajectory=("x", "x0"))
    assert torch.cuda.memory_allocated(device) == before                   # refused before any device work
    # the C entry refuses it as well, before it launches anything
    L = _ffi.lib()
    buf = torch.zeros(8 * 2 * 32 * 32 * m.padded_channels, device=device)
    _ffi.check(L.cindm_ddpm1d_set_recorder(d._handle(), _ffi.ptr(buf), buf.numel(), 2, 3))
    with pytest.raises(cindm_amd.CindmError, match="x0"):
        d.ddim_sample(shape, seed=71)                                      # (armed behind the Python face's back)
    assert torch.equal(out, d.ddim_sample(shape, seed=71))                 # consumed: the next call runs unrecorded


# ------------------------------------------------------------------ 10. guided 2-D
def test_guided_2d(device):
    m, _ = build_unet2d(device)
    sdf = O.synth_state_dict_2d(O.force_unet_param_shapes(), 7)
    f = cindm_amd.ForceUnet(dim=64, dim_mults=(1, 2, 4, 8), channels=4)
    f.load_state_dict(sdf, strict=True)
    f = f.to(device)
    fo = cindm_amd.ForceObjective(f, 1, 2, FRAMES, p_min=PMIN, p_max=PMAX)
    shape = (1, 2, 21, 64, 64)
    kw = dict(design_fn=fo, design_guidance="standard-alpha", seed=81)
    d = _diff2d(device, m, 64, coeff_ratio=0.05)
    out, rec = d.sample(batch_size=1, num_boundaries=2, t_stop=998, return_trajectory_every=1, **kw)
    assert rec.t == [999, 998] and torch.equal(rec.x[-1], out)
    _check_cuts(rec, lambda s, t: d.sample(batch_size=1, num_boundaries=2, t_stop=t, **kw), [1, 2])
    dd = _diff2d(device, m, 64, S=250, ddim_sampling_eta=0.5, coeff_ratio=0.05)
    out, rec = dd.ddim_sample(shape, step_range=(0, 2), return_trajectory_every=1, **kw)
    assert torch.equal(rec.x[-1], out)
    _check_cuts(rec, lambda s, t: dd.ddim_sample(shape, step_range=(0, s), **kw), [1, 2])
    # the per-step Python route of the same definition records with the same indexing
    out_l, rec_l = dd.ddim_sample(shape, step_range=(0, 2), return_trajectory_every=1, fused=False, **kw)
    assert rec_l.step == rec.step and rec_l.t == rec.t and torch.equal(rec_l.x[-1], out_l) and tuple(rec_l.x.shape) == tuple(rec.x.shape)


def test_guided_2d_recovered_chain_records_the_rerun(device):
    """The surrogate's exchange time-out (option dbg = 39, tests/test_gpu_ddim_guided_2d.py) inside the recorded guided chains:
    force_chain_with_recovery re-arms the recorder, the records are those of the exchange-free derivative's chain."""
    m, _ = build_unet2d(device)
    sdf = O.synth_state_dict_2d(O.force_unet_param_shapes(), 7)

    def force():
        f = cindm_amd.ForceUnet(dim=64, dim_mults=(1, 2, 4, 8), channels=4)
        f.load_state_dict(sdf, strict=True)
        return f.to(device)
    fo = lambda f: cindm_amd.ForceObjective(f, 1, 2, FRAMES, p_min=PMIN, p_max=PMAX)
    shape = (1, 2, 21, 64, 64)
    d = _diff2d(device, m, 64, coeff_ratio=0.05)
    dd = _diff2d(device, m, 64, S=250, ddim_sampling_eta=0.5, coeff_ratio=0.05)
    ddpm = lambda f: d.sample(batch_size=1, num_boundaries=2, design_fn=fo(f), design_guidance="standard-alpha", seed=91, t_stop=998,
                              return_trajectory_every=1, trajectory=("x", "x0"))
    ddim = lambda f: dd.ddim_sample(shape, design_fn=fo(f), design_guidance="standard-alpha", seed=91, step_range=(0, 2),
                                    return_trajectory_every=1)
    ref = force().set_option("gn_bwd_fused", 1)                           # the exchange-free derivative, selected up front
    want_p, rec_p = ddpm(ref)
    want_i, rec_i = ddim(ref)
    f = force()
    f.set_option("dbg", 39)
    try:
        got_p, got_rec_p = ddpm(f)
        got_i, got_rec_i = ddim(f)
    finally:
        f.set_option("dbg", 0)
    assert f.recovered == 2
    assert torch.equal(got_p, want_p) and torch.equal(got_rec_p.x, rec_p.x) and torch.equal(got_rec_p.x0, rec_p.x0)
    assert torch.equal(got_i, want_i) and torch.equal(got_rec_i.x, rec_i.x) and torch.equal(got_rec_i.x[-1], got_i)


def test_multibodies_with_conditioning_rows(device, unet8):
    """sample_compose_multibodies, N <= 401: two models, conditioned_steps > 0 (the gathered step, one state slot); the records hold
    the [B, rollout_steps, F] state."""
    m4, _ = build_unet(device, F=4)
    d = cindm_amd.GaussianDiffusion1D(unet8[0], image_size=20, conditioned_steps=4, timesteps=1000, sampling_timesteps=1000).to(device)
    d.model_unconditioned = m4
    cond = (torch.rand((2, 4, 16), generator=torch.Generator().manual_seed(3)) * 2 - 1).to(device)
    out, rec = d.sample_compose_multibodies(cond, 400, 0, 4, seed=9, t_stop=395, return_trajectory_every=2, trajectory=("x", "x0"))
    assert rec.t == [398, 396, 395] and tuple(rec.x.shape) == (3, 2, 20, 16) and torch.equal(rec.x[-1], out)
    _check_cuts(rec, lambda s, t: d.sample_compose_multibodies(cond, 400, 0, 4, seed=9, t_stop=t), [2, 4, 5])
    assert torch.equal(out, d.sample_compose_multibodies(cond, 400, 0, 4, seed=9, t_stop=395))
    full, rec_f = d.sample_compose_multibodies(cond, 400, 0, 4, seed=9, t_stop=395, full_state=True, return_trajectory_every=2)
    assert tuple(full.shape) == (2, 24, 16) and torch.equal(full[:, 4:], out) and torch.equal(rec_f.x, rec.x)


# ------------------------------------------------------------------ 11. refusals
def test_refusals(device, unet8, diff8):
    m, _ = unet8
    da = cindm_amd.GaussianDiffusion1D(m, image_size=20, conditioned_steps=4, timesteps=1000, sampling_timesteps=4).to(device)
    with pytest.raises(NotImplementedError, match="return_trajectory_every"):
        da.autoregress_time_compose_sample(2, torch.zeros((2, 4, 8), device=device), 1, seed=1, return_trajectory_every=2)
    with pytest.raises(NotImplementedError, match="return_trajectory_every"):
        da.sample_compose_multibodies(torch.zeros((2, 4, 16), device=device), 1000, 2, 4, seed=1, return_trajectory_every=2)
    # the C entries: a too-small buffer is an error and x still equals x_T; the recorder is consumed by the refused call
    d, L = diff8, _ffi.lib()
    B = 3
    x_T = d._init_state((B, HZ, 8), device, None, 5, 0, d.num_timesteps)
    x = x_T.clone()
    desc = d._desc_for((B, HZ, 8), "mean", 0, 4, HZ, 2, outside=True)
    h, un, ws = d._prepare(desc, B, device)

    def sample():
        with torch.cuda.device(device):
            return L.cindm_ddpm1d_sample(h, m._h, un, C.byref(desc), _ffi.ptr(x), None, None, C.c_uint64(5), 0, None, 0, None,
                                         999, 996, B, _ffi.ptr(ws), ws.numel(), _ffi.current_stream(device), 1)
    info = (C.c_int32 * 4)()
    small = torch.zeros(2 * B * HZ * 8 - 4, device=device)                 # every = 2 over 4 steps needs two records
    _ffi.check(L.cindm_ddpm1d_set_recorder(h, _ffi.ptr(small), small.numel(), 2, 1))
    assert sample() != 0
    assert b"too small" in L.cindm_last_error()
    torch.cuda.synchronize(device)
    assert torch.equal(x, x_T) and not bool(small.any())
    _ffi.check(L.cindm_ddpm1d_recorder_info(h, info))
    assert list(info) == [0, 0, 0, 0]
    assert sample() == 0                                                   # unrecorded: the refused call consumed the recorder
    torch.cuda.synchronize(device)
    _ffi.check(L.cindm_ddpm1d_recorder_info(h, info))
    assert list(info) == [0, 0, 0, 0] and not bool(small.any())
    assert torch.equal(x, d.sample(batch_size=B, n_composed=0, compose_n_bodies=2, seed=5, t_stop=996))
    # the two chains that are left for later refuse an armed recorder before they touch anything
    big = torch.zeros(64 * B * HZ * 8, device=device)
    _ffi.check(L.cindm_ddpm1d_set_recorder(da._handle(), _ffi.ptr(big), big.numel(), 1, 1))
    with pytest.raises(cindm_amd.CindmError, match="recorder"):
        da.autoregress_time_compose_sample(2, torch.zeros((2, 4, 8), device=device), 1, seed=1)
    out = da.autoregress_time_compose_sample(2, torch.zeros((2, 4, 8), device=device), 1, seed=1)        # consumed
    assert bool(torch.isfinite(out).all()) and not bool(big.any())
    # disarming
    _ffi.check(L.cindm_ddpm1d_set_recorder(h, _ffi.ptr(big), big.numel(), 1, 1))
    _ffi.check(L.cindm_ddpm1d_set_recorder(h, None, 0, 1, 1))
    x.copy_(x_T)
    assert sample() == 0
    torch.cuda.synchronize(device)
    assert not bool(big.any())


# ------------------------------------------------------------------ 12. recovery: the re-run overwrites from record 0
def test_recovered_chain_records_the_rerun(device):
    """dbg = 39 (tests/test_gpu_paths.py::test_exchange_timeout_is_recovered): a bounded spin raises the flag, nothing faults; the
    chain is re-run once on the exchange-free plan.  What the caller reads belongs entirely to that run."""
    m, _ = build_unet(device)
    m.set_option("auto_range", 0)           # (the calibration forward at finalize would hit the ablation too)
    d = _diff(device, m)
    kw = dict(batch_size=32, n_composed=0, compose_n_bodies=2, seed=1, t_stop=995, return_trajectory_every=2, trajectory=("x", "x0"))
    m.exchange_free(True)                   # option no_exchange = 1
    ref, rec_ref = d.sample(**kw)
    m.exchange_free(False)
    assert m.recovered == 0
    m.set_option("dbg", 39)
    try:
        got, rec = d.sample(**kw)
        info = d.last_chain_info()
    finally:
        m.set_option("dbg", 0)
    assert info["recovered"] and m.recovered == 1
    assert rec.step == [2, 4, 5] and torch.equal(got, ref)
    assert torch.equal(rec.x, rec_ref.x) and torch.equal(rec.x0, rec_ref.x0) and torch.equal(rec.x[-1], got)
