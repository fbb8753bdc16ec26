"""GPU (MI355X): replacement conditioning of the 2-D chains (``known=`` / ``known_mask=`` / ``cond=``; cindm_ddpm1d_set_known2d,
known2d_kernel) -- the four library chains against the per-step Python routes with ``GaussianDiffusion.known_replace`` (the
definition in torch), against the CPU oracle's pieces, and the bitwise properties the definition promises.

The region of most tests: ``cond=`` (cond_frames = 2: channels 0 .. 5, i.e. channel group 0 whole and half of group 1) plus the
boundary image of design 0's copy 1 (channels 18 .. 20: the upper half of group 4 and, of group 5, the one channel that is not
padding), so whole, partial and padded groups of the kernel's 16-byte stores all occur; two boundary copies is the smallest case
in which the shared state draw can go wrong.

Short DDPM chains: a diffusion with timesteps = 5 (or 2) runs its WHOLE chain in that many steps -- rule 1, steps with
t_next >= 0 and the last one with t_next < 0 -- on tapes of that many rows; a 1000-step diffusion cut by ``t_stop`` covers the
truncated chain.  Tolerances: fused against the per-step loop 1e-6 (test_guided_ddim2d_fused_equals_loop_equals_eager's bound);
single steps against the oracle 2e-5 (TOL_STEP of tests/test_gpu_parity_2d.py, TOL of tests/test_gpu_ddim_guided_2d.py)."""
import pytest
import torch

import cindm_amd
import cindm_oracle as O
from test_gpu_parity_2d import build_unet2d, rel

pytestmark = pytest.mark.gpu

TOL = 2e-5
CH, HW, FRAMES = 21, 64, 6
PMIN, PMAX = -37.7, 57.6


@pytest.fixture(scope="module")
def unet2d(device):
    return build_unet2d(device)


@pytest.fixture(scope="module")
def force(device):
    sd = O.synth_state_dict_2d(O.force_unet_param_shapes(), 7)
    m = cindm_amd.ForceUnet(dim=64, dim_mults=(1, 2, 4, 8), channels=4)
    m.load_state_dict(sd, strict=True)
    return m.to(device), sd


def _diff(unet2d, device, S, T=1000, **kw):
    kw.setdefault("coeff_ratio", 0.05)
    return cindm_amd.GaussianDiffusion(unet2d[0], image_size=64, frames=FRAMES, cond_frames=2, timesteps=T, loss_type="l2",
                                       sampling_timesteps=S, **kw).to(device)


def _objective(force, B, nb):
    return cindm_amd.ForceObjective(force[0], B, nb, FRAMES, p_min=PMIN, p_max=PMAX)


def _tape(seed, steps, shape):
    """Step rows and known rows of ``steps`` steps (DDPM with T = steps: indexed by t; DDIM: by step index)."""
    b, nb, c, h, w = shape
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(s, generator=g)
    return cindm_amd.NoiseTape2D((rn(b, 1, c - 3, h, w), rn(b, nb, 3, h, w)), rn(steps, b, 1, c - 3, h, w), rn(steps, b, nb, 3, h, w),
                                 known_init=(rn(b, 1, c - 3, h, w), rn(b, nb, 3, h, w)), known_state=rn(steps, b, 1, c - 3, h, w),
                                 known_boundary=rn(steps, b, nb, 3, h, w))


def _region(seed, shape, device):
    """(keywords of the sampling calls, values k and mask m [B, nb, C, H, W] on the device): cond= plus one boundary image."""
    b, nb, c, h, w = shape
    g = torch.Generator().manual_seed(seed)
    cond = torch.rand((b, 6, h, w), generator=g) * 2 - 1
    known = torch.rand(shape, generator=g) * 2 - 1
    km = torch.zeros(shape, dtype=torch.bool)
    km[0, 1, -3:] = True
    k, m = known.clone(), km.clone()
    k[:, :, :6] = cond[:, None]
    m[:, :, :6] = True
    return dict(cond=cond.to(device), known=known.to(device), known_mask=km.to(device)), k.to(device), m.to(device)


def _x_T(tape, shape, device):
    return O.sample_noise_2d(*tape.init).reshape(shape[0] * shape[1], *shape[2:]).to(device)


def _step_noise(tape, row, shape, device):
    return O.sample_noise_2d(tape.step_state[row], tape.step_boundary[row]).reshape(shape[0] * shape[1], *shape[2:]).to(device)


def _q(d, k, t, zs, zb):
    """The definition, written out: q(k, t, z) with the state draw shared over the boundary copies."""
    if t < 0:
        return k
    z = O.sample_noise_2d(zs, zb).to(k.device)
    return d.sqrt_alphas_cumprod[t] * k + d.sqrt_one_minus_alphas_cumprod[t] * z


def _counter_noise(d, shape, seed, tag, device):
    """The counter-based draw keyed (seed, design / image, tag) as [B*nb, C, H, W]: what a chain's step at t = tag adds."""
    from cindm_amd import _ffi
    b, nb, c, h, w = shape
    cp = d.model.padded_channels
    z = torch.empty((b * nb, h * w, cp), dtype=torch.float32, device=device)
    with torch.cuda.device(device):
        _ffi.check(_ffi.lib().cindm_fill_noise2d(_ffi.ptr(z), b, nb, h * w, c, cp, seed, 0, tag, _ffi.current_stream(device)))
    return cindm_amd.unet2d.from_device_layout(z, c, h, w)


def _shared(x):
    return all(torch.equal(x[:, 0, :-3], x[:, k, :-3]) for k in range(1, x.shape[1]))


# ------------------------------------------------------------------ 1. chain equals loop
def _ddpm_loop(d, shape, tape, k, m, fn=None):
    """p_sample per step + the torch helper (T = the tape's rows: the whole chain)."""
    T = d.num_timesteps
    x = d.known_replace(shape, _x_T(tape, shape, k.device), k, m, T - 1, tape.known_init)
    for t in range(T - 1, -1, -1):
        nz = _step_noise(tape, t, shape, k.device) if t > 0 else None
        x, _ = d.p_sample(shape, x, t, design_fn=fn, design_guidance="standard-alpha", noise=nz)
        x = d.known_replace(shape, x, k, m, t - 1, None if t == 0 else (tape.known_state[t], tape.known_boundary[t]))
    return x.reshape(shape)


def _ddim_loop(d, shape, tape, k, m, i0, i1):
    """One-step ddim_sample calls (no region) + the torch helper."""
    times, _ = d.ddim_schedule()
    x = d.known_replace(shape, _x_T(tape, shape, k.device), k, m, times[i0], tape.known_init)
    for i in range(i0, i1):
        x = d.ddim_sample(shape, noise=tape, init_img=x, step_range=(i, i + 1))
        x = d.known_replace(shape, x, k, m, times[i + 1], None if times[i + 1] < 0 else (tape.known_state[i], tape.known_boundary[i]))
    return x.reshape(shape)


@pytest.mark.parametrize("chain", ["ddpm", "ddim", "ddpm_force", "ddim_force"])
def test_known2d_chain_equals_loop_equals_eager(device, unet2d, force, chain):
    guided, ddim = chain.endswith("force"), chain.startswith("ddim")
    shape = (2, 2, CH, HW, HW) if ddim else (1, 2, CH, HW, HW)
    kw, k, m = _region(5, shape, device)
    fn = _objective(force, shape[0], 2) if guided else None
    gkw = dict(design_fn=fn, design_guidance="standard-alpha") if guided else {}
    if ddim:
        d = _diff(unet2d, device, 250, ddim_sampling_eta=0.5)
        tape = _tape(31, 5, shape)
        run = lambda **o: d.ddim_sample(shape, noise=tape, step_range=(0, 5), **gkw, **kw, **o)
        loop = run(fused=False) if guided else _ddim_loop(d, shape, tape, k, m, 0, 5)
        t_end = d.ddim_schedule()[0][5]
        want = _q(d, k, t_end, tape.known_state[4], tape.known_boundary[4])
    else:
        d = _diff(unet2d, device, 5, T=5)
        tape = _tape(32, 5, shape)
        run = lambda **o: d.p_sample_loop(shape, noise=tape, **gkw, **kw, **o)
        loop = _ddpm_loop(d, shape, tape, k, m, fn)
        if guided:
            assert torch.equal(run(fused=False), loop)          # the class's own per-step route IS that loop
        want = k
    fused = run()
    eager = run(use_graph=False)
    assert bool(torch.isfinite(fused).all())
    r = rel(fused, loop)
    print(f"{chain}: fused vs per-step loop rel {r:.3e}")
    assert torch.equal(fused[m], loop[m]) and torch.equal(fused[m], want[m])
    assert r < 1e-6
    assert torch.equal(fused, eager)
    plain = d.ddim_sample(shape, noise=tape, step_range=(0, 5), **gkw) if ddim else d.p_sample_loop(shape, noise=tape, **gkw)
    assert not torch.equal(fused[~m], plain[~m])                # the region steers the rest of the state


# ------------------------------------------------------------------ 2. final exactness
def test_known2d_final_exactness(device, unet2d):
    shape = (2, 2, CH, HW, HW)
    kw, k, m = _region(6, shape, device)
    d = _diff(unet2d, device, 50, ddim_sampling_eta=0.5)
    x = torch.randn(shape, generator=torch.Generator().manual_seed(1)) * 0.6
    x[:, 1, :-3] = x[:, 0, :-3]
    out = d.ddim_sample(shape, init_img=x.to(device), step_range=(48, 50), seed=3, **kw)          # the last two pairs
    assert bool(torch.isfinite(out).all()) and torch.equal(out[m], k[m])
    d2 = _diff(unet2d, device, 2, T=2)                                                              # the DDPM steps t = 1, 0
    out = d2.p_sample_loop(shape, seed=3, **kw)
    assert bool(torch.isfinite(out).all()) and torch.equal(out[m], k[m])
    assert not torch.equal(out[~m], d2.p_sample_loop(shape, seed=3)[~m])


# ------------------------------------------------------------------ 3. everything known
def test_known2d_everything_known(device, unet2d):
    """With the whole state known one step returns the region's level, whatever the model predicted from whatever input."""
    shape = (1, 2, CH, HW, HW)
    g = torch.Generator().manual_seed(8)
    k = torch.rand(shape, generator=g) * 2 - 1
    k[:, 1, :-3] = k[:, 0, :-3]
    k = k.to(device)
    every = torch.ones((), dtype=torch.bool)
    d = _diff(unet2d, device, 50, ddim_sampling_eta=0.5)
    times, _ = d.ddim_schedule()
    tape = _tape(9, 50, shape)
    xa, xb = torch.randn(shape, generator=g).to(device), torch.zeros(shape, device=device)
    for x in (xa, xb):
        last = d.ddim_sample(shape, init_img=x, step_range=(49, 50), known=k, known_mask=every)
        assert torch.equal(last, k)
        first = d.ddim_sample(shape, init_img=x, step_range=(0, 1), noise=tape, known=k, known_mask=every)
        assert torch.equal(first, _q(d, k, times[1], tape.known_state[0], tape.known_boundary[0]))
    d5 = _diff(unet2d, device, 5, T=5)
    t5 = _tape(10, 5, shape)
    one = d5.p_sample_loop(shape, noise=t5, t_stop=4, known=k, known_mask=every)                    # the step at t = 4: level 3
    assert torch.equal(one, _q(d5, k, 3, t5.known_state[4], t5.known_boundary[4]))
    assert torch.equal(d5.p_sample_loop(shape, noise=t5, known=k, known_mask=every), k)


# ------------------------------------------------------------------ 4. one teacher-forced step against the oracle's pieces
def test_known2d_teacher_forced_steps_vs_oracle(device, unet2d):
    """DDPM: the first step of a 5-step diffusion (t = 4) from x_T = the tape's init rows (p_sample_loop with t_stop = 4) -- rule 1
    on x_T, O.p_sample_2d, rule 2 at level 3.  DDIM (S = 50, eta 0.5): the pairs 24 (t_next >= 0) and 49 (t_next = -1) from a given state -- rule 1 at
    the pair's t, O.model_predictions_2d + O.ddim_coefs, rule 2.  The definition itself in CPU torch."""
    shape = (1, 2, CH, HW, HW)
    B, nb = shape[:2]
    kw, k, m = _region(12, shape, device)
    kc, mc = k.cpu(), m.cpu()
    od = O.Diffusion2D(unet2d[1], image_size=64, frames=FRAMES, coeff_ratio=0.05)
    sa, sm = od.tab["sqrt_alphas_cumprod"], od.tab["sqrt_one_minus_alphas_cumprod"]
    q = lambda t, zs, zb: kc if t < 0 else sa[t] * kc + sm[t] * O.sample_noise_2d(zs, zb)
    # DDPM
    d = _diff(unet2d, device, 5, T=5)
    o5 = O.Diffusion2D(unet2d[1], image_size=64, frames=FRAMES, timesteps=5)
    s5, m5 = o5.tab["sqrt_alphas_cumprod"], o5.tab["sqrt_one_minus_alphas_cumprod"]
    q5 = lambda t, zs, zb: s5[t] * kc + m5[t] * O.sample_noise_2d(zs, zb)
    g = torch.Generator().manual_seed(13)
    tape = _tape(13, 5, shape)
    x = torch.where(mc, q5(4, *tape.known_init), O.sample_noise_2d(*tape.init))
    nz = O.sample_noise_2d(tape.step_state[4], tape.step_boundary[4]).reshape(B * nb, CH, HW, HW)
    ref, _ = O.p_sample_2d(o5, shape, x.reshape(B * nb, CH, HW, HW), 4, nz)
    ref = torch.where(mc, q5(3, tape.known_state[4], tape.known_boundary[4]), ref.reshape(shape))
    out = d.p_sample_loop(shape, noise=tape, t_stop=4, **kw)
    r = rel(out, ref)
    print(f"DDPM step t=4 of 5 with a known region: rel {r:.3e}")
    assert r < TOL and torch.equal(out.cpu()[mc], ref[mc])
    # DDIM
    dd = _diff(unet2d, device, 50, ddim_sampling_eta=0.5)
    pairs = O.ddim_time_pairs(1000, 50)
    tp = _tape(14, 50, shape)
    for i in (24, 49):
        t, tn = pairs[i]
        x0_ = torch.randn(shape, generator=g) * 0.6
        x0_[:, 1, :-3] = x0_[:, 0, :-3]
        x = torch.where(mc, q(t, *tp.known_init), x0_).reshape(B * nb, CH, HW, HW)
        eps, xs = O.model_predictions_2d(od, shape, x, t, clip_x_start=True, rederive_pred_noise=True)
        if tn < 0:
            ref = xs
        else:
            san, cc, sg = O.ddim_coefs(od, t, tn, 0.5)
            ref = xs * san + cc * eps + sg * O.sample_noise_2d(tp.step_state[i], tp.step_boundary[i]).reshape(B * nb, CH, HW, HW)
        ref = torch.where(mc, q(tn, tp.known_state[i], tp.known_boundary[i]), ref.reshape(shape))
        out = dd.ddim_sample(shape, init_img=x0_.to(device), step_range=(i, i + 1), noise=tp, **kw)
        r = rel(out, ref)
        print(f"DDIM step i={i} t={t} t_next={tn} with a known region: rel {r:.3e}")
        assert r < TOL and torch.equal(out.cpu()[mc], ref[mc])


# ------------------------------------------------------------------ 5. nothing known
def test_known2d_nothing_known_and_arming_is_consumed(device, unet2d):
    shape = (1, 2, CH, HW, HW)
    kw, k, m = _region(15, shape, device)
    none = torch.zeros((), dtype=torch.bool)
    for d, run in ((_diff(unet2d, device, 250, ddim_sampling_eta=0.5), lambda d, **o: d.ddim_sample(shape, seed=4, step_range=(0, 3), **o)),
                   (_diff(unet2d, device, 1000), lambda d, **o: d.p_sample_loop(shape, seed=4, t_stop=997, **o))):
        plain = run(d)
        assert torch.equal(run(d, known=k, known_mask=none), plain)          # an all-false mask: the plain chain, bit for bit
        held = run(d, **kw)
        assert not torch.equal(held, plain)
        assert torch.equal(run(d), plain)                                      # the arming was consumed by the call it armed
    # ... also by a call that fails: arm by hand, let the chain refuse its arguments, run the plain chain
    from cindm_amd import _ffi
    keep = d._known_arm(d._handle(), (k, m), shape, None, slice(None), torch.device(device))
    with pytest.raises(cindm_amd.CindmError):
        d.p_sample_loop(shape, seed=4, t_stop=1000)                           # bad timestep range: refused before any work
    assert torch.equal(run(d), plain)
    # ... and a region made for another state is refused with the reason, before the state is touched
    d._known_arm(d._handle(), (k[:, :1], m[:, :1]), (1, 1, CH, HW, HW), None, slice(None), torch.device(device))
    with pytest.raises(cindm_amd.CindmError, match="known region: made for 1 images"):
        run(d)
    assert torch.equal(run(d), plain)
    del keep


# ------------------------------------------------------------------ 6. invariants (counter-based draws)
@pytest.mark.parametrize("ddim", [False, True], ids=["ddpm", "ddim"])
def test_known2d_invariants_and_counter_draws(device, unet2d, ddim):
    """State channels stay shared over the boundary axis, boundary channels do not; a batch of 2 equals its halves run with
    sample_offset; and the counter-based draws of the library chain are the ones the Python routes make (``_known_z``: the per-step
    loop is written out here with them) -- the known region bit for bit, the state within the fused-against-loop bound.  The DDPM chain is a truncated one: it ends at level t_stop - 1."""
    shape, half = (2, 2, CH, HW, HW), (1, 2, CH, HW, HW)
    kw, k, m = _region(16, shape, device)
    if ddim:
        d = _diff(unet2d, device, 250, ddim_sampling_eta=0.5)
        run = lambda shp, **o: d.ddim_sample(shp, seed=7, step_range=(0, 3), **o)
    else:
        d = _diff(unet2d, device, 1000)
        run = lambda shp, **o: d.p_sample_loop(shp, seed=7, t_stop=997, **o)
    full = run(shape, **kw)
    assert bool(torch.isfinite(full).all())
    assert _shared(full) and not torch.equal(full[:, 0, -3:], full[:, 1, -3:])
    assert not torch.equal(full[m], k[m])                                      # the chain stopped at a level with noise
    cut = lambda o, a, b: {n: v[a:b] for n, v in o.items()}
    lo, hi = run(half, sample_offset=0, **cut(kw, 0, 1)), run(half, sample_offset=1, **cut(kw, 1, 2))
    assert torch.equal(full[:1], lo) and torch.equal(full[1:], hi)
    dev = torch.device(device)
    kz = lambda row, tag: d._known_z(shape, None, row, tag, 7, 0, dev)
    x = cindm_amd.unet2d.from_device_layout(d._x_T(shape, None, 7, 0, dev), CH, HW, HW)
    if ddim:
        times, _ = d.ddim_schedule()
        x = d.known_replace(shape, x, k, m, times[0], kz(None, d.num_timesteps))
        for i in range(3):
            x = d.ddim_sample(shape, seed=7, init_img=x, step_range=(i, i + 1))
            x = d.known_replace(shape, x, k, m, times[i + 1], kz(i, times[i + 1]))
    else:
        x = d.known_replace(shape, x, k, m, 999, kz(None, d.num_timesteps))
        for t in (999, 998, 997):
            x, _ = d.p_sample(shape, x, t, noise=_counter_noise(d, shape, 7, t, dev))          # the chain's own step draw: (seed, design, t)
            x = d.known_replace(shape, x, k, m, t - 1, kz(t, t - 1))
    loop = x.reshape(shape)
    r = rel(full, loop)
    print(f"counter draws, chain vs per-step loop: rel {r:.3e}")
    assert torch.equal(full[m], loop[m]) and r < 1e-6


# ------------------------------------------------------------------ 7. recorder
def test_known2d_recorder_records_after_the_overwrite(device, unet2d):
    shape = (1, 2, CH, HW, HW)
    kw, k, m = _region(17, shape, device)
    d = _diff(unet2d, device, 250, ddim_sampling_eta=0.5)
    times, _ = d.ddim_schedule()
    tape = _tape(18, 4, shape)
    out, rec = d.ddim_sample(shape, noise=tape, step_range=(0, 4), return_trajectory_every=2, **kw)
    assert len(rec) == 2
    assert torch.equal(rec.x[-1], out)
    assert torch.equal(rec.x[0][m], _q(d, k, times[2], tape.known_state[1], tape.known_boundary[1])[m])
    assert torch.equal(out[m], _q(d, k, times[4], tape.known_state[3], tape.known_boundary[3])[m])
    assert torch.equal(out, d.ddim_sample(shape, noise=tape, step_range=(0, 4), **kw))
    d5 = _diff(unet2d, device, 5, T=5)
    t5 = _tape(19, 5, shape)
    out, rec = d5.p_sample_loop(shape, noise=t5, return_trajectory_every=2, trajectory=("x", "x0"), **kw)
    assert len(rec) == 3 and torch.equal(rec.x[-1], out) and torch.equal(out[m], k[m])
    assert torch.equal(rec.x[0][m], _q(d5, k, 2, t5.known_state[3], t5.known_boundary[3])[m])      # after the steps t = 4, 3: level 2


# ------------------------------------------------------------------ 8. recovery
def test_known2d_exchange_timeout_is_recovered(device, unet2d):
    """As test_guided_ddim2d_exchange_timeout_is_recovered (option `dbg` = 39: slab 1 of every image never publishes), with a
    known region: the re-run starts from rule 1 again on the kept x_T, so the recovered chain IS the undisturbed one."""
    sd = O.synth_state_dict_2d(O.force_unet_param_shapes(), 7)

    def model():
        m = cindm_amd.ForceUnet(dim=64, dim_mults=(1, 2, 4, 8), channels=4)
        m.load_state_dict(sd, strict=True)
        return m.to(device)

    shape = (1, 2, CH, HW, HW)
    rkw, k, msk = _region(20, shape, device)
    d = _diff(unet2d, device, 250, ddim_sampling_eta=0.5)
    tape = _tape(31, 3, shape)
    kw = dict(design_guidance="standard-alpha", noise=tape, step_range=(0, 3), **rkw)
    ref = model().set_option("gn_bwd_fused", 1)                     # the exchange-free derivative, selected up front
    want = d.ddim_sample(shape, design_fn=cindm_amd.ForceObjective(ref, 1, 2, FRAMES, p_min=PMIN, p_max=PMAX), **kw)
    m = model()
    m.set_option("dbg", 39)
    before = m.recovered
    got = d.ddim_sample(shape, design_fn=cindm_amd.ForceObjective(m, 1, 2, FRAMES, p_min=PMIN, p_max=PMAX), **kw)
    m.set_option("dbg", 0)
    assert m.recovered == before + 1 and bool(torch.isfinite(got).all()) and torch.equal(got, want)
    times, _ = d.ddim_schedule()
    assert torch.equal(got[msk], _q(d, k, times[3], tape.known_state[2], tape.known_boundary[2])[msk])
