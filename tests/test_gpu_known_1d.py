"""GPU (MI355X): replacement conditioning of the four 1-D library chains (``known=`` / ``known_mask=``; known1d_kernel,
cindm_ddpm1d_set_known1d).

Expectations come from ``oracle/cindm_oracle.py`` pieces (p_mean_variance, _design_shift, _relax_coefs, model_predictions,
ddim_coefs, p_sample, p_sample_compose_outside) plus the definition written out here,
    x[m] = sqrt_alphas_cumprod[l] k + sqrt_one_minus_alphas_cumprod[l] z   (l >= 0),     x[m] = k   (l < 0),
applied where DESIGN 4.5o says: before the first step at its level (rule 1), after every relaxation at level t, after the step at
level t_next.  Tolerances are the project's (tests/test_gpu_parity.py: TOL_STEP for one step, TOL_CHAIN for a chain and for the
comparison of the built-in with the generic route, as tests/test_gpu_waypoint.py and tests/test_gpu_ddim_guided.py use it); on the
region itself every tape-driven comparison is ``torch.equal``: both sides evaluate the same three fp32 operations on the same
table entries.

The region of most tests holds row 0 whole, the positions of the last two rows (partly known bodies: the kernel blends), one
interior row of body 1 whole, and body 0 of design 0 on every row (which makes the mask per design): store-without-read, blend,
skip, shared values and a per-design mask all occur at B = 3.  Seeds, objective coefficients and the short schedules (a DDPM
diffusion of 6 and of 8 timesteps over the same U-Net, so that a whole chain is 6 U-Net steps at noise levels where the region
reaches the rest of the state) were chosen by running the oracle side on the CPU first; the guards that a case is not vacuous
are asserted on the oracle at test time."""
import ctypes as C

import pytest
import torch

import cindm_amd
import cindm_oracle as O
from cindm_amd import _ffi
from test_gpu_ddim_guided import _diff, _not_degenerate, _nt, _tape
from test_gpu_parity import TOL_CHAIN, TOL_STEP, build_unet, rel

pytestmark = pytest.mark.gpu

HZ, B = 24, 3


def _say(name, v):
    print(f"[known-1d] {name}: {v:.3e}")
    return v


@pytest.fixture(scope="module")
def unet8(device):
    return build_unet(device)


def _ddpm(device, m, T=1000):
    return cindm_amd.GaussianDiffusion1D(m, image_size=HZ, conditioned_steps=0, timesteps=T, sampling_timesteps=T, loss_type="l1").to(device)


# ------------------------------------------------------------------ the region, its tapes, the definition
def region(L, F, seed=0, batch=B):
    g = torch.Generator().manual_seed(7000 + seed)
    k = (torch.rand((batch, L, F), generator=g) * 2 - 1) * 0.8
    m = torch.zeros((batch, L, F), dtype=torch.bool)
    m[:, 0, :] = True
    m[:, L - 2:, torch.tensor([f for f in range(F) if f % 4 < 2])] = True
    m[:, L // 2, 4:8] = True
    m[0, :, 0:4] = True
    assert 0 < int(m.sum()) < m.numel()
    return k, m


def ktape(seed, shape, rows, iters=0):
    g = torch.Generator().manual_seed(7100 + seed)
    t = {"known_init": torch.randn(shape, generator=g), "known_step": torch.randn((rows,) + tuple(shape), generator=g)}
    if iters:
        t["known_recur"] = torch.randn((rows, iters) + tuple(shape), generator=g)
    return t


def nt_ddpm(tape, kt):
    return cindm_amd.NoiseTape(tape.init, tape.step, tape.recur, known_init=kt["known_init"], known_step=kt["known_step"],
                               known_recur=kt.get("known_recur"))


def nt_ddim(tp, kt):
    return cindm_amd.NoiseTape(tp["init"], tp["step"], tp["recur"], known_init=kt["known_init"], known_step=kt["known_step"],
                               known_recur=kt.get("known_recur"))


def put(od, x, kn, level, z):
    """The definition, on the oracle's tables."""
    if kn is None:
        return x
    k, m = kn
    if level < 0:
        return torch.where(m, k, x)
    q = od.tab["sqrt_alphas_cumprod"][level] * k + od.tab["sqrt_one_minus_alphas_cumprod"][level] * z
    return torch.where(m, q, x)


def waypoints(L, nb, coef=2.0, **kw):
    """Waypoints off the region: body 1 at row 5, the last body at row L - 5."""
    target = torch.zeros((L, nb, 2))
    weight = torch.zeros((L, nb))
    target[5, 1] = torch.tensor([0.3, -0.2])
    target[L - 5, nb - 1] = torch.tensor([-0.4, 0.1])
    weight[5, 1] = weight[L - 5, nb - 1] = 1.0
    return cindm_amd.WaypointObjective(target, weight, coef=coef, **kw)


def inside_kw(n_composed=0, cs=4, nb=2):
    return dict(n_composed=n_composed, compose_start_step=cs, compose_n_bodies=nb, compose_mode="mean-inside")


def pmv_kw(skw, T1=HZ):
    return dict(compose_mode=skw["compose_mode"], n_composed=skw["n_composed"], compose_start_step=skw["compose_start_step"],
                single_model_step=T1, compose_n_bodies=skw["compose_n_bodies"])


# ------------------------------------------------------------------ the oracle's chains with a region, from its pieces
def o_guided_iters(od, x, t, row, recur, kn, kt, obj, guid, pk):
    """The iterations of one guided step (p_sample's recurrence branch, piece by piece), the region put back after every
    relaxation but the last, whose state is never used.  Returns the last iteration's (pred, logvar, x_start, eps, shift)."""
    R = O._recurrence_times(guid)
    for r in range(R):
        mean, logvar, x_start, eps = O.p_mean_variance(od, x, None, t, True, **pk)
        shift = O._design_shift(od, obj, guid, x, x_start, t)
        pred = mean - shift
        if r < R - 1:
            a, b = O._relax_coefs(od, t)
            x = put(od, a * pred + b * recur[row][r], kn, t, None if kn is None else kt["known_recur"][row][r])
    return pred, logvar, x_start, eps, shift


def o_ddpm(od, x, ts, tape, kn, kt, *, skw=None, obj=None, guid="standard", init=True):
    """DDPM steps ts (descending) from x; skw None: the default (outside, mean) prediction of sample().  Returns (x, last x_start)."""
    if init:
        x = put(od, x, kn, ts[0], None if kn is None else kt["known_init"])
    for t in ts:
        if obj is None and skw is None:
            x, x_start = O.p_sample_compose_outside(od, x, None, t, tape.step[t], compose_mode="mean", n_composed=0, single_model_step=HZ)
        elif obj is None:
            x, x_start = O.p_sample(od, x, None, t, tape.step[t], pmv_kwargs=pmv_kw(skw))
        else:
            pred, logvar, x_start, _, _ = o_guided_iters(od, x, t, t, tape.recur, kn, kt, obj, guid, pmv_kw(skw))
            x = pred + (0.5 * logvar).exp() * tape.step[t] if t > 0 else pred
        x = put(od, x, kn, t - 1, None if kn is None else kt["known_step"][t])
    return x, x_start


def o_ddim(od, x, steps, tp, kn, kt, *, eta, skw=None, obj=None, guid=None, init=True):
    """DDIM steps [(i, t, t_next)] from x.  Returns (x, last x_start)."""
    if init:
        x = put(od, x, kn, steps[0][1], None if kn is None else kt["known_init"])
    for i, t, tn in steps:
        if obj is None:
            eps, x_start = O.model_predictions(od, x, None, t, clip_x_start=True)
        else:
            _, _, x_start, eps, shift = o_guided_iters(od, x, t, i, tp["recur"], kn, kt, obj, guid, pmv_kw(skw))
            eps = eps + shift
        san, c, sigma = O.ddim_coefs(od, t, tn, eta)
        x = x_start if tn < 0 else x_start * san + c * eps + sigma * tp["step"][i]
        x = put(od, x, kn, tn, None if kn is None else kt["known_step"][i])
    return x, x_start


def pairs(od, S):
    return [(i, t, tn) for i, (t, tn) in enumerate(O.ddim_time_pairs(od.num_timesteps, S))]


def agree(name, out, ref, m, tol):
    """torch.equal on the region, ``tol`` off it (relative to the largest reference value, as rel())."""
    out, off = out.detach().cpu(), ~m
    assert bool(torch.isfinite(out).all()), name
    assert torch.equal(out[m], ref[m]), f"{name}: the region differs"
    assert _say(name, float((out - ref)[off].abs().max() / ref.abs().max())) < tol


def reaches(name, with_region, without, m, tol):
    """Guard: off the region the oracle's result depends on the region by more than 100 x the tolerance in use -- else a wrong
    level on the region could not show there."""
    off = ~m
    v = _say(name + " (region reaches the rest)", float((with_region - without)[off].abs().max() / with_region.abs().max()))
    assert v > 100 * tol, f"{name}: the region does not reach the rest of the state ({v:.2e})"


def unsaturated(name, x_start, m):
    assert float((x_start[~m].abs() < 1.0).float().mean()) > 0.25, f"{name}: the clamp saturates (almost) every element off the region"


def noisy(od, seed, shape, t):
    """A state at level t: q_sample of clean values inside [-1, 1]."""
    g = torch.Generator().manual_seed(7200 + seed)
    return O.q_sample(od, (torch.rand(shape, generator=g) * 2 - 1) * 0.7, t, torch.randn(shape, generator=g))


# ------------------------------------------------------------------ the library's DDPM entries over t0 .. t1 (sample() starts at T - 1)
def lib_ddpm(d, device, x, t0, t1, nt, kn_host, *, skw=None, obj=None, guid="standard", use_graph=True, seed=0, sample_offset=0):
    x = x.to(device).clone()
    full = tuple(x.shape)
    nt = None if nt is None else nt.to(device)
    if skw is None:
        desc = d._desc_for(full, "mean", 0, 4, HZ, 2, outside=True)
    else:
        desc = d._desc_for(full, skw["compose_mode"], skw["n_composed"], skw["compose_start_step"], HZ, skw["compose_n_bodies"])
    iters = max(O._recurrence_times(guid), 1)
    kn = None if kn_host is None else d._known_region(full, kn_host[0], kn_host[1], None, None, nt, t0 + 1, 0 if obj is None else iters)
    karm = d._known_armer(kn, full, nt, device)
    if obj is None:
        return d._run_loop(x, None, desc, t0, t1, noise_steps=None if nt is None else nt.step, seed=seed, sample_offset=sample_offset,
                           inpaint_cond=None, inpaint_noise_steps=None, use_graph=use_graph, karm=karm)
    dz, tables = d._builtin(obj, guid, full[0], full[1], full[2] // 4)
    assert dz is not None
    return d._run_guided_loop(x, None, desc, dz, t0, t1, noise=nt, seed=seed, sample_offset=sample_offset, inpaint_cond=None,
                              initial_state_overwrite=None, use_graph=use_graph, tables=tables, karm=karm)


# ------------------------------------------------------------------ 1. one teacher-forced step
@pytest.mark.parametrize("t", [600, 30, 0])
@pytest.mark.parametrize("guided", [False, True])
def test_one_ddpm_step_vs_oracle(device, unet8, t, guided):
    """cindm_ddpm1d_sample (L = 24, the default prediction) and cindm_ddpm1d_sample_guided (L = 56: three windows, cs = 16,
    mean-inside, standard-recurrence-2) over the one step t: rule 1 at level t, a relaxation at level t, the step to level t - 1.
    t = 0 returns k exactly."""
    m, sd = unet8
    od = O.Diffusion1D(sd, image_size=HZ, conditioned_steps=0)
    d = _ddpm(device, m)
    L = 56 if guided else HZ
    shape = (B, L, 8)
    skw = inside_kw(2, 16) if guided else None
    obj = waypoints(L, 2) if guided else None
    guid = "standard-recurrence-2" if guided else "standard"
    kn, kt = region(L, 8, t), ktape(t, shape, 1000, 2 if guided else 0)
    tape = O.NoiseTape.make(7300 + t, shape, 1000, recur=2 if guided else 0)
    x = noisy(od, t, shape, t)
    ref, x0 = o_ddpm(od, x, [t], tape, kn, kt, skw=skw, obj=obj, guid=guid)
    unsaturated(f"ddpm step t={t}", x0, kn[1])
    if guided:
        _not_degenerate(obj, ref)
    out = lib_ddpm(d, device, x, t, t, nt_ddpm(tape, kt), kn, skw=skw, obj=obj, guid=guid)
    agree(f"ddpm step t={t} guided={guided}", out, ref, kn[1], TOL_STEP)
    if t == 0:
        assert torch.equal(out.cpu()[kn[1]], kn[0][kn[1]])


@pytest.mark.parametrize("i", [0, 2, 3])
@pytest.mark.parametrize("guided", [False, True])
def test_one_ddim_step_vs_oracle(device, unet8, i, guided):
    """cindm_ddpm1d_sample_ddim (F = 8) and cindm_ddpm1d_sample_ddim_guided (F = 16: four bodies composed from the pair model,
    standard-alpha-recurrence-3) over DDIM step i of S = 4: the first from x_T (rule 1), the others from a handed-over state
    (no rule 1), the last one returning k exactly."""
    m, sd = unet8
    S, eta = 4, 0.5
    od = O.Diffusion1D(sd, image_size=HZ, conditioned_steps=0)
    d = _diff(device, m, S, eta)
    F = 16 if guided else 8
    shape = (B, HZ, F)
    skw = inside_kw(0, 4, 4) if guided else None
    obj = waypoints(HZ, 4, time_consistency_coef=0.25) if guided else None
    guid = "standard-alpha-recurrence-3" if guided else None
    R = 3 if guided else 1
    kn, kt = region(HZ, F, 10 + i), ktape(10 + i, shape, S, R)
    tp = _tape(7400 + i, shape, S, R)
    step = pairs(od, S)[i]
    x = tp["init"] if i == 0 else noisy(od, 20 + i, shape, step[1])
    ref, x0 = o_ddim(od, x, [step], tp, kn, kt, eta=eta, skw=skw, obj=obj, guid=guid, init=i == 0)
    if i > 0:                                                            # (t = 999: the clamp saturates x0 whatever the input)
        unsaturated(f"ddim step {i}", x0, kn[1])
    if guided:
        _not_degenerate(obj, ref)
    kw = dict(noise=nt_ddim(tp, kt), known=kn[0], known_mask=kn[1], step_range=(i, i + 1))
    if guided:
        kw.update(design_fn=obj, design_guidance=guid, **skw)
    if i > 0:
        kw["init_img"] = x
    out = d.ddim_sample(shape, None, **kw)
    agree(f"ddim step {i} guided={guided}", out, ref, kn[1], TOL_STEP)
    if i == S - 1:
        assert torch.equal(out.cpu()[kn[1]], kn[0][kn[1]])


# ------------------------------------------------------------------ 2. chain equals loop
def test_plain_ddpm_chain_equals_per_step_calls(device, unet8):
    """Four steps of cindm_ddpm1d_sample with the region inside the captured step against four one-step calls of the same entry
    without a region and known_replace in between: the same kernels, so bit for bit."""
    m, _ = unet8
    d = _ddpm(device, m)
    shape = (B, HZ, 8)
    kn, kt = region(HZ, 8, 30), ktape(30, shape, 1000)
    tape = O.NoiseTape.make(7500, shape, 1000)
    nt = nt_ddpm(tape, kt)
    chain = d.p_sample_loop(shape, None, n_composed=0, noise=nt, known=kn[0], known_mask=kn[1], t_stop=996)
    dev = lambda v: v.to(device)
    x = d.known_replace(dev(tape.init), dev(kn[0]), dev(kn[1]), 999, dev(kt["known_init"]))
    for t in (999, 998, 997, 996):
        x = lib_ddpm(d, device, x, t, t, cindm_amd.NoiseTape(tape.init, tape.step), None)
        x = d.known_replace(x, dev(kn[0]), dev(kn[1]), t - 1, dev(kt["known_step"][t]))
    assert torch.equal(chain, x)
    assert not torch.equal(chain, d.p_sample_loop(shape, None, n_composed=0, noise=nt, t_stop=996))


def test_plain_ddim_chain_equals_per_step_calls(device, unet8):
    m, _ = unet8
    S = 5
    d = _diff(device, m, S, eta=0.7)
    shape = (B, HZ, 8)
    kn, kt = region(HZ, 8, 31), ktape(31, shape, S)
    tp = _tape(7501, shape, S, 1)
    chain = d.ddim_sample(shape, None, noise=nt_ddim(tp, kt), known=kn[0], known_mask=kn[1])
    dev = lambda v: v.to(device)
    times = d.ddim_schedule()[0]
    x = d.known_replace(dev(tp["init"]), dev(kn[0]), dev(kn[1]), times[0], dev(kt["known_init"]))
    for i in range(S):
        x = d.ddim_sample(shape, None, noise=_nt(tp), init_img=x, step_range=(i, i + 1))
        x = d.known_replace(x, dev(kn[0]), dev(kn[1]), times[i + 1], dev(kt["known_step"][i]))
    assert torch.equal(chain, x)
    assert torch.equal(chain.cpu()[kn[1]], kn[0][kn[1]])


GUIDED = {
    # name -> (ddim?, guidance, L, F, sample kwargs, objective)
    "ddpm_r2_three_windows": (False, "standard-recurrence-2", 56, 8, inside_kw(2, 16), lambda: waypoints(56, 2)),
    "ddim_alpha_r3_four_bodies": (True, "standard-alpha-recurrence-3", HZ, 16, inside_kw(0, 4, 4), lambda: waypoints(HZ, 4, time_consistency_coef=0.25)),
    "ddim_r2_resampling_only": (True, "standard-recurrence-2", HZ, 8, inside_kw(), lambda: waypoints(HZ, 2, coef=0.0)),
    "ddpm_r3_resampling_only": (False, "standard-recurrence-3", HZ, 8, inside_kw(), lambda: waypoints(HZ, 2, coef=0.0)),
}


@pytest.mark.parametrize("name", sorted(GUIDED))
def test_guided_chain_equals_generic_route(device, unet8, name):
    """The guided library chains (region, relaxation level and known_recur inside the captured step) against the route that loops
    in Python -- library predictions, autograd on the same callable, known_replace at the same points -- on the same tape: equal on
    the region, the routes' bound (TOL_CHAIN, as test_builtin_route_equals_generic_route) off it.  An objective whose weights are
    all 0 contributes exactly 0: RePaint's resampling alone."""
    ddim, guid, L, F, skw, make = GUIDED[name]
    m, _ = unet8
    obj = make()
    R = int(guid.split("-")[-1])
    shape = (B, L, F)
    kn = region(L, F, 40 + len(name))
    if ddim:
        S = 4
        d = _diff(device, m, S, eta=0.4)
        kt, tp = ktape(40, shape, S, R), _tape(7600 + len(name), shape, S, R)
        kw = dict(noise=nt_ddim(tp, kt))
    else:
        d = _ddpm(device, m)
        kt, tape = ktape(41, shape, 1000, R), O.NoiseTape.make(7601 + len(name), shape, 1000, recur=R)
        kw = dict(noise=nt_ddpm(tape, kt), t_stop=997)
    kw.update(design_guidance=guid, known=kn[0], known_mask=kn[1], **skw)
    # (sample() fixes the DDIM state to [B, image_size, channels]: the four-body state goes through ddim_sample itself)
    run = (lambda **o: d.ddim_sample(shape, None, **o)) if ddim else (lambda **o: d.sample(batch_size=B, **o))
    fast = run(design_fn=obj, **kw)
    slow = run(design_fn=lambda x: obj(x), **kw)
    assert tuple(fast.shape) == shape and bool(torch.isfinite(slow).all())
    if "resampling" not in name:
        _not_degenerate(obj, slow.cpu())
    else:
        assert float(obj(slow.cpu())) == 0.0                             # (the objective is identically 0)
    agree(f"routes {name}", fast, slow.cpu(), kn[1], TOL_CHAIN)
    if ddim:
        assert torch.equal(fast.cpu()[kn[1]], kn[0][kn[1]])
    # the region is held: without it the same tape gives another state
    plain = run(design_fn=obj, **{k: v for k, v in kw.items() if k not in ("known", "known_mask")})
    assert rel(plain, fast) > 100 * TOL_CHAIN


# ------------------------------------------------------------------ 3. short whole chains against the oracle
@pytest.mark.parametrize("T,t_stop", [(6, 0), (8, 2)])
def test_ddpm_chain_vs_oracle(device, unet8, T, t_stop):
    """A whole DDPM chain of six steps down to t = 0 (a diffusion of 6 timesteps) and a truncated one (8 timesteps, t_stop = 2: the
    region ends at level 1 like the rest of the state), through the public p_sample_loop.
    Measured on one MI355X: 8.9e-5 (T = 6) and 8.4e-7 (T = 8) off the region at these tapes against the bound 1e-4; three other
    tapes of the T = 6 chain give 3.2e-6 .. 4.8e-6.  The first step of so short a cosine schedule multiplies the U-Net's rounding
    by sqrt_recip_alphas_cumprod ~ 1e2 on the elements the clamp leaves free, with or without a region: the same chains without one
    sit at 3.5e-6 .. 1.2e-5 (T = 6) and up to 4.6e-5 (T = 4)."""
    m, sd = unet8
    od = O.Diffusion1D(sd, image_size=HZ, conditioned_steps=0, timesteps=T)
    d = _ddpm(device, m, T)
    shape = (B, HZ, 8)
    kn, kt = region(HZ, 8, 50 + T), ktape(50 + T, shape, T)
    tape = O.NoiseTape.make(7700 + T, shape, T)
    ts = list(range(T - 1, t_stop - 1, -1))
    ref, x0 = o_ddpm(od, tape.init, ts, tape, kn, kt)
    bare, _ = o_ddpm(od, tape.init, ts, tape, None, None)
    reaches(f"ddpm T={T}", ref, bare, kn[1], TOL_CHAIN)
    unsaturated(f"ddpm T={T}", x0, kn[1])
    out = d.p_sample_loop(shape, None, n_composed=0, noise=nt_ddpm(tape, kt), known=kn[0], known_mask=kn[1], t_stop=t_stop)
    agree(f"ddpm chain T={T} t_stop={t_stop}", out, ref, kn[1], TOL_CHAIN)
    if t_stop == 0:
        assert torch.equal(out.cpu()[kn[1]], kn[0][kn[1]])
    else:
        assert torch.equal(out.cpu()[kn[1]], put(od, ref, kn, t_stop - 1, kt["known_step"][t_stop])[kn[1]])
        assert not torch.equal(out.cpu()[kn[1]], kn[0][kn[1]])


def test_ddim_chain_vs_oracle(device, unet8):
    """DDIM with S = 4: the last pair has t_next = -1, so the chain returns k on the region."""
    m, sd = unet8
    S, eta = 4, 0.5
    od = O.Diffusion1D(sd, image_size=HZ, conditioned_steps=0)
    d = _diff(device, m, S, eta)
    shape = (B, HZ, 8)
    kn, kt = region(HZ, 8, 60), ktape(60, shape, S)
    tp = _tape(7800, shape, S, 1)
    ref, x0 = o_ddim(od, tp["init"], pairs(od, S), tp, kn, kt, eta=eta)
    bare, _ = o_ddim(od, tp["init"], pairs(od, S), tp, None, None, eta=eta)
    reaches("ddim S=4", ref, bare, kn[1], TOL_CHAIN)
    unsaturated("ddim S=4", x0, kn[1])
    out = d.sample(batch_size=B, noise=nt_ddim(tp, kt), known=kn[0], known_mask=kn[1])
    agree("ddim chain S=4", out, ref, kn[1], TOL_CHAIN)
    assert torch.equal(out.cpu()[kn[1]], kn[0][kn[1]])


# ------------------------------------------------------------------ 4. bitwise properties (counter-based draws)
def test_bitwise_properties_plain(device):
    """Graph == stream, ping-pong on == off, fused update on == off, shared values == the same values per design, two shards with
    sample_offset == the whole batch -- for the plain DDPM and DDIM chains."""
    m, _ = build_unet(device)
    k, msk = region(HZ, 8, 70, batch=4)
    for d in (_ddpm(device, m, 7), _diff(device, m, 5, eta=1.0)):
        run = lambda **o: d.sample(**dict(dict(batch_size=4, n_composed=0, seed=11, known=k, known_mask=msk), **o))
        a = run()
        assert bool(torch.isfinite(a).all()) and torch.equal(a.cpu()[msk], k[msk])
        launches, fused = d.last_step_info()
        assert fused                                                     # a chain with a region still fuses its update
        assert torch.equal(a, run(use_graph=False))
        for opt in ("pingpong", "fuse_update"):
            m.set_option(opt, 0)
            try:
                assert torch.equal(a, run()), opt
                if opt == "fuse_update":
                    assert not d.last_step_info()[1]
            finally:
                m.set_option(opt, 1)
        shared = run(known=k[0], known_mask=msk[1])
        assert torch.equal(shared, run(known=k[:1].expand(4, -1, -1).contiguous(), known_mask=msk[1:2].expand(4, -1, -1).contiguous()))
        parts = [run(batch_size=2, sample_offset=lo, known=k[lo:lo + 2], known_mask=msk[lo:lo + 2]) for lo in (0, 2)]
        assert torch.equal(torch.cat(parts), a)
        assert not torch.equal(a, run(seed=12)) and torch.equal(a.cpu()[msk], run(seed=12).cpu()[msk])


def test_bitwise_properties_guided(device):
    m, _ = build_unet(device)
    k, msk = region(HZ, 8, 71, batch=4)
    obj = waypoints(HZ, 2)
    for d, guid in ((_ddpm(device, m, 6), "standard-recurrence-2"), (_diff(device, m, 3, eta=1.0), "standard-recurrence-3")):
        run = lambda **o: d.sample(**dict(dict(batch_size=4, seed=5, known=k, known_mask=msk, design_fn=obj, design_guidance=guid,
                                               **inside_kw()), **o))
        a = run()
        assert bool(torch.isfinite(a).all()) and torch.equal(a.cpu()[msk], k[msk])
        assert torch.equal(a, run(use_graph=False))
        parts = [run(batch_size=2, sample_offset=lo, known=k[lo:lo + 2], known_mask=msk[lo:lo + 2]) for lo in (0, 2)]
        assert torch.equal(torch.cat(parts), a)
        # the route that loops in Python draws the region's z from the same counter-based generator (its step and relaxation draws
        # are torch.randn there, so the rest of the state differs): after every step the region is bit for bit the chain's
        _, fast = run(return_trajectory_every=1)
        _, slow = run(design_fn=lambda x: obj(x), return_trajectory_every=1)
        assert len(fast) == len(slow) >= 3
        for j in range(len(fast)):
            assert torch.equal(fast.x[j].cpu()[msk], slow.x[j].cpu()[msk]), (guid, j)
        assert not torch.equal(fast.x[0].cpu()[msk], k[msk]) and not torch.equal(fast.x[0], slow.x[0])


def test_everything_known_returns_known(device):
    """A region that is the whole state comes back as ``known`` whatever the weights compute (even inf / nan)."""
    m, _ = build_unet(device, seed=3)
    k = (torch.rand((B, HZ, 8), generator=torch.Generator().manual_seed(72)) * 2 - 1)
    full = torch.ones((HZ, 8), dtype=torch.bool)
    obj = waypoints(HZ, 2)
    assert torch.equal(_ddpm(device, m, 5).sample(batch_size=B, n_composed=0, seed=1, known=k, known_mask=full).cpu(), k)
    assert torch.equal(_diff(device, m, 3).sample(batch_size=B, seed=1, known=k, known_mask=full).cpu(), k)
    assert torch.equal(_diff(device, m, 3).sample(batch_size=B, seed=1, known=k, known_mask=full, design_fn=obj,
                                                  design_guidance="standard-recurrence-2", **inside_kw()).cpu(), k)
    assert torch.equal(_ddpm(device, m, 5).sample(batch_size=B, seed=1, known=k[0], known_mask=full, design_fn=obj,
                                                  design_guidance="standard-recurrence-2", **inside_kw()).cpu(), k[:1].expand(B, -1, -1))


# ------------------------------------------------------------------ 5. nothing armed, and arming consumed
def _null_call(name, h):
    """A chain entry called with the handle and nothing else: every entry takes what is armed before it looks at its arguments."""
    fn = getattr(_ffi.lib(), name)
    args = [h] + [None if a is C.c_void_p or hasattr(a, "contents") or a is C.c_char_p else 0 for a in _ffi.SIGNATURES[name][1][1:]]
    rc = fn(*args)
    return rc, _ffi.lib().cindm_last_error().decode()


def test_nothing_armed_and_arming_is_consumed(device, unet8):
    m, _ = unet8
    d = _ddpm(device, m, 6)
    k, msk = region(HZ, 8, 80)
    run = lambda **o: d.sample(batch_size=B, n_composed=0, seed=9, **o)
    before = run()
    n0, fused0 = d.last_step_info()
    armed = run(known=k, known_mask=msk)
    n1, fused1 = d.last_step_info()
    assert n1 == n0 + 1 and fused1 == fused0 and not torch.equal(armed, before)
    after = run()
    assert d.last_step_info() == (n0, fused0) and torch.equal(after, before)
    fresh = _ddpm(device, m, 6)
    assert torch.equal(fresh.sample(batch_size=B, n_composed=0, seed=9), before)
    # an armed region is consumed by the call that refuses it: the next chain is plain, and the handle works
    h = d._handle()
    kn = d._known_region((B, HZ, 8), k, msk, None, None)
    arm = d._known_armer(kn, (B, HZ, 8), None, device)
    for entry, word in (("cindm_ddpm1d_sample_autoregress", "rollout"), ("cindm_ddpm1d_sample_ula", "Langevin"),
                        ("cindm_ddpm2d_sample", "2-D")):
        arm(h)
        rc, msg = _null_call(entry, h)
        assert rc != 0 and "known region (1-D)" in msg and word in msg and "dropped" in msg, msg
        assert torch.equal(run(), before) and d.last_step_info() == (n0, fused0)
    # a region for another state is refused by the entry that would run it, and dropped
    arm_bad = d._known_armer(d._known_region((B, HZ + 1, 8), torch.zeros((HZ + 1, 8)), torch.ones((HZ + 1, 8), dtype=torch.bool), None, None),
                             (B, HZ + 1, 8), None, device)
    arm_bad(h)
    with pytest.raises(cindm_amd.CindmError, match="made for"):
        d._run_loop(torch.zeros((B, HZ, 8), device=device), None, d._desc_for((B, HZ, 8), "mean", 0, 4, HZ, 2, outside=True), 5, 0,
                    noise_steps=None, seed=9, sample_offset=0, inpaint_cond=None, inpaint_noise_steps=None)
    assert torch.equal(run(), before)
    assert torch.equal(run(known=k, known_mask=msk), armed)


# ------------------------------------------------------------------ 6. recorder
@pytest.mark.parametrize("which", ["ddpm", "ddim", "ddim_guided"])
def test_recorder_records_after_the_overwrite(device, unet8, which):
    m, _ = unet8
    shape = (B, HZ, 8)
    kn = region(HZ, 8, 90)
    dev = lambda v: v.to(device)
    if which == "ddpm":
        T = 6
        d = _ddpm(device, m, T)
        kt, tape = ktape(90, shape, T), O.NoiseTape.make(7900, shape, T)
        out, rec = d.sample(batch_size=B, n_composed=0, noise=nt_ddpm(tape, kt), known=kn[0], known_mask=kn[1],
                            return_trajectory_every=1, trajectory=("x", "x0"))
        levels, rows = [t - 1 for t in rec.t], list(rec.t)
    else:
        S, R = 4, 2
        d = _diff(device, m, S, eta=0.3)
        kt, tp = ktape(91, shape, S, R), _tape(7901, shape, S, R)
        kw = dict(design_fn=waypoints(HZ, 2), design_guidance="standard-recurrence-2", **inside_kw()) if which == "ddim_guided" else {}
        out, rec = d.sample(batch_size=B, noise=nt_ddim(tp, kt), known=kn[0], known_mask=kn[1], return_trajectory_every=1,
                            trajectory=("x", "x0"), **kw)
        times = d.ddim_schedule()[0]
        levels, rows = [times[i + 1] for i in range(S)], list(range(S))
    assert len(rec) == len(levels) and levels[-1] == -1
    for j, (level, row) in enumerate(zip(levels, rows)):
        want = d.known_replace(rec.x[j], dev(kn[0]), dev(kn[1]), level, dev(kt["known_step"][row]))
        assert torch.equal(rec.x[j], want), (which, j)                   # the x stream carries q(k, level, z) on the region
    assert torch.equal(rec.x[-1], out) and torch.equal(out.cpu()[kn[1]], kn[0][kn[1]])
    assert not torch.equal(rec.x0[-1].cpu()[kn[1]], kn[0][kn[1]])        # the x0 stream is the model's prediction, untouched


# ------------------------------------------------------------------ 7. recovery
@pytest.mark.parametrize("guided", [False, True])
def test_exchange_timeout_is_recovered_with_a_region(device, guided):
    """Option dbg = 39 stands in for a partner workgroup kept off the chip (tests/test_gpu_ddim_guided.py's pattern): the chain is
    re-run once from its x_T snapshot on the exchange-free kernels, rule 1 applied again, and equals what that selection computes
    undisturbed."""
    m, _ = build_unet(device)
    m.set_option("auto_range", 0)
    d = _diff(device, m, 4, eta=0.5)
    k, msk = region(HZ, 8, 95, batch=6)
    kw = dict(design_fn=waypoints(HZ, 2), design_guidance="standard-recurrence-2", **inside_kw()) if guided else {}
    run = lambda: d.sample(batch_size=6, seed=3, known=k, known_mask=msk, **kw)
    m.exchange_free(True)
    ref = run().clone()
    m.exchange_free(False)
    assert m.recovered == 0 and not d.last_chain_info()["recovered"]
    m.set_option("dbg", 39)
    try:
        got = run()
        info = d.last_chain_info()
    finally:
        m.set_option("dbg", 0)
    assert info["recovered"] and m.recovered == 1
    assert torch.equal(got, ref) and torch.equal(got.cpu()[msk], k[msk])
