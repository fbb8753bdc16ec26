"""GPU (MI355X): the second-order multistep solver (``solver="dpmpp-2m"``) inside the four DDIM chains
(cindm_ddpm1d_sample_ddim / _sample_ddim_guided, cindm_ddpm2d_sample_ddim / _sample_ddim_force) against its own statement:

    x' = [the DDIM value] + kappa_i (X_i - X_{i-1}),   the difference, the product and the sum rounded once each,

written out in torch on the library's and on the CPU oracle's model_predictions, against the routes that loop in Python, and
against itself (single steps threaded through ``history=``, graph / stream, seeds, batch partition, kappa == 0).

Bounds.  Bitwise (torch.equal) wherever both sides evaluate the same expressions on the same U-Net outputs.  TOL_CHAIN = 1e-4
(tests/test_gpu_parity.py, the project's chain tolerance) against the CPU oracle and between the built-in and the generic-callable
guided 1-D routes, as test_builtin_route_equals_generic_route holds them for DDIM: the two differentiate the objective differently.
The synthetic-weight U-Nets say nothing about convergence (tests/test_multistep_host.py holds the solver's order on an analytic
score); S = 5 and S = 6 exercise the 1-D replay's two-step graph with and without its odd tail."""
import ctypes as C

import pytest
import torch

import cindm_amd
import cindm_oracle as O
import test_ula_host as U
from cindm_amd import _ffi
from test_gpu_parity import TOL_CHAIN, build_unet, rel
from test_gpu_parity_2d import build_unet2d
from test_gpu_quadratic import make_quadratic

pytestmark = pytest.mark.gpu

HZ, B, F = 24, 3, 8
CH, HW, FRAMES = 21, 64, 6
PMIN, PMAX = -37.7, 57.6
MS = dict(solver="dpmpp-2m")
GUID = "standard-recurrence-2"
ONE_WINDOW = dict(n_composed=0, compose_mode="mean-inside", design_guidance=GUID)


def _say(name, v):
    print(f"[multistep] {name}: {v:.3e}")
    return v


@pytest.fixture(scope="module")
def unet8(device):
    return build_unet(device)


@pytest.fixture(scope="module")
def unet2d(device):
    return build_unet2d(device)


@pytest.fixture(scope="module")
def force(device):
    sd = O.synth_state_dict_2d(O.force_unet_param_shapes(), 7)
    m = cindm_amd.ForceUnet(dim=64, dim_mults=(1, 2, 4, 8), channels=4)
    m.load_state_dict(sd, strict=True)
    return m.to(device)


def _diff(device, m, S, eta=0.0):
    return cindm_amd.GaussianDiffusion1D(m, image_size=HZ, conditioned_steps=0, timesteps=1000, sampling_timesteps=S,
                                         loss_type="l1", ddim_sampling_eta=eta).to(device)


def _diff2(device, unet2d, S, **kw):
    kw.setdefault("coeff_ratio", 0.05)
    return cindm_amd.GaussianDiffusion(unet2d[0], image_size=64, frames=FRAMES, cond_frames=2, timesteps=1000, loss_type="l2",
                                       sampling_timesteps=S, **kw).to(device)


def _tape(seed, shape, S, R=2, cond_shape=None):
    g = torch.Generator().manual_seed(seed)
    t = {"init": torch.randn(shape, generator=g), "step": torch.randn((S,) + tuple(shape), generator=g),
         "recur": torch.randn((S, R) + tuple(shape), generator=g)}
    if cond_shape is not None:
        t["cond"] = torch.randn((S,) + tuple(cond_shape), generator=g)
    return t


def _nt(t, **kw):
    return cindm_amd.NoiseTape(t["init"], t["step"], t["recur"], t.get("cond"), **kw)


def _tape2(seed, steps, shape):
    b, nb, c, h, w = shape
    g = torch.Generator().manual_seed(seed)
    init = (torch.randn((b, 1, c - 3, h, w), generator=g), torch.randn((b, nb, 3, h, w), generator=g))
    return cindm_amd.NoiseTape2D(init, torch.randn((steps, b, 1, c - 3, h, w), generator=g),
                                 torch.randn((steps, b, nb, 3, h, w), generator=g))


def _objective(kind, L=HZ):
    if kind == "point":
        return cindm_amd.PointObjective([0.1, 0.2], 2, coef=2.0, time_consistency_coef=0.25)
    return make_quadratic(71, L, F, B, time_consistency_coef=0.25)


def _force_objective(force, b, nb):
    return cindm_amd.ForceObjective(force, b, nb, FRAMES, p_min=PMIN, p_max=PMAX)


def _statement(predict, tp, times, coefs, kappa, dev):
    """The solver's statement in torch: DDIM value left to right, then + kappa * (X - X_prev), every operation its own kernel."""
    img, prev = tp["init"].to(dev), None
    c, k = coefs.to(dev), kappa.to(dev)
    for i, (t, tn) in enumerate(zip(times[:-1], times[1:])):
        eps, x0 = predict(img, t)
        if tn < 0:
            img = x0
        else:
            img = x0 * c[i, 0] + c[i, 1] * eps + c[i, 2] * tp["step"][i].to(dev)
            if float(kappa[i]) != 0.0:
                img = img + k[i] * (x0 - prev)
        prev = x0
    return img


# ------------------------------------------------------------------ 1. the unguided 1-D chain
@pytest.mark.parametrize("S", [5, 6])
def test_unguided_chain_is_the_statement(device, unet8, S):
    m, sd = unet8
    d = _diff(device, m, S)
    shape = (B, HZ, F)
    tp = _tape(8100 + S, shape, S)
    out = d.ddim_sample(shape, None, noise=_nt(tp), **MS)
    launches, fused = d.last_step_info()
    plain = d.ddim_sample(shape, None, noise=_nt(tp))
    launches_ddim, fused_ddim = d.last_step_info()
    # the multistep update is never fused into the U-Net's last kernel: one launch more than the fused DDIM step
    assert fused_ddim and not fused and launches == launches_ddim + 1, (launches, launches_ddim)
    times, coefs = d.ddim_schedule()
    kappa = d.multistep_kappa()
    assert float(kappa[0]) == 0.0 and bool((kappa[1:-1] != 0).all())
    gpu = _statement(lambda x, t: d.model_predictions(x, None, t, clip_x_start=True), tp, times, coefs, kappa, device)
    assert bool(torch.isfinite(out).all()) and torch.equal(out, gpu)
    od = O.Diffusion1D(sd, image_size=HZ, conditioned_steps=0)
    cpu = _statement(lambda x, t: O.model_predictions(od, x, None, t, clip_x_start=True), tp, times, coefs, kappa, "cpu")
    assert _say(f"S={S} chain vs the statement on the oracle", rel(out, cpu)) < TOL_CHAIN
    assert _say(f"S={S} multistep vs ddim", rel(out, plain)) > 100 * TOL_CHAIN        # the term acts


def test_unguided_chain_equals_single_steps_through_history(device, unet8):
    m, _ = unet8
    S = 5
    d = _diff(device, m, S)
    shape = (B, HZ, F)
    tp = _tape(8110, shape, S)
    chain = d.ddim_sample(shape, None, noise=_nt(tp), **MS)
    x, hist = None, None
    for i in range(S):
        x, hist = d.ddim_sample(shape, None, noise=_nt(tp), init_img=x, step_range=(i, i + 1), history=hist, **MS)
    assert torch.equal(chain, x)
    with pytest.raises(ValueError, match="history"):
        d.ddim_sample(shape, None, noise=_nt(tp), init_img=x, step_range=(2, 3), **MS)


# ------------------------------------------------------------------ 2. the guided 1-D chain
@pytest.mark.parametrize("S", [5, 6])
@pytest.mark.parametrize("kind", ["point", "quadratic"])
def test_guided_builtin_route_equals_generic_route(device, unet8, kind, S):
    """One window through the public face (the route that loops in Python applies the term in torch), then two windows with
    compose_start_step = 8 (a state of 32 rows: ddim_sample's state is one window, so the library chain is issued through
    _run_guided_ddim and the generic route is written out here on _guided_step, as ddim_sample's loop does)."""
    m, _ = unet8
    d = _diff(device, m, S)
    shape = (B, HZ, F)
    obj = _objective(kind)
    tp = _tape(8200 + S, shape, S)
    fast = d.ddim_sample(shape, None, design_fn=obj, noise=_nt(tp), **ONE_WINDOW, **MS)
    slow = d.ddim_sample(shape, None, design_fn=lambda x: obj(x), noise=_nt(tp), **ONE_WINDOW, **MS)
    plain = d.ddim_sample(shape, None, design_fn=obj, noise=_nt(tp), **ONE_WINDOW)
    assert bool(torch.isfinite(slow).all())
    assert _say(f"{kind} S={S} routes, one window", rel(fast, slow)) < TOL_CHAIN
    assert _say(f"{kind} S={S} multistep vs ddim", rel(fast, plain)) > 100 * TOL_CHAIN

    L2 = HZ + 8
    full = (B, L2, F)
    obj2 = _objective(kind, L2)
    tp2 = _tape(8250 + S, full, S)
    times, coefs = d.ddim_schedule()
    desc = d._desc_for(full, "mean-inside", 1, 8, HZ, 2, clip=True)
    dz, tables = d._builtin(obj2, GUID, B, L2, 2)
    assert dz is not None and dz.recurrence == 2
    img = tp2["init"].to(device).clone()
    ms = d._multistep(True, 0, S, None, img)
    fast2 = d._run_guided_ddim(img, None, desc, dz, times, coefs, noise=_nt(tp2).to(device), seed=0, sample_offset=0, inpaint_cond=None,
                               initial_state_overwrite=None, tables=tables, ms=ms)
    kappa, c = d.multistep_kappa(), coefs.to(device)
    x, prev = tp2["init"].to(device), None
    for i, (t, tn) in enumerate(zip(times[:-1], times[1:])):
        eps, x0 = d._guided_step(x, None, t, desc, lambda v: obj2(v), GUID, None, None, tp2["recur"][i].to(device), ddim_return=True)
        if tn < 0:
            x = x0
        else:
            x = x0 * c[i, 0] + c[i, 1] * eps + c[i, 2] * tp2["step"][i].to(device)
            if float(kappa[i]) != 0.0:
                x = x + kappa[i].to(device) * (x0 - prev)
        prev = x0
    assert tuple(fast2.shape) == full and bool(torch.isfinite(x).all())
    assert _say(f"{kind} S={S} routes, two windows", rel(fast2, x)) < TOL_CHAIN
    assert _say(f"{kind} S={S} history vs the last x_start", rel(ms[1], prev)) < TOL_CHAIN


# ------------------------------------------------------------------ 3. the 2-D chains
def test_2d_unguided_chain_equals_single_steps_through_history(device, unet2d):
    shape = (1, 2, CH, HW, HW)
    S = 4
    d = _diff2(device, unet2d, S)
    tape = _tape2(8300, S, shape)
    chain = d.ddim_sample(shape, noise=tape, **MS)
    plain = d.ddim_sample(shape, noise=tape)
    x, hist = None, None
    for i in range(S):
        x, hist = d.ddim_sample(shape, noise=tape, init_img=x, step_range=(i, i + 1), history=hist, **MS)
        assert tuple(hist.shape) == shape
    assert bool(torch.isfinite(chain).all()) and torch.equal(chain, x)
    assert _say("2-D multistep vs ddim", rel(chain, plain)) > 100 * TOL_CHAIN
    # the history a segment hands back is the x_start of its last step: on the last pair, the state itself
    assert torch.equal(hist, chain)


def test_2d_force_guided_chain_equals_the_python_loop(device, unet2d, force):
    """The guided multistep kernel (term, then shift, in one pass) against ``fused=False``: the objective, one plain DDIM step of the
    library, the term in torch on model_predictions' x_start, the shift in torch."""
    shape = (1, 2, CH, HW, HW)
    S = 4
    d = _diff2(device, unet2d, S)
    fn = _force_objective(force, 1, 2)
    tape = _tape2(8310, S, shape)
    kw = dict(design_fn=fn, design_guidance="standard-alpha", noise=tape)
    fused = d.ddim_sample(shape, **kw, **MS)
    loop = d.ddim_sample(shape, fused=False, **kw, **MS)
    plain = d.ddim_sample(shape, **kw)
    _say("2-D guided fused vs loop", rel(fused, loop))
    _say("2-D guided multistep vs ddim", rel(fused, plain))
    assert bool(torch.isfinite(fused).all()) and torch.equal(fused, loop)
    assert rel(fused, plain) > 100 * TOL_CHAIN


# ------------------------------------------------------------------ 4. kappa == 0 is the DDIM chain
def test_zero_kappa_is_the_ddim_chain_on_all_four_entries(device, unet8, unet2d, force, monkeypatch):
    from cindm_amd import diffusion_base
    real = diffusion_base.multistep_kappa
    monkeypatch.setattr(diffusion_base, "multistep_kappa", lambda d: torch.zeros_like(real(d)))
    m, _ = unet8
    for S in (5, 6):
        d = _diff(device, m, S)
        assert not bool(d.multistep_kappa().any())
        shape = (B, HZ, F)
        assert torch.equal(d.ddim_sample(shape, None, seed=3, **MS), d.ddim_sample(shape, None, seed=3))
        kw = dict(design_fn=_objective("point"), seed=3, **ONE_WINDOW)
        assert torch.equal(d.ddim_sample(shape, None, **kw, **MS), d.ddim_sample(shape, None, **kw))
    shape2 = (1, 2, CH, HW, HW)
    d2 = _diff2(device, unet2d, 4)
    assert torch.equal(d2.ddim_sample(shape2, seed=3, **MS), d2.ddim_sample(shape2, seed=3))
    kw = dict(design_fn=_force_objective(force, 1, 2), design_guidance="standard-alpha", seed=3)
    assert torch.equal(d2.ddim_sample(shape2, **kw, **MS), d2.ddim_sample(shape2, **kw))


# ------------------------------------------------------------------ 5. the armed state does not leak
def test_ddim_after_a_multistep_call_is_a_fresh_handles_ddim(device, unet8, unet2d):
    m, _ = unet8
    shape = (B, HZ, F)
    kw = dict(design_fn=_objective("point"), seed=5, **ONE_WINDOW)
    used, fresh = _diff(device, m, 5), _diff(device, m, 5)
    a = used.ddim_sample(shape, None, seed=5, **MS)
    b = used.ddim_sample(shape, None, seed=5)
    g1 = used.ddim_sample(shape, None, **kw, **MS)
    g2 = used.ddim_sample(shape, None, **kw)
    assert torch.equal(b, fresh.ddim_sample(shape, None, seed=5)) and not torch.equal(a, b)
    assert torch.equal(g2, fresh.ddim_sample(shape, None, **kw)) and not torch.equal(g1, g2)
    assert used.last_step_info()[0] == fresh.last_step_info()[0]
    shape2 = (1, 2, CH, HW, HW)
    used2, fresh2 = _diff2(device, unet2d, 4), _diff2(device, unet2d, 4)
    a = used2.ddim_sample(shape2, seed=5, **MS)
    b = used2.ddim_sample(shape2, seed=5)
    assert torch.equal(b, fresh2.ddim_sample(shape2, seed=5)) and not torch.equal(a, b)


# ------------------------------------------------------------------ 6. / 7. graph, seeds, batch partition
@pytest.mark.parametrize("S", [5, 6])
def test_bitwise_properties_1d(device, unet8, S):
    m, _ = unet8
    d = _diff(device, m, S)
    for extra in ({}, dict(design_fn=_objective("point"), **ONE_WINDOW)):
        run = lambda b=B, **kw: d.ddim_sample((b, HZ, F), None, **{"seed": 11, **extra, **MS, **kw})
        a = run()
        assert bool(torch.isfinite(a).all())
        assert torch.equal(a, run(use_graph=False))
        assert torch.equal(a, run()) and not torch.equal(a, run(seed=12))
        assert torch.equal(a, torch.cat([run(1, sample_offset=0), run(2, sample_offset=1)]))
        assert float(a.abs().max()) <= 1.0 + 1e-5            # the last pair returns the clamped x_start


def test_bitwise_properties_2d(device, unet2d):
    d = _diff2(device, unet2d, 4)
    run = lambda b=2, **kw: d.ddim_sample((b, 2, CH, HW, HW), **{"seed": 11, **MS, **kw})
    a = run()
    assert bool(torch.isfinite(a).all())
    assert torch.equal(a, run(use_graph=False))
    assert torch.equal(a, run()) and not torch.equal(a, run(seed=12))
    assert torch.equal(a, torch.cat([run(1, sample_offset=0), run(1, sample_offset=1)]))


def test_sharded_samplers_forward_the_solver(device, unet8, unet2d):
    """dist.sample_sharded / sample2d_sharded (a world of one) pass ``solver=`` on; a rank's chain owns its history."""
    from cindm_amd import dist as cdist
    m, _ = unet8
    d = _diff(device, m, 5)
    whole = d.sample(batch_size=B, seed=21, **MS)
    assert torch.equal(cdist.sample_sharded(d, B, seed=21, **MS), whole)
    assert not torch.equal(cdist.sample_sharded(d, B, seed=21), whole)
    d2 = _diff2(device, unet2d, 4)
    whole2 = d2.sample(batch_size=1, num_boundaries=2, seed=21, **MS)
    assert torch.equal(cdist.sample2d_sharded(d2, 1, seed=21, num_boundaries=2, **MS), whole2)


# ------------------------------------------------------------------ 8. with a recorder, a known region, inpainting
@pytest.mark.parametrize("what", ["recorder", "known", "inpaint"])
def test_guided_1d_with_what_follows_the_update(device, unet8, what):
    """The term comes ahead of the inpainting overwrite, the known-region node and the recorder: the library chain against the
    route that loops in Python, which applies them in that order."""
    m, _ = unet8
    S = 5
    d = _diff(device, m, S)
    shape = (B, HZ, F)
    obj = _objective("point")
    cond = None
    extra, tkw = {}, {}
    g = torch.Generator().manual_seed(8800)
    if what == "recorder":
        extra = dict(return_trajectory_every=2, trajectory=("x", "x0"))
    elif what == "known":
        k = (torch.rand(shape, generator=g) * 2 - 1) * 0.8
        mask = torch.zeros(shape, dtype=torch.bool)
        mask[:, 0, :] = True
        mask[:, HZ // 2, 4:8] = True
        extra = dict(known=k, known_mask=mask)
        tkw = dict(known_init=torch.randn(shape, generator=g), known_step=torch.randn((S,) + shape, generator=g),
                   known_recur=torch.randn((S, 2) + shape, generator=g))
    else:
        cond = (torch.rand((B, 4, F), generator=g) * 2 - 1).to(device)
    tp = _tape(8801, shape, S, cond_shape=None if cond is None else tuple(cond.shape))
    run = lambda fn, **kw: d.ddim_sample(shape, cond, design_fn=fn, noise=_nt(tp, **tkw), **ONE_WINDOW, **extra, **kw)
    fast, slow, plain = run(obj, **MS), run(lambda x: obj(x), **MS), run(obj)
    if what == "recorder":
        (fast, frec), (slow, srec), (plain, _) = fast, slow, plain
        assert frec.step == srec.step == [2, 4, 5]
        assert _say("recorded x", rel(frec.x, srec.x)) < TOL_CHAIN and _say("recorded x0", rel(frec.x0, srec.x0)) < TOL_CHAIN
        assert torch.equal(frec.x[-1].to(device), fast)
    assert _say(f"routes with {what}", rel(fast, slow)) < TOL_CHAIN
    assert rel(fast, plain) > 100 * TOL_CHAIN
    if what == "known":
        assert torch.equal(fast.cpu()[mask], k[mask])


def test_2d_with_a_recorder_and_a_known_region(device, unet2d, force):
    """fused against ``fused=False`` with replacement conditioning (``cond=``) and a recorder; the bound of the DDIM twin
    (test_guided_ddim2d_fused_equals_loop_equals_eager: 1e-6)."""
    shape = (1, 2, CH, HW, HW)
    d = _diff2(device, unet2d, 4)
    g = torch.Generator().manual_seed(8810)
    cond = torch.rand((1, 6, HW, HW), generator=g) * 2 - 1
    kw = dict(design_fn=_force_objective(force, 1, 2), design_guidance="standard-alpha", seed=9, cond=cond, return_trajectory_every=2, **MS)
    fused, frec = d.ddim_sample(shape, **kw)
    loop, lrec = d.ddim_sample(shape, fused=False, **kw)
    assert frec.step == lrec.step == [2, 4]
    assert _say("2-D routes with region and recorder", rel(fused, loop)) < 1e-6
    assert _say("2-D recorded x", rel(frec.x, lrec.x)) < 1e-6
    assert torch.equal(fused[:, :, :6].cpu(), cond[:, None].expand(-1, 2, -1, -1, -1))


# ------------------------------------------------------------------ 9. every other entry refuses an armed solver
def _armed_refusal(d, run, numel, device):
    """Arms the handle directly, issues ``run`` (a chain entry that does not run the solver): it must fail with the solver's
    message, and the same call must pass afterwards -- the refused call consumed the solver."""
    L = _ffi.lib()
    kappa = (C.c_float * 3)(0.0, 0.1, 0.0)
    hist = torch.empty(numel, dtype=torch.float32, device=device)
    _ffi.check(L.cindm_ddpm1d_set_multistep(d._handle(), kappa, 3, _ffi.ptr(hist), numel))
    with pytest.raises(cindm_amd.CindmError, match="multistep solver"):
        run()
    out = run()
    out = out[0] if isinstance(out, tuple) else out
    assert bool(torch.isfinite(out).all())


def test_other_1d_entries_refuse_an_armed_solver(device, unet8):
    m, _ = unet8
    d = _diff(device, m, 1000)
    n = 2 * HZ * F
    _armed_refusal(d, lambda: d.sample(batch_size=2, seed=1, t_stop=998), n, device)                       # cindm_ddpm1d_sample
    _armed_refusal(d, lambda: d.sample(batch_size=2, seed=1, t_stop=998, design_fn=_objective("point"),   # _sample_guided
                                       **ONE_WINDOW), n, device)
    mh, _ = build_unet(device, 8, 8)
    dh = cindm_amd.GaussianDiffusion1D(mh, image_size=4, conditioned_steps=4, timesteps=1000, sampling_timesteps=3,
                                       loss_type="l1").to(device)
    cond = (torch.rand((2, 4, 8), generator=torch.Generator().manual_seed(1)) - 0.5).to(device)
    _armed_refusal(dh, lambda: dh.autoregress_time_compose_sample(2, cond, 1, seed=1), n, device)         # _sample_autoregress
    _armed_refusal(dh, lambda: dh.composing_time_sample((2, 4, 8), cond, n_composed=1, seed=1), n, device)   # _sample_timecompose
    m8, m4 = build_unet(device, U.HZ, 8)[0], build_unet(device, U.HZ, 4)[0]
    N = 1000
    du = cindm_amd.GaussianDiffusion1D(m8, image_size=U.R, conditioned_steps=U.LC, timesteps=1000, sampling_timesteps=1000,
                                       loss_type="l1", betas_inference=U.linear_beta_schedule(N)).to(device)
    du.model_unconditioned = m4
    x = torch.randn((2, U.HZ, U.F), generator=torch.Generator().manual_seed(2)).to(device)
    scalar = U.scalar_for_gradient(U.linear_beta_schedule(N))
    _armed_refusal(du, lambda: du.sample_step_ULA(x, torch.tensor([731, 731]), 1, 4, N, scalar, seed=1), n, device)   # _sample_ula


def test_other_2d_entries_refuse_an_armed_solver(device, unet2d, force):
    shape = (1, 2, CH, HW, HW)
    d = _diff2(device, unet2d, 1000)
    n = 2 * HW * HW * 24
    _armed_refusal(d, lambda: d.p_sample_loop(shape, seed=1, t_stop=998), n, device)                      # cindm_ddpm2d_sample
    fn = _force_objective(force, 1, 2)
    _armed_refusal(d, lambda: d.p_sample_loop(shape, fn, "standard-alpha", seed=1, t_stop=998), n, device)   # _sample_force


def test_device_checks_of_the_four_entries(device, unet8):
    """n_steps against the call and hist_floats against the state, through the ABI."""
    m, _ = unet8
    d = _diff(device, m, 5)
    L = _ffi.lib()
    shape = (B, HZ, F)
    hist = torch.empty(B * HZ * F, dtype=torch.float32, device=device)
    k3, k5 = (C.c_float * 3)(0.0, 0.1, 0.0), (C.c_float * 5)(0.0, 0.1, 0.1, 0.1, 0.0)
    _ffi.check(L.cindm_ddpm1d_set_multistep(d._handle(), k3, 3, _ffi.ptr(hist), hist.numel()))
    with pytest.raises(cindm_amd.CindmError, match="armed for 3 steps"):
        d.ddim_sample(shape, None, seed=1)
    _ffi.check(L.cindm_ddpm1d_set_multistep(d._handle(), k5, 5, _ffi.ptr(hist), hist.numel() - 4))
    with pytest.raises(cindm_amd.CindmError, match="history holds"):
        d.ddim_sample(shape, None, seed=1)
    ref = d.ddim_sample(shape, None, seed=1)                  # both refusals consumed the solver: this is the plain chain
    assert torch.equal(ref, _diff(device, m, 5).ddim_sample(shape, None, seed=1))
    de = _diff(device, m, 5, eta=0.5)
    _ffi.check(L.cindm_ddpm1d_set_multistep(de._handle(), k5, 5, _ffi.ptr(hist), hist.numel()))
    with pytest.raises(cindm_amd.CindmError, match="sigma"):
        de.ddim_sample(shape, None, seed=1)
