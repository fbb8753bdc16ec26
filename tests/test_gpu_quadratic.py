"""GPU (MI355X): the quadratic objective (cindm_amd.QuadraticObjective) inside the two captured guided chains
(cindm_ddpm1d_sample_guided / _sample_ddim_guided with descriptor mode 5, cindm_ddpm1d_set_design_quadratic, compose_update_quad_kernel).

Expectations come from oracle/cindm_oracle.py on the CPU at test time, differentiating the SAME callable with autograd where the update
kernel evaluates the closed form from its two device tables.  Tolerances: tests/test_gpu_parity.py's TOL_STEP on single guided steps
and TOL_CHAIN on short whole chains.

Tables (``make_quadratic``): terms on rows 0, 3, L // 3, L // 2 and L - 1 only; each such row gets three residuals a^T x - r with a
dense unit-norm a over all F features (velocities and cross-body couplings carry weight), r in [-0.6, 0.6] and weight (0.5 .. 1.5) *
scale; the third residual is negated and quartered on alternating rows ("keep apart": S is indefinite there); another pattern per
design.  scale = 0.3 for every chain and every recurrence case (eigenvalues of S inside about [-0.11, 0.66]; at scale 1 the DDPM chain
runs away to 6e2 in the oracle), 20 for the single steps without recurrence, where the gradient then dominates the step.  Every case
here was run through the oracle on the CPU first; every chain case asserts ``_not_degenerate``, max |ref| < 100 (far inside the
split-fp16 window) and that the objective moved the oracle's result by more than 100 * TOL_CHAIN against the zero-objective chain."""
import pytest
import torch

import cindm_amd
import cindm_oracle as O
from cindm_amd import _ffi
from cindm_amd import dist as cdist
from test_gpu_ddim_guided import _not_degenerate, _nt, _tape
from test_gpu_parity import TOL_CHAIN, TOL_STEP, build_unet, rel
from test_gpu_waypoint import make_tables

pytestmark = pytest.mark.gpu

HZ = 24
Q = cindm_amd.QuadraticObjective


def _say(name, v):
    print(f"[quadratic] {name}: {v:.3e}")
    return v


@pytest.fixture(scope="module")
def unet8(device):
    return build_unet(device)


@pytest.fixture(scope="module")
def diff8(device, unet8):
    return cindm_amd.GaussianDiffusion1D(unet8[0], image_size=HZ, conditioned_steps=0, timesteps=1000, sampling_timesteps=1000,
                                         loss_type="l1").to(device)


def _ddim(device, m, S, eta=0.0):
    return cindm_amd.GaussianDiffusion1D(m, image_size=HZ, conditioned_steps=0, timesteps=1000, sampling_timesteps=S,
                                         loss_type="l1", ddim_sampling_eta=eta).to(device)


def quad_tables(seed, L, F, B, scale):
    """(S [B, L, F, F], h [B, L, F]) of the recipe in the module docstring, per design."""
    g = torch.Generator().manual_seed(seed)
    rows = [0, 3, L // 3, L // 2, L - 1]
    ridx = torch.tensor([r for r in rows for _ in range(3)])
    M = ridx.numel()
    A = torch.randn((B, M, F), generator=g, dtype=torch.float64)
    A = A / A.norm(dim=-1, keepdim=True)
    r = torch.rand((B, M), generator=g, dtype=torch.float64) * 1.2 - 0.6
    w = (torch.rand((B, M), generator=g, dtype=torch.float64) + 0.5) * scale
    for b in range(B):
        for k in range(len(rows)):
            if (k + b) % 2 == 0:
                w[b, 3 * k + 2] *= -0.25
    o = Q.from_residuals(ridx, A, r, w, L, F)
    assert B == 1 or not torch.equal(o.S[0], o.S[1])
    free = [l for l in range(L) if l not in rows]
    assert float(o.S[:, free].abs().max()) == 0.0 and float(o.h[:, free].abs().max()) == 0.0
    assert float(torch.linalg.eigvalsh(o.S[:, rows].double()).min()) < 0.0          # the negated residuals show
    return o.S, o.h


def make_quadratic(seed, L, F, B, per_S=True, per_h=True, scale=0.3, cls=Q, **kw):
    S, h = quad_tables(seed, L, F, B, scale)
    return cls((S if per_S else S[0]).contiguous(), (h if per_h else h[0]).contiguous(), **kw)


def zero_objective(L, F, **kw):
    return Q(torch.zeros((L, F, F)), torch.zeros((L, F)), **kw)


class _NeverCalled(Q):
    def __call__(self, pos):
        raise AssertionError("the built-in route evaluated the objective in Python")


def _moved(name, obj, ref, ref0):
    """The guards of a chain case, on the oracle's result ``ref`` and its zero-objective result ``ref0``."""
    _not_degenerate(obj, ref)
    assert float(ref.abs().max()) < 100.0
    assert _say(f"{name}: objective moved the oracle's result by", rel(ref, ref0)) > 100 * TOL_CHAIN


# ------------------------------------------------------------------ 1. one guided step against the oracle
# (guidance, tc, S per design, h per design, initial_state_overwrite, scale): both guidances with and without recurrence, each of the
# four per-design combinations twice, tc and the overwrite in half of the cases each
STEP_CASES = [("standard", 0.0, False, False, False, 20.0), ("standard", 0.5, True, True, True, 20.0),
              ("standard-alpha", 0.5, True, False, False, 20.0), ("standard-alpha", 0.0, False, True, True, 20.0),
              ("standard-recurrence-2", 0.5, False, False, True, 0.3), ("standard-recurrence-2", 0.0, False, True, False, 0.3),
              ("standard-alpha-recurrence-3", 0.0, True, True, True, 0.3), ("standard-alpha-recurrence-3", 0.5, True, False, False, 0.3)]
STEP_B, STEP_L, STEP_F = 2, 56, 8
STEP_KW = dict(compose_mode="mean-inside", n_composed=2, compose_start_step=16, single_model_step=HZ, compose_n_bodies=2)


def step_inputs(guid, use_iso):
    """[(t, x, step noise, relaxation noise, overwrite)] of a step case: t = 600, 30, 0."""
    R = int(guid.split("-")[-1]) if "recurrence" in guid else 0
    g = torch.Generator().manual_seed(21)
    shape = (STEP_B, STEP_L, STEP_F)
    out = []
    for t in (600, 30, 0):
        x = torch.randn(shape, generator=g) * 0.7
        nz = torch.randn(shape, generator=g)
        rn = torch.randn((max(R, 1),) + shape, generator=g)
        iso = torch.randn((STEP_B, 4, STEP_F), generator=g) * 0.3 if use_iso else None
        out.append((t, x, nz, rn, iso))
    return R, out


def step_refs(od, guid, tc, per_S, per_h, use_iso, scale):
    """[(reference, unguided reference where the case compares with it)] of a step case, from the oracle."""
    R = step_inputs(guid, use_iso)[0]
    plain = make_quadratic(11, STEP_L, STEP_F, STEP_B, per_S, per_h, scale, time_consistency_coef=tc)
    refs = []
    for t, x, nz, rn, iso in step_inputs(guid, use_iso)[1]:
        ref, _ = O.p_sample_compose_inside(od, x.clone(), None, t, nz, design_fn=plain, design_guidance=guid, recur_noise=rn,
                                           initial_state_overwrite=iso, **STEP_KW)
        ung = None
        if R == 0 and t == 600:
            ung, _ = O.p_sample_compose_inside(od, x.clone(), None, t, nz, design_guidance=guid, initial_state_overwrite=iso, **STEP_KW)
        refs.append((ref, ung))
    return refs


@pytest.mark.parametrize("guid,tc,per_S,per_h,use_iso,scale", STEP_CASES)
def test_step_vs_oracle(device, unet8, diff8, guid, tc, per_S, per_h, use_iso, scale):
    """One guided reverse step (3 windows, mean-inside, L_tot = 56) at t = 600, 30, 0; the overwrite covers rows 0 .. 3, which carry
    terms (rows 0 and 3)."""
    _, sd = unet8
    B, L, F = STEP_B, STEP_L, STEP_F
    od = O.Diffusion1D(sd, image_size=HZ, conditioned_steps=0)
    obj = make_quadratic(11, L, F, B, per_S, per_h, scale, cls=_NeverCalled, time_consistency_coef=tc)
    R, inputs = step_inputs(guid, use_iso)
    refs = step_refs(od, guid, tc, per_S, per_h, use_iso, scale)
    desc = diff8._desc_for((B, L, F), "mean-inside", 2, 16, HZ, 2)
    for (t, x, nz, rn, iso), (ref, unguided) in zip(inputs, refs):
        assert bool(torch.isfinite(ref).all())
        if R == 0 and t == 600:           # the gradient moves the step by far more than the tolerance
            assert _say(f"step {guid} t={t}: gradient moved the step by", rel(unguided, ref)) > 100 * TOL_STEP
        step = torch.zeros((1000, B, L, F)); step[t] = nz
        rec = torch.zeros((1000, max(R, 1), B, L, F)); rec[t] = rn
        tape = cindm_amd.NoiseTape(None, step, rec).to(device)
        out = diff8._run_guided_loop(x.clone().to(device), None, desc, obj.descriptor(guid), t, t, noise=tape, seed=0, sample_offset=0,
                                     inpaint_cond=None, initial_state_overwrite=None if iso is None else iso.to(device), tables=obj)
        assert _say(f"step {guid} tc={tc} t={t}", rel(out, ref)) < TOL_STEP, (guid, t)


# ------------------------------------------------------------------ 2. short whole chains against the oracle
DDPM_KW = dict(n_composed=1, compose_start_step=16, compose_mode="mean-inside", design_guidance="standard-recurrence-2", t_stop=985)


def ddpm_case():
    """t = 999 .. 985, B = 3, one composed window more (L_tot = 40, cs = 16), per-design tables, tc = 0.25."""
    B, L = 3, 40
    tape = O.NoiseTape.make(92, (B, L, 8), 1000, recur=2)
    return B, L, (31, L, 8, B), dict(time_consistency_coef=0.25), tape


def test_ddpm_chain_vs_oracle(device, unet8, diff8):
    _, sd = unet8
    B, L, targs, okw, tape = ddpm_case()
    obj, plain = make_quadratic(*targs, cls=_NeverCalled, **okw), make_quadratic(*targs, **okw)
    od = O.Diffusion1D(sd, image_size=HZ, conditioned_steps=0)
    ref = O.sample(od, B, tape, design_fn=plain, **DDPM_KW)
    _moved("ddpm chain", plain, ref, O.sample(od, B, tape, design_fn=zero_objective(L, 8, **okw), **DDPM_KW))
    out = diff8.sample(batch_size=B, design_fn=obj, noise=cindm_amd.NoiseTape(tape.init, tape.step, tape.recur), **DDPM_KW)
    assert tuple(out.shape) == (B, L, 8)
    assert _say("ddpm chain vs oracle", rel(out, ref)) < TOL_CHAIN


# name -> (eta, guidance, n_bodies, tc, S per design, h per design, iso rows, inpaint rows)
DDIM_CASES = {
    "nb2": (0.0, "standard-recurrence-2", 2, 0.0, True, True, 0, 0),
    "nb4": (0.0, "standard-recurrence-2", 4, 0.0, True, True, 0, 0),
    "nb2_alpha_r1": (0.3, "standard-alpha-recurrence-1", 2, 0.0, False, True, 0, 0),
    "nb2_iso": (0.0, "standard-recurrence-2", 2, 0.5, True, False, 3, 0),
    "nb2_inpaint": (0.5, "standard-recurrence-2", 2, 0.0, True, True, 0, 4),
}


def ddim_case(name):
    """(S, eta, shape, table arguments, objective kwargs, sample kwargs, tape, cond, iso) of a DDIM chain case: S = 10, B = 2, L = 24."""
    eta, guid, nb, tc, per_S, per_h, iso_rows, inp_rows = DDIM_CASES[name]
    S, B, R, F = 10, 2, int(guid.split("-")[-1]), 4 * nb
    shape = (B, HZ, F)
    g = torch.Generator().manual_seed(600 + len(name))
    iso = torch.randn((B, iso_rows, F), generator=g) * 0.3 if iso_rows else None
    cond = torch.rand((B, inp_rows, F), generator=g) * 2 - 1 if inp_rows else None
    tp = _tape(6100 + len(name), shape, S, R, None if cond is None else tuple(cond.shape))
    kw = dict(n_composed=0, compose_mode="mean-inside", design_guidance=guid, **({"compose_n_bodies": 4} if nb == 4 else {}))
    return S, eta, shape, (41 + nb, HZ, F, B, per_S, per_h), dict(time_consistency_coef=tc), kw, tp, cond, iso


def ddim_refs(od, name):
    """(objective, oracle result, zero-objective oracle result) of a DDIM chain case."""
    S, eta, shape, targs, okw, kw, tp, cond, iso = ddim_case(name)
    plain = make_quadratic(*targs, **okw)
    run = lambda fn: O.ddim_sample(od, shape, cond, tp, sampling_timesteps=S, eta=eta, design_fn=fn, initial_state_overwrite=iso, **kw)
    return plain, run(plain), run(zero_objective(HZ, shape[2], **okw))


@pytest.mark.parametrize("name", sorted(DDIM_CASES))
def test_ddim_chain_vs_oracle(device, unet8, name):
    S, eta, shape, targs, okw, kw, tp, cond, iso = ddim_case(name)
    m, sd = unet8
    obj = make_quadratic(*targs, cls=_NeverCalled, **okw)
    plain, ref, ref0 = ddim_refs(O.Diffusion1D(sd, image_size=HZ, conditioned_steps=0), name)
    _moved(f"ddim {name}", plain, ref, ref0)
    d = _ddim(device, m, S, eta)
    dev = lambda t: None if t is None else t.to(device)
    out = d.ddim_sample(shape, dev(cond), design_fn=obj, initial_state_overwrite=dev(iso), noise=_nt(tp), **kw)
    assert tuple(out.shape) == shape
    assert _say(f"ddim {name} vs oracle", rel(out, ref)) < TOL_CHAIN


# ------------------------------------------------------------------ 3. velocities and couplings really act
VEL_ROWS = [0, 3, HZ // 3, HZ // 2, HZ - 1]


def velocity_coupling_objective(cls=Q):
    """S touches only the velocity features (2, 3 of every body: a pull of the velocity to a target, "arrive and stop" with target 0 on
    the last row) and the position block between bodies 0 and 1 (a pure coupling x_0 . x_1: no position diagonal)."""
    F = 8
    S, h = torch.zeros((HZ, F, F)), torch.zeros((HZ, F))
    g = torch.Generator().manual_seed(77)
    for l in VEL_ROWS:
        for j in range(2):
            S[l, 4 * j + 2, 4 * j + 2] = S[l, 4 * j + 3, 4 * j + 3] = 0.6
            h[l, 4 * j + 2:4 * j + 4] = 0.0 if l == HZ - 1 else 0.6 * (torch.rand((2,), generator=g) * 1.2 - 0.6)
        S[l, 0, 4] = S[l, 4, 0] = S[l, 1, 5] = S[l, 5, 1] = 0.3
    return cls(S, h)


VEL_KW = dict(n_composed=0, compose_mode="mean-inside", design_guidance="standard-recurrence-2")


def velocity_refs(od):
    shape = (2, HZ, 8)
    tp = _tape(6200, shape, 10, 2)
    plain = velocity_coupling_objective()
    run = lambda fn: O.ddim_sample(od, shape, None, tp, sampling_timesteps=10, eta=0.0, design_fn=fn, **VEL_KW)
    return shape, tp, plain, run(plain), run(zero_objective(HZ, 8))


def test_velocities_and_couplings_act(device, unet8):
    m, sd = unet8
    shape, tp, plain, ref, ref0 = velocity_refs(O.Diffusion1D(sd, image_size=HZ, conditioned_steps=0))
    _moved("velocity / coupling", plain, ref, ref0)
    d = _ddim(device, m, 10)
    out = d.ddim_sample(shape, None, design_fn=velocity_coupling_objective(_NeverCalled), noise=_nt(tp), **VEL_KW).cpu()
    out0 = d.ddim_sample(shape, None, design_fn=zero_objective(HZ, 8), noise=_nt(tp), **VEL_KW).cpu()
    vel, pos = [2, 3, 6, 7], [0, 1, 4, 5]
    for name, ch in (("velocities", vel), ("coupled positions", pos)):
        a, a0 = out[:, VEL_ROWS][..., ch], out0[:, VEL_ROWS][..., ch]
        assert _say(f"{name} moved by", float((a - a0).abs().max() / a0.abs().max())) > 100 * TOL_CHAIN
    assert _say("velocity / coupling vs oracle", rel(out, ref)) < TOL_CHAIN
    assert _say("zero objective vs oracle", rel(out0, ref0)) < TOL_CHAIN


# ------------------------------------------------------------------ 4. built-in route equals generic route
def test_builtin_route_equals_generic_route(device, unet8, diff8):
    m, _ = unet8
    B = 3
    obj = make_quadratic(71, HZ, 8, B, time_consistency_coef=0.25)
    d = _ddim(device, m, 10, 0.4)
    tp = _tape(6400, (B, HZ, 8), 10, 3)
    kw = dict(batch_size=B, n_composed=0, compose_mode="mean-inside", design_guidance="standard-alpha-recurrence-3")
    fast = d.sample(design_fn=obj, noise=_nt(tp), **kw)
    slow = d.sample(design_fn=lambda x: obj(x), noise=_nt(tp), **kw)
    assert bool(torch.isfinite(slow).all())
    assert _say("routes ddim", rel(fast, slow)) < TOL_CHAIN
    obj40 = make_quadratic(72, 40, 8, B, time_consistency_coef=0.25)
    tape = O.NoiseTape.make(94, (B, 40, 8), 1000, recur=2)
    kw = dict(batch_size=B, n_composed=1, compose_start_step=16, compose_mode="mean-inside", design_guidance="standard-recurrence-2",
              noise=cindm_amd.NoiseTape(tape.init, tape.step, tape.recur), t_stop=992)
    fast = diff8.sample(design_fn=obj40, **kw)
    slow = diff8.sample(design_fn=lambda x: obj40(x), **kw)
    assert bool(torch.isfinite(slow).all())
    assert _say("routes ddpm", rel(fast, slow)) < TOL_CHAIN


# ------------------------------------------------------------------ 5. the two kernel branches agree
RESTATE_KW = dict(n_composed=0, compose_mode="mean-inside", design_guidance="standard-recurrence-2")


def restated_waypoint(cls=Q):
    """(waypoint objective, its quadratic restatement, tape): coef 0.2 on weights of 0.5 .. 1.5, so that the restatement's S = diag 2 scale
    stays below 0.6 like the other chain tables (at coef 2 the step x - 6 (x - target) of "standard" guidance diverges on both branches)."""
    B, nb = 2, 2
    target, weight = make_tables(41, HZ, nb, B, True, True)
    way = cindm_amd.WaypointObjective(target, weight, coef=0.2, time_consistency_coef=0.25, design_fn_mode="L2square")
    S, h = torch.zeros((B, HZ, 8, 8)), torch.zeros((B, HZ, 8))
    for j in range(nb):
        for c in range(2):
            S[..., 4 * j + c, 4 * j + c] = 2.0 * way.scale[..., j]
            h[..., 4 * j + c] = 2.0 * way.scale[..., j] * way.target[..., j, c]
    return way, cls(S, h, time_consistency_coef=0.25), _tape(6500, (B, HZ, 8), 10, 2)


def test_quadratic_restatement_of_a_waypoint_objective(device, unet8):
    """scale * ||x - target||^2 = 1/2 x^T (2 scale I) x - (2 scale target)^T x + const on the position features: the waypoint branch
    (mode 4) and the quadratic branch compute the same chain -- within TOL_CHAIN, not bitwise: (s * 2) * (x - t) against
    (0 + (2 s) * x + 0 * ...) - (2 s) t."""
    m, sd = unet8
    way, quad, tp = restated_waypoint(_NeverCalled)
    od = O.Diffusion1D(sd, image_size=HZ, conditioned_steps=0)
    run = lambda fn: O.ddim_sample(od, (2, HZ, 8), None, tp, sampling_timesteps=10, eta=0.3, design_fn=fn, **RESTATE_KW)
    ref = run(way)
    _moved("restated waypoint", way, ref, run(zero_objective(HZ, 8, time_consistency_coef=0.25)))
    d = _ddim(device, m, 10, 0.3)
    a = d.sample(batch_size=2, design_fn=way, noise=_nt(tp), **RESTATE_KW)
    b = d.sample(batch_size=2, design_fn=quad, noise=_nt(tp), **RESTATE_KW)
    assert bool(torch.isfinite(a).all())
    assert _say("waypoint branch vs quadratic branch", rel(b, a)) < TOL_CHAIN
    assert _say("quadratic branch vs oracle", rel(b, ref)) < TOL_CHAIN


# ------------------------------------------------------------------ 6. bitwise by construction
def test_broadcast_equals_materialised(device, unet8):
    m, _ = unet8
    B = 3
    d = _ddim(device, m, 10, eta=0.5)
    S, h = quad_tables(61, HZ, 8, 1, 0.3)
    S, h = S[0], h[0]
    kw = dict(batch_size=B, n_composed=0, compose_mode="mean-inside", design_guidance="standard-recurrence-2", seed=17)
    shared = d.sample(design_fn=Q(S, h, time_consistency_coef=0.25), **kw)
    assert bool(torch.isfinite(shared).all())
    for SS, hh in ((S.expand(B, -1, -1, -1), h.expand(B, -1, -1)), (S.expand(B, -1, -1, -1), h), (S, h.expand(B, -1, -1))):
        assert torch.equal(d.sample(design_fn=Q(SS.contiguous(), hh.contiguous(), time_consistency_coef=0.25), **kw), shared)


def test_library_chain_properties(device, unet8, diff8):
    """The objective's Python side is never evaluated; graph == stream; two half-batches with shard + sample_offset == the whole batch
    (counter-based draws), through sample_sharded's own path as well."""
    m, _ = unet8
    B = 4
    d = _ddim(device, m, 9, eta=1.0)            # (9 steps x 3 iterations: odd, the result lands in the workspace buffer)
    obj = make_quadratic(81, HZ, 8, B, cls=_NeverCalled)
    kw = dict(n_composed=0, compose_mode="mean-inside", design_guidance="standard-recurrence-3")
    whole = d.sample(batch_size=B, design_fn=obj, seed=11, **kw)
    assert bool(torch.isfinite(whole).all())
    assert torch.equal(whole, d.sample(batch_size=B, design_fn=obj, seed=11, use_graph=False, **kw))
    parts = [d.sample(batch_size=hi - lo, design_fn=obj.shard(lo, hi), seed=11, sample_offset=lo, **kw) for lo, hi in ((0, 2), (2, 4))]
    assert torch.equal(torch.cat(parts), whole)
    assert not torch.equal(parts[0], parts[1])
    assert torch.equal(cdist.sample_sharded(d, B, seed=11, design_fn=obj, **kw), whole)
    with pytest.raises(AssertionError, match="in Python"):        # the generic routes do call it
        d.sample(batch_size=B, design_fn=obj, seed=11, n_composed=0, compose_mode="mean-inside",
                 design_guidance="universal-forward-recurrence-2")
    obj40 = make_quadratic(82, 40, 8, B, cls=_NeverCalled)
    kw = dict(n_composed=1, compose_start_step=16, compose_mode="mean-inside", design_guidance="standard", t_stop=992)
    whole = diff8.sample(batch_size=B, design_fn=obj40, seed=12, **kw)
    assert bool(torch.isfinite(whole).all())
    assert torch.equal(whole, diff8.sample(batch_size=B, design_fn=obj40, seed=12, use_graph=False, **kw))
    parts = [diff8.sample(batch_size=2, design_fn=obj40.shard(lo, lo + 2), seed=12, sample_offset=lo, **kw) for lo in (0, 2)]
    assert torch.equal(torch.cat(parts), whole)


def test_graph_follows_the_tables(device, unet8):
    """A and B are alive together on one handle, so their device tables have other addresses: the table addresses are part of the
    graph key, B captures its own step, and the same A afterwards gives A's designs again."""
    m, _ = unet8
    d = _ddim(device, m, 6, eta=0.5)
    kw = dict(batch_size=2, n_composed=0, compose_mode="mean-inside", design_guidance="standard-recurrence-2", seed=5)
    A, B_ = (make_quadratic(seed, HZ, 8, 2) for seed in (91, 92))
    a1 = d.sample(design_fn=A, **kw).clone()
    b = d.sample(design_fn=B_, **kw).clone()
    a2 = d.sample(design_fn=A, **kw)
    (Sa, ha), (Sb, hb) = A.tables(device), B_.tables(device)
    assert Sa.data_ptr() != Sb.data_ptr() and ha.data_ptr() != hb.data_ptr()
    assert torch.equal(a1, a2) and not torch.equal(a1, b)
    # B's designs are those of a handle that has never seen A
    assert torch.equal(b, _ddim(device, m, 6, eta=0.5).sample(design_fn=make_quadratic(92, HZ, 8, 2), **kw))


# ------------------------------------------------------------------ 7. with the recorder and a known region
def test_recorder_and_known_region(device, unet8, diff8):
    m, _ = unet8
    d = _ddim(device, m, 10, eta=0.5)
    g = torch.Generator().manual_seed(8)

    def region(L):
        known = torch.rand((L, 8), generator=g) * 1.2 - 0.6
        mask = torch.zeros((L, 8), dtype=torch.bool)
        mask[1] = True                    # a row without terms, whole
        mask[L - 1, 4:6] = True           # the positions of body 1 on the last row, which carries terms: the gradient's row is half known
        return known, mask

    known, mask = region(HZ)
    obj = make_quadratic(95, HZ, 8, 2, cls=_NeverCalled)
    kw = dict(batch_size=2, n_composed=0, compose_mode="mean-inside", design_fn=obj, design_guidance="standard-recurrence-2", seed=7,
              known=known, known_mask=mask)
    out, rec = d.sample(return_trajectory_every=3, trajectory=("x", "x0"), **kw)
    assert rec.step == [3, 6, 9, 10] and tuple(rec.x.shape) == (4, 2, HZ, 8) == tuple(rec.x0.shape)
    assert torch.equal(rec.x[-1], out) and torch.equal(out, d.sample(**kw))
    assert torch.equal(out.cpu()[:, mask], known[mask].expand(2, -1))
    assert not torch.equal(out, d.sample(**dict(kw, known=None, known_mask=None)))
    obj40 = make_quadratic(96, 40, 8, 2, cls=_NeverCalled)
    kw = dict(batch_size=2, n_composed=1, compose_start_step=16, compose_mode="mean-inside", design_fn=obj40,
              design_guidance="standard-recurrence-2", seed=7, t_stop=993)
    out, rec = diff8.sample(return_trajectory_every=3, trajectory=("x", "x0"), **kw)
    assert rec.t == [997, 994, 993] and torch.equal(rec.x[-1], out) and torch.equal(out, diff8.sample(**kw))


# ------------------------------------------------------------------ 8. refusals
def test_refusals_leave_the_handle_usable(device, unet8, diff8):
    B, L = 2, 40
    obj = make_quadratic(97, L, 8, B)
    point = cindm_amd.PointObjective([0.25, -0.5], 2, coef=2.0)
    way = cindm_amd.WaypointObjective(*make_tables(97, L, 2, B, True, True), coef=2.0)
    guid = "standard-recurrence-2"
    desc = diff8._desc_for((B, L, 8), "mean-inside", 1, 16, HZ, 2)
    x0 = torch.randn((B, L, 8), generator=torch.Generator().manual_seed(1)).to(device)
    run = lambda dz, tables: diff8._run_guided_loop(x0.clone(), None, desc, dz, 999, 998, noise=None, seed=3, sample_offset=0,
                                                    inpaint_cond=None, initial_state_overwrite=None, tables=tables)
    h = diff8._handle()
    good = run(obj.descriptor(guid), obj)
    good_way = run(way.descriptor(guid), way)
    assert bool(torch.isfinite(good).all()) and not torch.equal(good, good_way)

    def still_good():
        assert torch.equal(run(obj.descriptor(guid), obj), good)

    with pytest.raises(cindm_amd.CindmError, match="arm them with cindm_ddpm1d_set_design_quadratic"):
        run(obj.descriptor(guid), None)                                  # mode 5, nothing armed
    still_good()
    with pytest.raises(cindm_amd.CindmError, match="quadratic design tables are armed but the descriptor's mode is 1 .. 4"):
        run(point.descriptor(guid), obj)                                 # armed quadratic tables, point descriptor (mode 1)
    still_good()
    obj.arm(h, B, device)
    with pytest.raises(cindm_amd.CindmError, match="quadratic design tables are armed but the descriptor's mode is 1 .. 4"):
        run(way.descriptor(guid), way)                                   # both armed, waypoint descriptor (mode 3)
    assert torch.equal(run(way.descriptor(guid), way), good_way)
    still_good()
    way.arm(h, B, device)
    with pytest.raises(cindm_amd.CindmError, match="the descriptor's mode is 5"):
        run(obj.descriptor(guid), obj)                                   # both armed, quadratic descriptor
    still_good()
    with pytest.raises(cindm_amd.CindmError, match="the descriptor's mode is 5"):
        run(obj.descriptor(guid), way)                                   # waypoint tables alone under mode 5
    still_good()
    wrong = make_quadratic(97, L + 16, 8, B)
    with pytest.raises(cindm_amd.CindmError, match="56 rows, the state has 40"):
        run(wrong.descriptor(guid), wrong)                               # the library's own checks
    with pytest.raises(cindm_amd.CindmError, match="16 features, the composition's state has 8"):
        run(obj.descriptor(guid), make_quadratic(97, L, 16, B))
    with pytest.raises(cindm_amd.CindmError, match="batch of 3"):
        run(obj.descriptor(guid), make_quadratic(97, L, 8, 3))
    still_good()
    kw = dict(batch_size=B, n_composed=1, compose_start_step=16, compose_mode="mean-inside", design_guidance=guid, seed=3, t_stop=998)
    for bad in (wrong, make_quadratic(97, L, 16, B), make_quadratic(97, L, 8, 3)):
        with pytest.raises(ValueError, match="QuadraticObjective"):      # the public route refuses before any device work
            diff8.sample(design_fn=bad, **kw)
    # armed tables on a chain that is not guided: refused with the reason, consumed, and the next unguided chain runs
    obj.arm(h, B, device)
    with pytest.raises(cindm_amd.CindmError, match="quadratic design tables: only the guided 1-D chains"):
        diff8.sample(batch_size=B, n_composed=0, seed=3, t_stop=998)
    assert bool(torch.isfinite(diff8.sample(batch_size=B, n_composed=0, seed=3, t_stop=998)).all())
    S, hv = obj.tables(device)
    lib = _ffi.lib()
    assert lib.cindm_ddpm1d_set_design_quadratic(h, _ffi.ptr(S), 1, None, 1, L, 8, B) != 0          # one table without the other
    assert lib.cindm_ddpm1d_set_design_quadratic(h, _ffi.ptr(S), 1, _ffi.ptr(hv), 1, L, 6, B) != 0   # features no multiple of 4
    assert lib.cindm_ddpm1d_set_design_quadratic(h, _ffi.ptr(S), 1, _ffi.ptr(hv), 1, L, 36, B) != 0  # ... above 32
    _ffi.check(lib.cindm_ddpm1d_set_design_quadratic(h, _ffi.ptr(S), 1, _ffi.ptr(hv), 1, L, 8, B))
    _ffi.check(lib.cindm_ddpm1d_set_design_quadratic(h, None, 0, None, 0, 0, 0, 0))                 # disarm
    assert bool(torch.isfinite(diff8.sample(batch_size=B, n_composed=0, seed=3, t_stop=998)).all())
    # tables that are not 16-byte aligned
    off = torch.zeros((S.numel() + 1,), device=device)[1:]
    assert off.data_ptr() % 16 == 4
    _ffi.check(lib.cindm_ddpm1d_set_design_quadratic(h, _ffi.ptr(off), 1, _ffi.ptr(hv), 1, L, 8, B))
    with pytest.raises(cindm_amd.CindmError, match="16-byte aligned"):
        run(obj.descriptor(guid), None)
    still_good()
    assert bool(torch.isfinite(diff8.sample(design_fn=obj, **kw)).all())
