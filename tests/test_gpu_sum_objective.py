"""GPU (MI355X): the sum of built-in objectives (cindm_amd.SumObjective) inside the two captured guided chains
(cindm_ddpm1d_sample_guided / _sample_ddim_guided with descriptor mode 7, every term's tables armed, compose_update_sum_kernel<false>
and <true>).

1. Per element against float64, the idiom of tests/test_gpu_step1d_f64.py on the 40 cases of tests/sum_cases.py: the library's own
   U-Net outputs E -> ``compose_predict_f64`` -> the summed (g, A_g, n_g) of ``sum_cases.sum_grad_f64`` -> ``step1d_update_f64``;
   asserted |got - ref| <= (n_e + 4) * 2^-24 * A_e on every element, and that the multistep history handed back is the step's x_start
   bit for bit.  tests/test_sum_objective_host.py proves the statement first (fp32 closed form within the bound; mutations leave it).
2. A sum of one term returns that term's own chain, bit for bit, for each kind on both guided chains.
3. Against oracle/cindm_oracle.py, which differentiates the same ``SumObjective`` callable with autograd on the CPU: single steps
   within TOL_STEP, short chains on both guided entries within TOL_CHAIN (tests/test_gpu_parity.py's); the ``dpmpp-2m`` chain against
   the route that loops in Python.  A ``_NeverCalled`` subclass shows that the built-in route never evaluates the objective in Python.
   The chain cases' guards are conditions on the oracle alone (``chain_refs``): ``_not_degenerate``, max |ref| < 100, the sum moved the
   oracle's result by more than 100 * TOL_CHAIN against the zero-weight chain, dropping ANY single term (its tables zeroed) moves it by
   more than 100 * TOL_CHAIN -- a kernel that silently loses a term cannot pass -- and tests/test_gpu_pairdist.py's ``_conditions``.
   Tables are the existing recipes: ``make_tables``, ``make_quadratic``, ``pair_tables`` with scale 0.5 / n_bodies.
4. The graph follows the tables: other tables of the same shapes, then other kinds armed, on one handle.
5. Recorder, known region and ``sample_sharded`` with a per-design sum.
6. Refusals leave the handle usable."""
import pytest
import torch

import cindm_amd
import cindm_oracle as O
import step1d_cases as S
import sum_cases as SC
from cindm_amd import dist as cdist
from test_gpu_compose_f64 import _unet_outputs
from test_gpu_ddim_guided import _not_degenerate, _nt, _tape
from test_gpu_multistep import CH, HW, _diff2, _force_objective
from test_gpu_pairdist import _Watch, _conditions, make_pairdist
from test_gpu_parity import TOL_CHAIN, TOL_STEP, build_unet, rel
from test_gpu_parity_2d import build_unet2d
from test_gpu_quadratic import _ddim, make_quadratic
from test_gpu_step1d_f64 import TAB, _diff, _run
from test_gpu_waypoint import make_tables

pytestmark = pytest.mark.gpu

HZ = 24
WP, QD, PD, SUM = cindm_amd.WaypointObjective, cindm_amd.QuadraticObjective, cindm_amd.PairDistanceObjective, cindm_amd.SumObjective


def _say(name, v):
    print(f"[sum] {name}: {v:.3e}")
    return v


class _NeverCalled(SUM):
    def __call__(self, pos):
        raise AssertionError("the built-in route evaluated the objective in Python")


@pytest.fixture(scope="module")
def unet8(device):
    return build_unet(device)


@pytest.fixture(scope="module")
def diff8(device, unet8):
    return cindm_amd.GaussianDiffusion1D(unet8[0], image_size=HZ, conditioned_steps=0, timesteps=1000, sampling_timesteps=1000,
                                         loss_type="l1").to(device)


# ------------------------------------------------------------------ 1. per element against float64
def _hold(case, m, device):
    d = SC.inputs(case)
    t, tn = S.case_times(case)
    E, _ = _unet_outputs((m, None), case.desc(), d["x"], None, t, device)
    row = None
    if case.entry == "ddim":
        dd = _diff(device, m, case.objective, S.DDIM_S, case.eta)
        kap = dd.multistep_kappa()[case.step] if case.ms else torch.zeros(())
        row = torch.cat([dd.ddim_schedule()[1][case.step], kap.reshape(1)])
    st = SC.statement(case, d, E, TAB[case.objective], row=row)
    out, hist, x0 = _run(case, d, m, device)
    r, where = S.ratio(out, st["state"])
    print(f"{case.name}: err/bound {r:.4f} at {where}, clamped {st['clamped']:.3f}")
    if hist is not None:
        assert x0 is not None and torch.equal(hist, x0), case.name          # the history handed back IS the step's x_start
    return [] if r <= 1.0 else [(case.name, round(r, 3), where)]


GROUPS = sorted({(c.terms, c.entry) for c in SC.CASES})


@pytest.mark.parametrize("terms,entry", GROUPS, ids=[f"{t}-{e}" for t, e in GROUPS])
def test_step_against_float64(device, unet8, terms, entry):
    cases = [c for c in SC.CASES if (c.terms, c.entry) == (terms, entry)]
    assert cases
    over = []
    for c in cases:
        over += _hold(c, unet8[0], device)
    assert not over, over


# ------------------------------------------------------------------ the chain cases' objectives
def zeroed(t):
    """The term with its weights zeroed and its time-consistency coefficient kept."""
    tc = t.time_consistency_coef
    if isinstance(t, WP):
        return WP(t.target, None, _scale=torch.zeros_like(t.scale), time_consistency_coef=tc, design_fn_mode=t.design_fn_mode)
    if isinstance(t, QD):
        return QD(torch.zeros_like(t.S), torch.zeros_like(t.h), time_consistency_coef=tc)
    return PD(t.lo, t.hi, torch.zeros_like(t.weight), time_consistency_coef=tc)


def make_terms(seed, x0, nb, *, norm="L2", tc=0.25, per=(True, False, True), scales=(1.0, 0.3, None), pair_cls=PD):
    """(quadratic, waypoint, pair-distance) terms for the first state x0 [B, L, 4 nb] by the existing recipes; ``per``: which of them
    carry per-design tables (the waypoint's target and the pair's band and weight; the quadratic's S -- its h is per design where S is
    not); tc in halves on the quadratic and the waypoint term.  ``scales``: (waypoint coef, quadratic scale, pair scale | None = 0.5 / nb)."""
    B, L, F = x0.shape
    target, weight = make_tables(seed + 1, L, nb, B, per[1], not per[1])
    way = WP(target, weight, coef=scales[0], time_consistency_coef=0.5 * tc, design_fn_mode=norm)
    quad = make_quadratic(seed + 2, L, F, B, per[0], not per[0], scale=scales[1], time_consistency_coef=0.5 * tc)
    pair = make_pairdist(seed + 3, x0, nb, per[2], per[2], scales[2], cls=pair_cls)
    return quad, way, pair


# ------------------------------------------------------------------ 2. one term is that term
DDPM_KW = dict(n_composed=1, compose_start_step=16, compose_mode="mean-inside", design_guidance="standard-recurrence-2", t_stop=990,
               compose_n_bodies=3)
DDIM_KW = dict(n_composed=0, compose_mode="mean-inside", design_guidance="standard-recurrence-2", compose_n_bodies=3)


def test_one_term_sum_is_the_terms_own_chain(device, unet8, diff8):
    m, _ = unet8
    B, nb = 3, 3
    tape = O.NoiseTape.make(192, (B, 40, 4 * nb), 1000, recur=2)
    nt = cindm_amd.NoiseTape(tape.init, tape.step, tape.recur)
    tp = _tape(8100, (B, HZ, 4 * nb), 10, 2)
    d = _ddim(device, m, 10, 0.3)
    seen = []
    for k, (t40, t24) in enumerate(zip(make_terms(100, tape.init, nb, norm="L2square", scales=(0.2, 0.3, None)), make_terms(110, tp["init"], nb))):
        own = diff8.sample(batch_size=B, design_fn=t40, noise=nt, **DDPM_KW)
        assert bool(torch.isfinite(own).all()) and torch.equal(diff8.sample(batch_size=B, design_fn=SUM(t40), noise=nt, **DDPM_KW), own), k
        own24 = d.ddim_sample((B, HZ, 4 * nb), None, design_fn=t24, noise=_nt(tp), **DDIM_KW)
        assert bool(torch.isfinite(own24).all()) and torch.equal(d.ddim_sample((B, HZ, 4 * nb), None, design_fn=SUM(t24), noise=_nt(tp), **DDIM_KW), own24), k
        seen.append((own, own24))
    assert not torch.equal(seen[0][0], seen[1][0]) and not torch.equal(seen[1][1], seen[2][1])
    # a point term is its table form, and the point objective's own chain (two bodies: the point objective's chain state)
    pt = cindm_amd.PointObjective([0.25, -0.5], 3, coef=1.5, time_consistency_coef=0.25)
    d2 = _ddim(device, m, 10, 0.3)
    kw = dict(batch_size=2, n_composed=0, compose_mode="mean-inside", design_guidance="standard-recurrence-2", seed=5)
    assert torch.equal(d2.sample(design_fn=SUM(pt), **kw), d2.sample(design_fn=pt, **kw))


# ------------------------------------------------------------------ 3. against the oracle
STEP_CASES = [("standard", 0.0, "L2", False, 3), ("standard-alpha", 0.5, "L2square", True, 4), ("standard-recurrence-2", 0.5, "L2", True, 2),
              ("standard-alpha-recurrence-3", 0.0, "L2square", False, 3)]
STEP_B, STEP_L = 2, 56


def step_kw(nb):
    return dict(compose_mode="mean-inside", n_composed=2, compose_start_step=16, single_model_step=HZ, compose_n_bodies=nb)


def step_inputs(guid, use_iso, nb):
    R = int(guid.split("-")[-1]) if "recurrence" in guid else 0
    g = torch.Generator().manual_seed(121 + nb)
    shape = (STEP_B, STEP_L, 4 * nb)
    out = []
    for t in (600, 30, 0):
        x = torch.randn(shape, generator=g) * 0.7
        out.append((t, x, torch.randn(shape, generator=g), torch.randn((max(R, 1),) + shape, generator=g),
                    torch.randn((STEP_B, 4, 4 * nb), generator=g) * 0.3 if use_iso else None))
    return R, out


def step_objective(guid, tc, norm, nb, x, cls=SUM, pair_cls=PD):
    R = int(guid.split("-")[-1]) if "recurrence" in guid else 0
    amp = 100.0 if "alpha" in guid else 1.0          # (eta_t is 1e-4 .. 1e-2)
    q, w, p = make_terms(211, x, nb, norm=norm, tc=tc, scales=(amp, 0.3 * amp, (0.5 / nb if R else 1.0) * amp), pair_cls=pair_cls)
    return cls(q, w, p)


@pytest.mark.parametrize("guid,tc,norm,use_iso,nb", STEP_CASES)
def test_step_vs_oracle(device, unet8, diff8, guid, tc, norm, use_iso, nb):
    _, sd = unet8
    B, L, F = STEP_B, STEP_L, 4 * nb
    od = O.Diffusion1D(sd, image_size=HZ, conditioned_steps=0)
    R, inputs = step_inputs(guid, use_iso, nb)
    desc = diff8._desc_for((B, L, F), "mean-inside", 2, 16, HZ, nb)
    for t, x, nz, rn, iso in inputs:
        watch = step_objective(guid, tc, norm, nb, x, pair_cls=_Watch)
        ref, _ = O.p_sample_compose_inside(od, x.clone(), None, t, nz, design_fn=watch, design_guidance=guid, recur_noise=rn,
                                           initial_state_overwrite=iso, **step_kw(nb))
        _conditions(f"step {guid} nb={nb} t={t}", watch.terms[2])
        assert bool(torch.isfinite(ref).all())
        if R == 0 and t == 600:           # the gradient moves the step by far more than the tolerance
            ung, _ = O.p_sample_compose_inside(od, x.clone(), None, t, nz, design_guidance=guid, initial_state_overwrite=iso, **step_kw(nb))
            assert _say(f"step {guid} t={t}: gradient moved the step by", rel(ung, ref)) > 100 * TOL_STEP
        obj = step_objective(guid, tc, norm, nb, x, cls=_NeverCalled)
        obj.check_state(B, L, nb)
        step = torch.zeros((1000, B, L, F)); step[t] = nz
        rec = torch.zeros((1000, max(R, 1), B, L, F)); rec[t] = rn
        tape = cindm_amd.NoiseTape(None, step, rec).to(device)
        out = diff8._run_guided_loop(x.clone().to(device), None, desc, obj.descriptor(guid), t, t, noise=tape, seed=0, sample_offset=0,
                                     inpaint_cond=None, initial_state_overwrite=None if iso is None else iso.to(device), tables=obj)
        assert _say(f"step {guid} nb={nb} tc={tc} t={t}", rel(out, ref)) < TOL_STEP, (guid, t)


CHAIN_KW = dict(DDPM_KW, t_stop=994)


def ddpm_case():
    """t = 999 .. 994, B = 3, three bodies, one composed window more (L_tot = 40, cs = 16), tc = 0.25."""
    B, L, nb = 3, 40, 3
    return B, L, nb, O.NoiseTape.make(292, (B, L, 4 * nb), 1000, recur=2)


def ddim_case():
    """S = 10, eta = 0.3, B = 2, L = 24, three bodies, overwrite rows 0 .. 2."""
    B, nb = 2, 3
    shape = (B, HZ, 4 * nb)
    iso = torch.randn((B, 3, 4 * nb), generator=torch.Generator().manual_seed(801)) * 0.3
    return shape, nb, _tape(8200, shape, 10, 2), iso


DDPM_TERMS = dict(norm="L2", tc=0.25, per=(True, False, True), scales=(1.0, 0.3, None))
DDIM_TERMS = dict(norm="L2square", tc=0.25, per=(False, True, True), scales=(0.5, 0.3, None))
MS_TERMS = dict(DDPM_TERMS, scales=(0.3, 0.3, None))          # (test_ddim_chain_with_the_multistep_solver says why)


def chain_refs(od, which):
    """(the oracle's result, guards asserted) of a chain case -- conditions on the oracle alone, no library call: runs on the CPU."""
    if which == "ddpm":
        B, L, nb, tape = ddpm_case()
        terms = make_terms(300, tape.init, nb, pair_cls=_Watch, **DDPM_TERMS)
        run = lambda fn: O.sample(od, B, tape, design_fn=fn, **CHAIN_KW)
    else:
        shape, nb, tp, iso = ddim_case()
        terms = make_terms(310, tp["init"], nb, pair_cls=_Watch, **DDIM_TERMS)
        run = lambda fn: O.ddim_sample(od, shape, None, tp, sampling_timesteps=10, eta=0.3, design_fn=fn, initial_state_overwrite=iso, **DDIM_KW)
    obj = SUM(*terms)
    ref = run(obj)
    _conditions(f"{which} chain", terms[2])
    plain = [PD(t.lo, t.hi, t.weight, time_consistency_coef=t.time_consistency_coef) if isinstance(t, PD) else t for t in terms]
    _not_degenerate(SUM(*plain), ref)
    assert float(ref.abs().max()) < 100.0
    assert _say(f"{which} chain: the sum moved the oracle's result by", rel(ref, run(SUM(*(zeroed(t) for t in plain))))) > 100 * TOL_CHAIN
    for j, name in enumerate(("quadratic", "waypoint", "pair-distance")):
        less = SUM(*(zeroed(t) if i == j else t for i, t in enumerate(plain)))
        assert _say(f"{which} chain: dropping the {name} term moves the oracle's result by", rel(run(less), ref)) > 100 * TOL_CHAIN
    return ref


def test_ddpm_chain_vs_oracle(device, unet8, diff8):
    _, sd = unet8
    B, L, nb, tape = ddpm_case()
    ref = chain_refs(O.Diffusion1D(sd, image_size=HZ, conditioned_steps=0), "ddpm")
    obj = _NeverCalled(*make_terms(300, tape.init, nb, **DDPM_TERMS))
    out = diff8.sample(batch_size=B, design_fn=obj, noise=cindm_amd.NoiseTape(tape.init, tape.step, tape.recur), **CHAIN_KW)
    assert tuple(out.shape) == (B, L, 4 * nb)
    assert _say("ddpm chain vs oracle", rel(out, ref)) < TOL_CHAIN


def test_ddim_chain_vs_oracle(device, unet8):
    m, sd = unet8
    shape, nb, tp, iso = ddim_case()
    ref = chain_refs(O.Diffusion1D(sd, image_size=HZ, conditioned_steps=0), "ddim")
    obj = _NeverCalled(*make_terms(310, tp["init"], nb, **DDIM_TERMS))
    d = _ddim(device, m, 10, 0.3)
    out = d.ddim_sample(shape, None, design_fn=obj, initial_state_overwrite=iso.to(device), noise=_nt(tp), **DDIM_KW)
    assert tuple(out.shape) == shape
    assert _say("ddim chain vs oracle", rel(out, ref)) < TOL_CHAIN
    with pytest.raises(AssertionError, match="in Python"):        # the generic routes do call it
        d.ddim_sample(shape, None, design_fn=obj, seed=11, n_composed=0, compose_mode="mean-inside", compose_n_bodies=nb,
                      design_guidance="universal-forward-recurrence-2")


def test_ddim_chain_with_the_multistep_solver(device, unet8):
    """compose_update_sum_kernel<true>: against the route that loops in Python (library predictions, autograd on the callable, the
    solver's term in torch), as tests/test_gpu_multistep.py holds the other objectives' guided chains.

    A condition on that route alone says that the case measures the kernel and not the chain: x_T scaled by 1 + 2^-22 (four fp32
    roundings) must move ITS result by less than TOL_CHAIN / 5.  The two routes differ by about one rounding per iteration over 20
    iterations -- five times that perturbation -- so a case that holds the condition cannot explain a disagreement of TOL_CHAIN by its
    own amplification.  With the "L2" waypoint at coef = 1 the condition fails (measured: 2.8e-5, and 1.2e-4 without the solver; the
    routes then differ by 6e-4): under "standard" guidance a body within coef of its target hops over it, where the normalised
    gradient is discontinuous.  The case therefore runs that term at coef = 0.3 (measured: 1.2e-5, routes 1.2e-5); the "L2" norm at
    full scale under the solver is held per element by the float64 cases above."""
    m, _ = unet8
    shape, nb, tp, _ = ddim_case()
    d = _ddim(device, m, 10)
    terms = make_terms(320, tp["init"], nb, pair_cls=_Watch, **MS_TERMS)
    watch = SUM(*terms)
    slow = d.ddim_sample(shape, None, design_fn=lambda x: watch(x), noise=_nt(tp), solver="dpmpp-2m", **DDIM_KW)
    _conditions("ddim multistep", terms[2])
    obj = _NeverCalled(*make_terms(320, tp["init"], nb, **MS_TERMS))
    again = SUM(*make_terms(320, tp["init"], nb, **MS_TERMS))
    nudged = d.ddim_sample(shape, None, design_fn=lambda x: again(x), noise=_nt(dict(tp, init=tp["init"] * (1 + 2.0 ** -22))), solver="dpmpp-2m", **DDIM_KW)
    assert _say("multistep: the Python route's own sensitivity to four roundings of x_T", rel(nudged, slow)) < TOL_CHAIN / 5
    fast = d.ddim_sample(shape, None, design_fn=obj, noise=_nt(tp), solver="dpmpp-2m", **DDIM_KW)
    plain = d.ddim_sample(shape, None, design_fn=obj, noise=_nt(tp), **DDIM_KW)
    assert bool(torch.isfinite(slow).all()) and float(slow.abs().max()) < 100.0
    assert _say("multistep routes", rel(fast, slow)) < TOL_CHAIN
    assert _say("multistep vs ddim", rel(fast, plain)) > 100 * TOL_CHAIN
    for j, name in enumerate(("quadratic", "waypoint", "pair-distance")):
        less = SUM(*(zeroed(t) if i == j else t for i, t in enumerate(obj.terms)))
        moved = rel(d.ddim_sample(shape, None, design_fn=less, noise=_nt(tp), solver="dpmpp-2m", **DDIM_KW), fast)
        assert _say(f"multistep: dropping the {name} term moves the result by", moved) > 100 * TOL_CHAIN


# ------------------------------------------------------------------ 4. the graph follows the tables
def test_graph_follows_the_tables(device, unet8):
    m, _ = unet8
    B, nb = 2, 3
    d = _ddim(device, m, 6, eta=0.5)
    shape = (B, HZ, 4 * nb)
    kw = dict(seed=5, **DDIM_KW)
    x0 = torch.randn(shape, generator=torch.Generator().manual_seed(8))
    A, B_ = (SUM(*make_terms(seed, x0, nb)) for seed in (400, 410))
    run = lambda dd, fn: dd.ddim_sample(shape, None, design_fn=fn, **kw).clone()
    a1, b, a2 = run(d, A), run(d, B_), run(d, A)
    for ta, tb in zip(A.terms, B_.terms):
        assert all(u.data_ptr() != v.data_ptr() for u, v in zip(ta.tables(device), tb.tables(device)))
    assert torch.equal(a1, a2) and not torch.equal(a1, b)
    fresh = lambda fn: run(_ddim(device, m, 6, eta=0.5), fn)
    assert torch.equal(b, fresh(SUM(*make_terms(410, x0, nb))))
    # other kinds armed, on the same handle: every subset gives what a handle that has seen nothing else gives
    q, w, p = A.terms
    for sub in ((q, p), (w,), (w, p), (q, w), (q, w, p)):
        got = run(d, SUM(*sub))
        assert torch.equal(got, fresh(SUM(*sub))), [type(t).__name__ for t in sub]
        assert torch.equal(got, a1) == (len(sub) == 3)


# ------------------------------------------------------------------ 5. recorder, known region, sample_sharded
def test_recorder_known_region_and_shards(device, unet8, diff8):
    m, _ = unet8
    d = _ddim(device, m, 10, eta=0.5)
    g = torch.Generator().manual_seed(8)
    known = torch.rand((HZ, 8), generator=g) * 1.2 - 0.6
    mask = torch.zeros((HZ, 8), dtype=torch.bool)
    mask[1] = True
    mask[HZ - 1, 4:6] = True
    obj = _NeverCalled(*make_terms(500, torch.randn((2, HZ, 8), generator=g), 2))
    assert obj.per_design == 2
    kw = dict(batch_size=2, n_composed=0, compose_mode="mean-inside", design_fn=obj, design_guidance="standard-recurrence-2", seed=7,
              known=known, known_mask=mask)
    out, rec = d.sample(return_trajectory_every=3, trajectory=("x", "x0"), **kw)
    assert rec.step == [3, 6, 9, 10] and tuple(rec.x.shape) == (4, 2, HZ, 8) == tuple(rec.x0.shape)
    assert torch.equal(rec.x[-1], out) and torch.equal(out, d.sample(**kw))
    assert torch.equal(out.cpu()[:, mask], known[mask].expand(2, -1))
    assert not torch.equal(out, d.sample(**dict(kw, known=None, known_mask=None)))
    assert not torch.equal(out, d.sample(**dict(kw, design_fn=SUM(*(zeroed(t) for t in obj.terms)))))
    obj40 = _NeverCalled(*make_terms(510, torch.randn((2, 40, 8), generator=g), 2))
    kw = dict(batch_size=2, n_composed=1, compose_start_step=16, compose_mode="mean-inside", design_fn=obj40,
              design_guidance="standard-recurrence-2", seed=7, t_stop=993)
    out, rec = diff8.sample(return_trajectory_every=3, trajectory=("x", "x0"), **kw)
    assert rec.t == [997, 994, 993] and torch.equal(rec.x[-1], out) and torch.equal(out, diff8.sample(**kw))
    # two half-batches with shard + sample_offset == the whole batch (counter-based draws), and sample_sharded's own path
    B = 4
    d9 = _ddim(device, m, 9, eta=1.0)
    obj4 = _NeverCalled(*make_terms(520, torch.randn((B, HZ, 8), generator=g), 2))
    kw = dict(n_composed=0, compose_mode="mean-inside", design_guidance="standard-recurrence-3")
    whole = d9.sample(batch_size=B, design_fn=obj4, seed=11, **kw)
    assert bool(torch.isfinite(whole).all())
    assert torch.equal(whole, d9.sample(batch_size=B, design_fn=obj4, seed=11, use_graph=False, **kw))
    parts = [d9.sample(batch_size=hi - lo, design_fn=obj4.shard(lo, hi), seed=11, sample_offset=lo, **kw) for lo, hi in ((0, 2), (2, 4))]
    assert torch.equal(torch.cat(parts), whole) and not torch.equal(parts[0], parts[1])
    assert torch.equal(cdist.sample_sharded(d9, B, seed=11, design_fn=obj4, **kw), whole)


# ------------------------------------------------------------------ 6. refusals
def test_refusals_leave_the_handle_usable(device, unet8, diff8):
    B, L = 2, 40
    x0 = torch.randn((B, L, 8), generator=torch.Generator().manual_seed(1))
    q, w, p = make_terms(600, x0, 2)
    obj = SUM(q, w, p)
    obj.check_state(B, L, 2)
    point = cindm_amd.PointObjective([0.25, -0.5], 2, coef=2.0)
    guid = "standard-recurrence-2"
    desc = diff8._desc_for((B, L, 8), "mean-inside", 1, 16, HZ, 2)
    xd = x0.to(device)

    class Arm:
        """What _run_guided_loop arms per issue: the given objectives' tables."""
        def __init__(self, *objs):
            self.objs = objs

        def arm(self, h, B, device):
            for o in self.objs:
                o.arm(h, B, device)

    run = lambda dz, tables: diff8._run_guided_loop(xd.clone(), None, desc, dz, 999, 998, noise=None, seed=3, sample_offset=0,
                                                    inpaint_cond=None, initial_state_overwrite=None, tables=tables)
    good = run(obj.descriptor(guid), obj)
    good_way = run(w.descriptor(guid), w)
    plain_kw = dict(batch_size=B, n_composed=0, seed=3, t_stop=998)
    good_plain = diff8.sample(**plain_kw)
    assert bool(torch.isfinite(good).all()) and not torch.equal(good, good_way)

    def still_good():
        assert torch.equal(diff8.sample(**plain_kw), good_plain)                # a plain chain
        assert torch.equal(run(obj.descriptor(guid), obj), good)                # and a guided one, on the same handle

    dz = obj.descriptor(guid)
    assert dz.mode == 7
    with pytest.raises(cindm_amd.CindmError, match="mode 7 sums the table objectives armed on the handle: arm at least one"):
        run(dz, None)
    still_good()
    x12 = torch.randn((B, L, 12), generator=torch.Generator().manual_seed(2))
    x56 = torch.randn((B, L + 16, 8), generator=torch.Generator().manual_seed(2))
    q56, w56, p56 = make_terms(600, x56, 2)
    q12, w12, p12 = make_terms(600, x12, 3)
    q3, w3, p3 = make_terms(600, torch.cat([x0, x0[:1]]), 2)
    for bad, msg in ((w56, "design tables: 56 rows, the state has 40"), (q56, "quadratic design tables: 56 rows, the state has 40"),
                     (p56, "pair-distance design tables: 56 rows, the state has 40"), (w12, "design tables: 3 bodies, the composition has 2"),
                     (q12, "quadratic design tables: 12 features, the composition's state has 8"),
                     (p12, "pair-distance design tables: 3 bodies, the composition has 2"),
                     (w3, "design tables: made for a batch of 3"), (q3, "quadratic design tables: made for a batch of 3"),
                     (p3, "pair-distance design tables: made for a batch of 3")):
        fits = [t for t in (q, w, p) if type(t) is not type(bad)]
        with pytest.raises(cindm_amd.CindmError, match=msg):
            run(dz, Arm(bad, *fits))                                            # one kind does not fit, the others do
        still_good()
    for norm in (0, 3, -1):
        bad_dz = obj.descriptor(guid)
        bad_dz.last_n_step = norm
        with pytest.raises(cindm_amd.CindmError, match="last_n_step names the waypoint term's norm"):
            run(bad_dz, obj)
        still_good()
        ref_dz = (q + p).descriptor(guid)
        ref_dz.time_consistency_coef = bad_dz.time_consistency_coef
        assert ref_dz.last_n_step == 0 and torch.equal(run(bad_dz, Arm(q, p)), run(ref_dz, q + p))          # ignored without waypoint tables
    # modes 1 - 6 still refuse a foreign armed kind, with their messages
    with pytest.raises(cindm_amd.CindmError, match="pair-distance design tables are armed but the descriptor's mode is 1 .. 5"):
        run(w.descriptor(guid), Arm(w, p))
    with pytest.raises(cindm_amd.CindmError, match="quadratic design tables are armed but the descriptor's mode is 1 .. 4"):
        run(point.descriptor(guid), q)
    with pytest.raises(cindm_amd.CindmError, match=r"design tables \(target, scale\) are armed but the descriptor's mode is 6"):
        run(p.descriptor(guid), Arm(w, p))
    with pytest.raises(cindm_amd.CindmError, match="arm them with cindm_ddpm1d_set_design_quadratic"):
        run(q.descriptor(guid), None)
    assert torch.equal(run(w.descriptor(guid), w), good_way)
    still_good()
    # the public route refuses before any device work
    kw = dict(batch_size=B, n_composed=1, compose_start_step=16, compose_mode="mean-inside", design_guidance=guid, seed=3, t_stop=998)
    with pytest.raises(ValueError, match="QuadraticObjective: tables of 56 rows"):
        diff8.sample(design_fn=SUM(q56, w56, p56), **kw)
    assert bool(torch.isfinite(diff8.sample(design_fn=obj, **kw)).all())
    # armed tables on chains that are not guided: refused with the reason, consumed
    obj.arm(diff8._handle(), B, device)
    with pytest.raises(cindm_amd.CindmError, match="design tables: only the guided chains"):
        diff8.sample(**plain_kw)
    still_good()
    m, _ = unet8
    dd = _ddim(device, m, 5)
    Arm(q, p).arm(dd._handle(), B, device)
    with pytest.raises(cindm_amd.CindmError, match="quadratic design tables: only the guided 1-D chains"):
        dd.sample(batch_size=B, n_composed=0, seed=3)                    # the unguided DDIM chain
    assert bool(torch.isfinite(dd.sample(batch_size=B, n_composed=0, seed=3)).all())
    still_good()


def test_2d_entries_refuse_armed_tables(device):
    unet2d = build_unet2d(device)
    sd = O.synth_state_dict_2d(O.force_unet_param_shapes(), 7)
    force = cindm_amd.ForceUnet(dim=64, dim_mults=(1, 2, 4, 8), channels=4)
    force.load_state_dict(sd, strict=True)
    force = force.to(device)
    shape = (1, 2, CH, HW, HW)
    fn = _force_objective(force, 1, 2)
    q, w, p = make_terms(700, torch.randn((2, HZ, 8), generator=torch.Generator().manual_seed(3)), 2)
    for d, call in ((_diff2(device, unet2d, 1000), lambda d: d.p_sample_loop(shape, seed=1, t_stop=998)),
                    (_diff2(device, unet2d, 2), lambda d: d.ddim_sample(shape, fn, "standard-alpha", seed=1))):
        for t in (q, w, p):
            t.arm(d._handle(), 2, device)
        with pytest.raises(cindm_amd.CindmError, match="design tables: only the guided chains"):
            call(d)
        out = call(d)                                                     # the refused call consumed every kind
        assert bool(torch.isfinite(out[0] if isinstance(out, tuple) else out).all())
