"""GPU (MI355X): the pair-distance objective (cindm_amd.PairDistanceObjective) inside the two captured guided chains
(cindm_ddpm1d_sample_guided / _sample_ddim_guided with descriptor mode 6, cindm_ddpm1d_set_design_pairdist, compose_update_pair_kernel<false> and <true>).

Expectations come from oracle/cindm_oracle.py on the CPU at test time, differentiating the SAME callable with autograd where the update
kernel evaluates the closed form from its two device tables.  Tolerances: tests/test_gpu_parity.py's TOL_STEP on single guided steps
and TOL_CHAIN on short whole chains.  The oracle has no multistep solver: the one ``solver="dpmpp-2m"`` chain is held against the
route that loops in Python (library predictions, autograd on the callable, the solver's term in torch), as tests/test_gpu_multistep.py
holds the other objectives' guided chains.

Tables (``pair_tables``): entries on every second row and on the last row, for every pair; an entry's relation goes by (its running
number + the design) % 3 -- apart, within, at -- and a fifth of them have weight 0.  The bound d of an entry is set from the distance r0
of its pair in the case's first state (design 0's for shared tables): one apart and one within entry in four is active in that state
(lo = 1.3 r0, hi = 0.7 r0), the others are not (lo = 0.4 r0, hi = 2.5 r0: wide, so that most stay inactive in the other designs of a
shared table too), and at entries (1.3 r0 or 0.7 r0) always are: half of the entries in all.  Weights are (0.5 .. 1.5) * scale with scale = 0.5 / n_bodies for
every chain and recurrence case ("standard" guidance takes the raw gradient: x - 2 w n_bodies (..) has to contract) and 1.0 for the
single steps without recurrence, where the gradient then dominates the step.

The oracle's callable is a ``_Watch``: it notes, in every state the oracle visits, the smallest distance of a weighted pair, and in
the first one the share of the weighted entries that are active.  Every case asserts r > 1e-3 throughout, at least a quarter active
and a quarter inactive at the start, and all three relations among the weighted entries (``_conditions``).  Chain cases also keep the
quadratic file's guards: ``_not_degenerate``, max |ref| < 100 and that the objective moved the oracle's result by more than 100 *
TOL_CHAIN against the zero-weight chain."""
import pytest
import torch

import cindm_amd
import cindm_oracle as O
import test_ula_host as U
from cindm_amd import _ffi
from cindm_amd import dist as cdist
from test_gpu_ddim_guided import _not_degenerate, _nt, _tape
from test_gpu_multistep import CH, HW, _diff2, _force_objective
from test_gpu_parity import TOL_CHAIN, TOL_STEP, build_unet, rel
from test_gpu_parity_2d import build_unet2d
from test_gpu_quadratic import _ddim, make_quadratic
from test_gpu_waypoint import make_tables

pytestmark = pytest.mark.gpu

HZ = 24
INF = float("inf")
PD = cindm_amd.PairDistanceObjective


def _say(name, v):
    print(f"[pairdist] {name}: {v:.3e}")
    return v


@pytest.fixture(scope="module")
def unet8(device):
    return build_unet(device)


@pytest.fixture(scope="module")
def diff8(device, unet8):
    return cindm_amd.GaussianDiffusion1D(unet8[0], image_size=HZ, conditioned_steps=0, timesteps=1000, sampling_timesteps=1000,
                                         loss_type="l1").to(device)


def _pairs(nb):
    return [(i, j) for i in range(nb) for j in range(i + 1, nb)]


def _dist(x, nb):
    """r [B, L, P] of a state x [B, L, 4 nb], float64 on the CPU."""
    p = x.detach().cpu().double().reshape(x.shape[0], x.shape[1], nb, 4)[..., :2]
    I, J = (torch.tensor(v) for v in zip(*_pairs(nb)))
    return (p[:, :, I] - p[:, :, J]).norm(dim=-1)


def pair_tables(seed, x0, nb, scale):
    """(lo, hi, weight), each [B, L, P], of the recipe in the module docstring for the first state x0 [B, L, 4 nb]."""
    B, L, _ = x0.shape
    P = nb * (nb - 1) // 2
    g = torch.Generator().manual_seed(seed)
    r0 = _dist(x0, nb).float()
    lo, hi, w = torch.zeros((B, L, P)), torch.full((B, L, P), INF), torch.zeros((B, L, P))
    rows = sorted(set(range(0, L, 2)) | {L - 1})
    for b in range(B):
        k = b
        for l in rows:
            for p in range(P):
                active = (k // 3) % 4 == 0
                if k % 3 == 0:
                    lo[b, l, p] = float(r0[b, l, p]) * (1.3 if active else 0.4)                  # apart
                elif k % 3 == 1:
                    lo[b, l, p], hi[b, l, p] = 0.0, float(r0[b, l, p]) * (0.7 if active else 2.5)  # within
                else:
                    lo[b, l, p] = hi[b, l, p] = float(r0[b, l, p]) * (1.3 if active else 0.7)    # at
                w[b, l, p] = 0.0 if k % 5 == 4 else (0.5 + float(torch.rand((), generator=g))) * scale
                k += 1
    return lo, hi, w


def make_pairdist(seed, x0, nb, per_band=True, per_w=True, scale=None, cls=PD, **kw):
    lo, hi, w = pair_tables(seed, x0, nb, 0.5 / nb if scale is None else scale)
    pick = lambda t, per: (t if per else t[0]).contiguous()
    return cls(pick(lo, per_band), pick(hi, per_band), pick(w, per_w), **kw)


def zero_weights(obj, **kw):
    return PD(obj.lo, obj.hi, torch.zeros_like(obj.weight), **kw)


class _Watch(PD):
    """The oracle's callable: the objective, noting what ``_conditions`` asserts."""
    def __call__(self, pos):
        r = _dist(pos, self.n_bodies)
        on = (self.weight > 0).expand(r.shape)
        if not hasattr(self, "seen"):
            act = on & ((r < self.lo.double()) | (r > self.hi.double()))
            self.seen, self.min_r, self.first_share = 0, INF, float(act.sum()) / float(on.sum())
        self.seen += 1
        self.min_r = min(self.min_r, float(r[on].min()))
        return super().__call__(pos)


class _NeverCalled(PD):
    def __call__(self, pos):
        raise AssertionError("the built-in route evaluated the objective in Python")


def _conditions(name, watch):
    """The conditions on a case's tables, from what the oracle's run of it saw."""
    _say(f"{name}: states seen", float(watch.seen))
    assert _say(f"{name}: smallest weighted distance", watch.min_r) > 1e-3
    assert 0.25 <= _say(f"{name}: active share at the start", watch.first_share) <= 0.75
    lo, hi, on = torch.broadcast_tensors(watch.lo, watch.hi, watch.weight > 0)
    assert bool((torch.isinf(hi) & on).any()) and bool(((lo == 0) & on).any()) and bool(((lo == hi) & on).any())


def _moved(name, obj, ref, ref0):
    """The guards of a chain case, on the oracle's result ``ref`` and its zero-weight result ``ref0``."""
    _not_degenerate(obj, ref)
    assert float(ref.abs().max()) < 100.0
    assert _say(f"{name}: objective moved the oracle's result by", rel(ref, ref0)) > 100 * TOL_CHAIN


# ------------------------------------------------------------------ 1. one guided step against the oracle
# (guidance, tc, band per design, weight per design, initial_state_overwrite, n_bodies): both guidances with and without recurrence,
# each of the four per-design combinations twice, tc and the overwrite in half of the cases each, 2, 3 and 4 bodies (P = 1, 3, 6: the
# pair order and the ascending sum show from 3)
STEP_CASES = [("standard", 0.0, False, False, False, 2), ("standard", 0.5, True, True, True, 3),
              ("standard-alpha", 0.5, True, False, False, 4), ("standard-alpha", 0.0, False, True, True, 2),
              ("standard-recurrence-2", 0.5, False, False, True, 4), ("standard-recurrence-2", 0.0, False, True, False, 3),
              ("standard-alpha-recurrence-3", 0.0, True, True, True, 2), ("standard-alpha-recurrence-3", 0.5, True, False, False, 3)]
STEP_B, STEP_L = 2, 56


def step_kw(nb):
    return dict(compose_mode="mean-inside", n_composed=2, compose_start_step=16, single_model_step=HZ, compose_n_bodies=nb)


def step_inputs(guid, use_iso, nb):
    """[(t, x, step noise, relaxation noise, overwrite)] of a step case: t = 600, 30, 0."""
    R = int(guid.split("-")[-1]) if "recurrence" in guid else 0
    g = torch.Generator().manual_seed(21 + nb)
    shape = (STEP_B, STEP_L, 4 * nb)
    out = []
    for t in (600, 30, 0):
        x = torch.randn(shape, generator=g) * 0.7
        nz = torch.randn(shape, generator=g)
        rn = torch.randn((max(R, 1),) + shape, generator=g)
        iso = torch.randn((STEP_B, 4, 4 * nb), generator=g) * 0.3 if use_iso else None
        out.append((t, x, nz, rn, iso))
    return R, out


def step_objective(guid, tc, per_band, per_w, use_iso, nb, x, cls=PD):
    R = int(guid.split("-")[-1]) if "recurrence" in guid else 0
    return make_pairdist(11, x, nb, per_band, per_w, None if R else 1.0, cls=cls, time_consistency_coef=tc)


def step_refs(od, guid, tc, per_band, per_w, use_iso, nb):
    """[(reference, unguided reference where the case compares with it)] of a step case, from the oracle; every step's tables are
    made for its own state and pass ``_conditions``."""
    R, inputs = step_inputs(guid, use_iso, nb)
    refs = []
    for t, x, nz, rn, iso in inputs:
        watch = step_objective(guid, tc, per_band, per_w, use_iso, nb, x, cls=_Watch)
        ref, _ = O.p_sample_compose_inside(od, x.clone(), None, t, nz, design_fn=watch, design_guidance=guid, recur_noise=rn,
                                           initial_state_overwrite=iso, **step_kw(nb))
        _conditions(f"step {guid} nb={nb} t={t}", watch)
        ung = None
        if R == 0 and t == 600:
            ung, _ = O.p_sample_compose_inside(od, x.clone(), None, t, nz, design_guidance=guid, initial_state_overwrite=iso, **step_kw(nb))
        refs.append((ref, ung))
    return refs


@pytest.mark.parametrize("guid,tc,per_band,per_w,use_iso,nb", STEP_CASES)
def test_step_vs_oracle(device, unet8, diff8, guid, tc, per_band, per_w, use_iso, nb):
    """One guided reverse step (3 windows, mean-inside, L_tot = 56) at t = 600, 30, 0; the overwrite covers rows 0 .. 3, of which rows
    0 and 2 carry terms."""
    _, sd = unet8
    B, L, F = STEP_B, STEP_L, 4 * nb
    od = O.Diffusion1D(sd, image_size=HZ, conditioned_steps=0)
    R, inputs = step_inputs(guid, use_iso, nb)
    refs = step_refs(od, guid, tc, per_band, per_w, use_iso, nb)
    desc = diff8._desc_for((B, L, F), "mean-inside", 2, 16, HZ, nb)
    for (t, x, nz, rn, iso), (ref, unguided) in zip(inputs, refs):
        obj = step_objective(guid, tc, per_band, per_w, use_iso, nb, x, cls=_NeverCalled)
        assert bool(torch.isfinite(ref).all())
        if R == 0 and t == 600:           # the gradient moves the step by far more than the tolerance
            assert _say(f"step {guid} t={t}: gradient moved the step by", rel(unguided, ref)) > 100 * TOL_STEP
        step = torch.zeros((1000, B, L, F)); step[t] = nz
        rec = torch.zeros((1000, max(R, 1), B, L, F)); rec[t] = rn
        tape = cindm_amd.NoiseTape(None, step, rec).to(device)
        out = diff8._run_guided_loop(x.clone().to(device), None, desc, obj.descriptor(guid), t, t, noise=tape, seed=0, sample_offset=0,
                                     inpaint_cond=None, initial_state_overwrite=None if iso is None else iso.to(device), tables=obj)
        assert _say(f"step {guid} nb={nb} tc={tc} t={t}", rel(out, ref)) < TOL_STEP, (guid, t)


# ------------------------------------------------------------------ 2. short whole chains against the oracle
DDPM_KW = dict(n_composed=1, compose_start_step=16, compose_mode="mean-inside", design_guidance="standard-recurrence-2", t_stop=985,
               compose_n_bodies=3)


def ddpm_case():
    """t = 999 .. 985, B = 3, three bodies, one composed window more (L_tot = 40, cs = 16), per-design tables, tc = 0.25."""
    B, L, nb = 3, 40, 3
    tape = O.NoiseTape.make(92, (B, L, 4 * nb), 1000, recur=2)
    return B, L, nb, dict(time_consistency_coef=0.25), tape


def ddpm_refs(od):
    B, L, nb, okw, tape = ddpm_case()
    watch = make_pairdist(31, tape.init, nb, cls=_Watch, **okw)
    ref = O.sample(od, B, tape, design_fn=watch, **DDPM_KW)
    _conditions("ddpm chain", watch)
    return watch, ref, O.sample(od, B, tape, design_fn=zero_weights(watch, **okw), **DDPM_KW)


def test_ddpm_chain_vs_oracle(device, unet8, diff8):
    _, sd = unet8
    B, L, nb, okw, tape = ddpm_case()
    plain, ref, ref0 = ddpm_refs(O.Diffusion1D(sd, image_size=HZ, conditioned_steps=0))
    _moved("ddpm chain", plain, ref, ref0)
    obj = make_pairdist(31, tape.init, nb, cls=_NeverCalled, **okw)
    out = diff8.sample(batch_size=B, design_fn=obj, noise=cindm_amd.NoiseTape(tape.init, tape.step, tape.recur), **DDPM_KW)
    assert tuple(out.shape) == (B, L, 4 * nb)
    assert _say("ddpm chain vs oracle", rel(out, ref)) < TOL_CHAIN


# name -> (eta, guidance, n_bodies, tc, band per design, weight per design, iso rows, inpaint rows)
DDIM_CASES = {
    "nb2": (0.0, "standard-recurrence-2", 2, 0.0, True, True, 0, 0),
    "nb4": (0.0, "standard-recurrence-2", 4, 0.0, True, True, 0, 0),
    "nb3_alpha_r1": (0.3, "standard-alpha-recurrence-1", 3, 0.0, False, True, 0, 0),
    "nb2_iso": (0.0, "standard-recurrence-2", 2, 0.5, True, False, 3, 0),
    "nb2_inpaint": (0.5, "standard-recurrence-2", 2, 0.0, True, True, 0, 4),
}


def ddim_case(name):
    """(S, eta, shape, table arguments, objective kwargs, sample kwargs, tape, cond, iso) of a DDIM chain case: S = 10, B = 2, L = 24."""
    eta, guid, nb, tc, per_band, per_w, iso_rows, inp_rows = DDIM_CASES[name]
    S, B, R, F = 10, 2, int(guid.split("-")[-1]), 4 * nb
    shape = (B, HZ, F)
    g = torch.Generator().manual_seed(700 + len(name))
    iso = torch.randn((B, iso_rows, F), generator=g) * 0.3 if iso_rows else None
    cond = torch.rand((B, inp_rows, F), generator=g) * 2 - 1 if inp_rows else None
    tp = _tape(7100 + len(name), shape, S, R, None if cond is None else tuple(cond.shape))
    kw = dict(n_composed=0, compose_mode="mean-inside", design_guidance=guid, **({"compose_n_bodies": nb} if nb != 2 else {}))
    return S, eta, shape, (41 + nb, tp["init"], nb, per_band, per_w), dict(time_consistency_coef=tc), kw, tp, cond, iso


def ddim_refs(od, name):
    """(objective, oracle result, zero-weight oracle result) of a DDIM chain case."""
    S, eta, shape, targs, okw, kw, tp, cond, iso = ddim_case(name)
    watch = make_pairdist(*targs, cls=_Watch, **okw)
    run = lambda fn: O.ddim_sample(od, shape, cond, tp, sampling_timesteps=S, eta=eta, design_fn=fn, initial_state_overwrite=iso, **kw)
    ref = run(watch)
    _conditions(f"ddim {name}", watch)
    return watch, ref, run(zero_weights(watch, **okw))


@pytest.mark.parametrize("name", sorted(DDIM_CASES))
def test_ddim_chain_vs_oracle(device, unet8, name):
    S, eta, shape, targs, okw, kw, tp, cond, iso = ddim_case(name)
    m, sd = unet8
    obj = make_pairdist(*targs, cls=_NeverCalled, **okw)
    plain, ref, ref0 = ddim_refs(O.Diffusion1D(sd, image_size=HZ, conditioned_steps=0), name)
    _moved(f"ddim {name}", plain, ref, ref0)
    d = _ddim(device, m, S, eta)
    dev = lambda t: None if t is None else t.to(device)
    out = d.ddim_sample(shape, dev(cond), design_fn=obj, initial_state_overwrite=dev(iso), noise=_nt(tp), **kw)
    assert tuple(out.shape) == shape
    assert _say(f"ddim {name} vs oracle", rel(out, ref)) < TOL_CHAIN


MS_KW = dict(n_composed=0, compose_mode="mean-inside", design_guidance="standard-recurrence-2", compose_n_bodies=3)


def test_ddim_chain_with_the_multistep_solver(device, unet8):
    """compose_update_pair_kernel<true>: three bodies, S = 10, against the route that loops in Python (module docstring); the watch runs
    on that route, on the device's states."""
    m, _ = unet8
    shape = (2, HZ, 12)
    tp = _tape(7300, shape, 10, 2)
    d = _ddim(device, m, 10)
    watch = make_pairdist(51, tp["init"], 3, cls=_Watch)
    slow = d.ddim_sample(shape, None, design_fn=lambda x: watch(x), noise=_nt(tp), solver="dpmpp-2m", **MS_KW)
    _conditions("ddim multistep", watch)
    obj = make_pairdist(51, tp["init"], 3, cls=_NeverCalled)
    fast = d.ddim_sample(shape, None, design_fn=obj, noise=_nt(tp), solver="dpmpp-2m", **MS_KW)
    plain = d.ddim_sample(shape, None, design_fn=obj, noise=_nt(tp), **MS_KW)
    zero = d.ddim_sample(shape, None, design_fn=zero_weights(obj), noise=_nt(tp), solver="dpmpp-2m", **MS_KW)
    assert bool(torch.isfinite(slow).all()) and float(slow.abs().max()) < 100.0
    assert _say("multistep routes", rel(fast, slow)) < TOL_CHAIN
    assert _say("multistep vs ddim", rel(fast, plain)) > 100 * TOL_CHAIN
    assert _say("multistep: objective moved the result by", rel(fast, zero)) > 100 * TOL_CHAIN


# ------------------------------------------------------------------ 3. built-in route equals generic route
def test_builtin_route_equals_generic_route(device, unet8, diff8):
    m, _ = unet8
    B, nb = 3, 3
    d = _ddim(device, m, 10, 0.4)
    tp = _tape(7400, (B, HZ, 4 * nb), 10, 3)
    obj = make_pairdist(71, tp["init"], nb, time_consistency_coef=0.25)
    never = make_pairdist(71, tp["init"], nb, cls=_NeverCalled, time_consistency_coef=0.25)
    # (ddim_sample with the state's shape: sample() sizes the state by the model's 8 channels)
    shape = (B, HZ, 4 * nb)
    kw = dict(n_composed=0, compose_mode="mean-inside", design_guidance="standard-recurrence-3", compose_n_bodies=nb)
    fast = d.ddim_sample(shape, None, design_fn=never, noise=_nt(tp), **kw)
    slow = d.ddim_sample(shape, None, design_fn=lambda x: obj(x), noise=_nt(tp), **kw)
    assert bool(torch.isfinite(slow).all())
    assert _say("routes ddim", rel(fast, slow)) < TOL_CHAIN
    tape = O.NoiseTape.make(94, (B, 40, 8), 1000, recur=2)
    obj40 = make_pairdist(72, tape.init, 2, time_consistency_coef=0.25)
    never40 = make_pairdist(72, tape.init, 2, cls=_NeverCalled, time_consistency_coef=0.25)
    kw = dict(batch_size=B, n_composed=1, compose_start_step=16, compose_mode="mean-inside", design_guidance="standard-recurrence-2",
              noise=cindm_amd.NoiseTape(tape.init, tape.step, tape.recur), t_stop=992)
    fast = diff8.sample(design_fn=never40, **kw)
    slow = diff8.sample(design_fn=lambda x: obj40(x), **kw)
    assert bool(torch.isfinite(slow).all())
    assert _say("routes ddpm", rel(fast, slow)) < TOL_CHAIN
    with pytest.raises(AssertionError, match="in Python"):        # the generic routes do call it
        d.ddim_sample(shape, None, design_fn=never, seed=11, n_composed=0, compose_mode="mean-inside", compose_n_bodies=nb,
                      design_guidance="universal-forward-recurrence-2")


# ------------------------------------------------------------------ 4. the quadratic branch agrees on at(0)
def at_zero_pair(L, nb, B, seed, tc):
    """(at(0) objective, its QuadraticObjective restatement): w r^2 = 1/2 (2 w) ((x_i - x_j)^2 + (y_i - y_j)^2), weights that are
    multiples of 1/64 (the quadratic tables hold sums of them, exact in fp32)."""
    g = torch.Generator().manual_seed(seed)
    P = nb * (nb - 1) // 2
    w = torch.randint(4, 13, (B, L, P), generator=g).float() / 64 * (torch.rand((B, L, P), generator=g) > 0.3)
    rows, A, wt = [], [], []
    for l in range(L):
        for p, (i, j) in enumerate(_pairs(nb)):
            for c in (0, 1):
                a = torch.zeros(4 * nb, dtype=torch.float64)
                a[4 * i + c], a[4 * j + c] = 1.0, -1.0
                rows.append(l); A.append(a); wt.append(2.0 * w[:, l, p].double())
    quad = cindm_amd.QuadraticObjective.from_residuals(rows, torch.stack(A), torch.zeros(len(rows)), torch.stack(wt, dim=1), L, 4 * nb,
                                                       time_consistency_coef=tc)
    return PD.at(0.0, w, time_consistency_coef=tc), quad


def test_at_zero_chains_equal_their_quadratic_restatement(device, unet8, diff8):
    """((((w 2) r) d) / r against the quadratic branch's sum over the row: the same chain within TOL_STEP, not bitwise.  The chains are
    two steps of two iterations each (four U-Net evaluations, two of them behind a gradient).  The two expressions differ by 1.2e-7
    on a state of order 1 -- the quadratic branch forms (2 w_a + 2 w_b) x_i - 2 w_a x_a - 2 w_b x_b, which cancels where at(0) has pulled
    the bodies together.  Restated in torch and run through the CPU oracle, that difference is 1e-6 after the two DDIM steps used here
    and 4e-3 after six (the synthetic U-Net amplifies it; closed form against autograd of the one objective: 2e-3 after six): a
    longer chain measures the U-Net, not the two branches."""
    m, _ = unet8
    B, nb = 2, 3
    a0, q0 = at_zero_pair(HZ, nb, B, 61, 0.25)
    d = _ddim(device, m, 2, 0.3)
    tp = _tape(7500, (B, HZ, 4 * nb), 2, 2)
    kw = dict(n_composed=0, compose_mode="mean-inside", design_guidance="standard-recurrence-2", compose_n_bodies=nb)
    run = lambda fn: d.ddim_sample((B, HZ, 4 * nb), None, design_fn=fn, noise=_nt(tp), **kw)       # (sample() sizes the state by the model's 8 channels)
    a, q, z = run(a0), run(q0), run(zero_weights(a0, time_consistency_coef=0.25))
    assert bool(torch.isfinite(a).all()) and _say("at(0) ddim: objective moved the result by", rel(a, z)) > 100 * TOL_CHAIN
    assert _say("at(0) ddim vs quadratic branch", rel(a, q)) < TOL_STEP
    a1, q1 = at_zero_pair(40, 2, B, 62, 0.0)
    tape = O.NoiseTape.make(95, (B, 40, 8), 1000, recur=2)
    kw = dict(batch_size=B, n_composed=1, compose_start_step=16, compose_mode="mean-inside", design_guidance="standard-recurrence-2",
              noise=cindm_amd.NoiseTape(tape.init, tape.step, tape.recur), t_stop=998)
    a, q, z = diff8.sample(design_fn=a1, **kw), diff8.sample(design_fn=q1, **kw), diff8.sample(design_fn=zero_weights(a1), **kw)
    assert bool(torch.isfinite(a).all()) and _say("at(0) ddpm: objective moved the result by", rel(a, z)) > 100 * TOL_CHAIN
    assert _say("at(0) ddpm vs quadratic branch", rel(a, q)) < TOL_STEP


# ------------------------------------------------------------------ 5. bitwise by construction
def test_zero_weights_equal_a_zero_weight_waypoint_objective(device, unet8, diff8):
    m, _ = unet8
    B = 2
    d = _ddim(device, m, 10, eta=0.5)
    kw = dict(batch_size=B, n_composed=0, compose_mode="mean-inside", design_guidance="standard-alpha-recurrence-2", seed=17)
    x0 = torch.randn((B, HZ, 8), generator=torch.Generator().manual_seed(3))
    zero = zero_weights(make_pairdist(60, x0, 2), time_consistency_coef=0.25)
    target, weight = make_tables(41, HZ, 2, B, True, True)
    way = cindm_amd.WaypointObjective(target, torch.zeros_like(weight), time_consistency_coef=0.25)
    out = d.sample(design_fn=zero, **kw)
    assert bool(torch.isfinite(out).all()) and torch.equal(out, d.sample(design_fn=way, **kw))
    kw = dict(batch_size=B, n_composed=1, compose_start_step=16, compose_mode="mean-inside", design_guidance="standard", seed=12, t_stop=994)
    x0 = torch.randn((B, 40, 8), generator=torch.Generator().manual_seed(4))
    zero = zero_weights(make_pairdist(60, x0, 2))
    target, weight = make_tables(41, 40, 2, B, True, True)
    way = cindm_amd.WaypointObjective(target, torch.zeros_like(weight))
    assert torch.equal(diff8.sample(design_fn=zero, **kw), diff8.sample(design_fn=way, **kw))


def test_broadcast_equals_materialised(device, unet8):
    m, _ = unet8
    B, nb = 3, 3
    d = _ddim(device, m, 10, eta=0.5)
    x0 = torch.randn((1, HZ, 4 * nb), generator=torch.Generator().manual_seed(5))
    lo, hi, w = (t[0] for t in pair_tables(61, x0, nb, 0.5 / nb))
    kw = dict(n_composed=0, compose_mode="mean-inside", design_guidance="standard-recurrence-2", seed=17, compose_n_bodies=nb)
    run = lambda ll, hh, ww: d.ddim_sample((B, HZ, 4 * nb), None, design_fn=PD(ll, hh, ww, time_consistency_coef=0.25), **kw)
    shared = run(lo, hi, w)
    assert bool(torch.isfinite(shared).all())
    assert not torch.equal(shared, run(lo, hi, torch.zeros_like(w)))
    e = lambda t: t.expand(B, -1, -1).contiguous()
    for ll, hh, ww in ((e(lo), e(hi), e(w)), (e(lo), hi, w), (lo, e(hi), w), (lo, hi, e(w))):
        assert torch.equal(run(ll, hh, ww), shared)


def test_library_chain_properties(device, unet8, diff8):
    """The objective's Python side is never evaluated; graph == stream; two half-batches with shard + sample_offset == the whole batch
    (counter-based draws), through sample_sharded's own path as well."""
    m, _ = unet8
    B = 4
    d = _ddim(device, m, 9, eta=1.0)            # (9 steps x 3 iterations: odd, the result lands in the workspace buffer)
    x0 = torch.randn((B, HZ, 8), generator=torch.Generator().manual_seed(6))
    obj = make_pairdist(81, x0, 2, cls=_NeverCalled)
    kw = dict(n_composed=0, compose_mode="mean-inside", design_guidance="standard-recurrence-3")
    whole = d.sample(batch_size=B, design_fn=obj, seed=11, **kw)
    assert bool(torch.isfinite(whole).all())
    assert torch.equal(whole, d.sample(batch_size=B, design_fn=obj, seed=11, use_graph=False, **kw))
    parts = [d.sample(batch_size=hi - lo, design_fn=obj.shard(lo, hi), seed=11, sample_offset=lo, **kw) for lo, hi in ((0, 2), (2, 4))]
    assert torch.equal(torch.cat(parts), whole)
    assert not torch.equal(parts[0], parts[1])
    assert torch.equal(cdist.sample_sharded(d, B, seed=11, design_fn=obj, **kw), whole)
    x0 = torch.randn((B, 40, 8), generator=torch.Generator().manual_seed(7))
    obj40 = make_pairdist(82, x0, 2, cls=_NeverCalled)
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
    x0 = torch.randn((2, HZ, 8), generator=torch.Generator().manual_seed(8))
    A, B_ = (make_pairdist(seed, x0, 2) for seed in (91, 92))
    a1 = d.sample(design_fn=A, **kw).clone()
    b = d.sample(design_fn=B_, **kw).clone()
    a2 = d.sample(design_fn=A, **kw)
    (ba, wa), (bb, wb) = A.tables(device), B_.tables(device)
    assert ba.data_ptr() != bb.data_ptr() and wa.data_ptr() != wb.data_ptr()
    assert torch.equal(a1, a2) and not torch.equal(a1, b)
    # B's designs are those of a handle that has never seen A
    assert torch.equal(b, _ddim(device, m, 6, eta=0.5).sample(design_fn=make_pairdist(92, x0, 2), **kw))


# ------------------------------------------------------------------ 6. with the recorder and a known region
def test_recorder_and_known_region(device, unet8, diff8):
    m, _ = unet8
    d = _ddim(device, m, 10, eta=0.5)
    g = torch.Generator().manual_seed(8)

    def region(L):
        known = torch.rand((L, 8), generator=g) * 1.2 - 0.6
        mask = torch.zeros((L, 8), dtype=torch.bool)
        mask[1] = True                    # a row without terms, whole
        mask[L - 1, 4:6] = True           # the positions of body 1 on the last row, which carries terms: the pair is half known
        return known, mask

    known, mask = region(HZ)
    obj = make_pairdist(95, torch.randn((2, HZ, 8), generator=g), 2, cls=_NeverCalled)
    kw = dict(batch_size=2, n_composed=0, compose_mode="mean-inside", design_fn=obj, design_guidance="standard-recurrence-2", seed=7,
              known=known, known_mask=mask)
    out, rec = d.sample(return_trajectory_every=3, trajectory=("x", "x0"), **kw)
    assert rec.step == [3, 6, 9, 10] and tuple(rec.x.shape) == (4, 2, HZ, 8) == tuple(rec.x0.shape)
    assert torch.equal(rec.x[-1], out) and torch.equal(out, d.sample(**kw))
    assert torch.equal(out.cpu()[:, mask], known[mask].expand(2, -1))
    assert not torch.equal(out, d.sample(**dict(kw, known=None, known_mask=None)))
    assert not torch.equal(out, d.sample(**dict(kw, design_fn=zero_weights(obj))))
    obj40 = make_pairdist(96, torch.randn((2, 40, 8), generator=g), 2, cls=_NeverCalled)
    kw = dict(batch_size=2, n_composed=1, compose_start_step=16, compose_mode="mean-inside", design_fn=obj40,
              design_guidance="standard-recurrence-2", seed=7, t_stop=993)
    out, rec = diff8.sample(return_trajectory_every=3, trajectory=("x", "x0"), **kw)
    assert rec.t == [997, 994, 993] and torch.equal(rec.x[-1], out) and torch.equal(out, diff8.sample(**kw))


# ------------------------------------------------------------------ 7. refusals
def test_refusals_leave_the_handle_usable(device, unet8, diff8):
    B, L = 2, 40
    x0 = torch.randn((B, L, 8), generator=torch.Generator().manual_seed(1))
    obj = make_pairdist(97, x0, 2)
    point = cindm_amd.PointObjective([0.25, -0.5], 2, coef=2.0)
    way = cindm_amd.WaypointObjective(*make_tables(97, L, 2, B, True, True), coef=2.0)
    quad = make_quadratic(97, L, 8, B)
    guid = "standard-recurrence-2"
    desc = diff8._desc_for((B, L, 8), "mean-inside", 1, 16, HZ, 2)
    xd = x0.to(device)
    run = lambda dz, tables: diff8._run_guided_loop(xd.clone(), None, desc, dz, 999, 998, noise=None, seed=3, sample_offset=0,
                                                    inpaint_cond=None, initial_state_overwrite=None, tables=tables)
    h = diff8._handle()
    good = run(obj.descriptor(guid), obj)
    good_way, good_quad = run(way.descriptor(guid), way), run(quad.descriptor(guid), quad)
    assert bool(torch.isfinite(good).all()) and not torch.equal(good, good_way) and not torch.equal(good, good_quad)

    def still_good():
        assert torch.equal(run(obj.descriptor(guid), obj), good)

    with pytest.raises(cindm_amd.CindmError, match="arm them with cindm_ddpm1d_set_design_pairdist"):
        run(obj.descriptor(guid), None)                                  # mode 6, nothing armed
    still_good()
    with pytest.raises(cindm_amd.CindmError, match="pair-distance design tables are armed but the descriptor's mode is 1 .. 5"):
        run(point.descriptor(guid), obj)                                 # armed pair-distance tables, point descriptor (mode 1)
    still_good()
    obj.arm(h, B, device)
    with pytest.raises(cindm_amd.CindmError, match="pair-distance design tables are armed but the descriptor's mode is 1 .. 5"):
        run(way.descriptor(guid), way)                                   # both armed, waypoint descriptor (mode 3)
    assert torch.equal(run(way.descriptor(guid), way), good_way)
    still_good()
    obj.arm(h, B, device)
    with pytest.raises(cindm_amd.CindmError, match="pair-distance design tables are armed but the descriptor's mode is 1 .. 5"):
        run(quad.descriptor(guid), quad)                                 # both armed, quadratic descriptor (mode 5)
    assert torch.equal(run(quad.descriptor(guid), quad), good_quad)
    still_good()
    way.arm(h, B, device)
    with pytest.raises(cindm_amd.CindmError, match=r"design tables \(target, scale\) are armed but the descriptor's mode is 6"):
        run(obj.descriptor(guid), obj)                                   # waypoint tables under mode 6
    still_good()
    quad.arm(h, B, device)
    with pytest.raises(cindm_amd.CindmError, match="quadratic design tables are armed but the descriptor's mode is 6"):
        run(obj.descriptor(guid), obj)                                   # quadratic tables under mode 6
    still_good()
    with pytest.raises(cindm_amd.CindmError, match="the descriptor's mode is 6"):
        run(obj.descriptor(guid), way)                                   # waypoint tables alone under mode 6
    still_good()
    wrong = make_pairdist(97, torch.randn((B, L + 16, 8), generator=torch.Generator().manual_seed(2)), 2)
    x12 = torch.randn((B, L, 12), generator=torch.Generator().manual_seed(2))
    with pytest.raises(cindm_amd.CindmError, match="56 rows, the state has 40"):
        run(wrong.descriptor(guid), wrong)                               # the library's own checks
    with pytest.raises(cindm_amd.CindmError, match="3 bodies, the composition has 2"):
        run(obj.descriptor(guid), make_pairdist(97, x12, 3))
    with pytest.raises(cindm_amd.CindmError, match="batch of 3"):
        run(obj.descriptor(guid), make_pairdist(97, torch.cat([x0, x0[:1]]), 2))
    still_good()
    kw = dict(batch_size=B, n_composed=1, compose_start_step=16, compose_mode="mean-inside", design_guidance=guid, seed=3, t_stop=998)
    for bad in (wrong, make_pairdist(97, x12, 3), make_pairdist(97, torch.cat([x0, x0[:1]]), 2)):
        with pytest.raises(ValueError, match="PairDistanceObjective"):   # the public route refuses before any device work
            diff8.sample(design_fn=bad, **kw)
    # armed tables on a chain that is not guided: refused with the reason, consumed, and the next unguided chain runs
    obj.arm(h, B, device)
    with pytest.raises(cindm_amd.CindmError, match="pair-distance design tables: only the guided 1-D chains"):
        diff8.sample(batch_size=B, n_composed=0, seed=3, t_stop=998)
    assert bool(torch.isfinite(diff8.sample(batch_size=B, n_composed=0, seed=3, t_stop=998)).all())
    m, _ = unet8
    dd = _ddim(device, m, 5)
    obj.arm(dd._handle(), B, device)
    with pytest.raises(cindm_amd.CindmError, match="pair-distance design tables: only the guided 1-D chains"):
        dd.sample(batch_size=B, n_composed=0, seed=3)                    # the unguided DDIM chain
    assert bool(torch.isfinite(dd.sample(batch_size=B, n_composed=0, seed=3)).all())
    band, wt = obj.tables(device)
    lib = _ffi.lib()
    assert lib.cindm_ddpm1d_set_design_pairdist(h, _ffi.ptr(band), 1, None, 1, L, 2, B) != 0           # one table without the other
    assert lib.cindm_ddpm1d_set_design_pairdist(h, _ffi.ptr(band), 1, _ffi.ptr(wt), 1, L, 1, B) != 0   # one body has no pair
    assert lib.cindm_ddpm1d_set_design_pairdist(h, _ffi.ptr(band), 1, _ffi.ptr(wt), 1, L, 9, B) != 0   # more than 8
    assert lib.cindm_ddpm1d_set_design_pairdist(h, _ffi.ptr(band), 1, _ffi.ptr(wt), 1, 0, 2, B) != 0
    _ffi.check(lib.cindm_ddpm1d_set_design_pairdist(h, _ffi.ptr(band), 1, _ffi.ptr(wt), 1, L, 2, B))
    _ffi.check(lib.cindm_ddpm1d_set_design_pairdist(h, None, 0, None, 0, 0, 0, 0))                    # disarm
    assert bool(torch.isfinite(diff8.sample(batch_size=B, n_composed=0, seed=3, t_stop=998)).all())
    still_good()
    assert bool(torch.isfinite(diff8.sample(design_fn=obj, **kw)).all())


def _armed_refusal(d, run, device):
    """Arms the handle directly, issues ``run`` (a chain entry that does not read the tables): it must fail with the tables' message, and
    the same call must pass afterwards -- the refused call consumed the tables."""
    band, wt = torch.zeros((2, 4, 1, 2), device=device), torch.ones((2, 4, 1), device=device)
    _ffi.check(_ffi.lib().cindm_ddpm1d_set_design_pairdist(d._handle(), _ffi.ptr(band), 1, _ffi.ptr(wt), 1, 4, 2, 2))
    with pytest.raises(cindm_amd.CindmError, match="pair-distance design tables: only the guided 1-D chains"):
        run()
    out = run()
    out = out[0] if isinstance(out, tuple) else out
    assert bool(torch.isfinite(out).all())


def test_other_1d_entries_refuse_armed_tables(device, unet8):
    m, _ = unet8
    d = _ddim(device, m, 1000)
    _armed_refusal(d, lambda: d.sample(batch_size=2, seed=1, t_stop=998), device)                          # cindm_ddpm1d_sample
    d5 = _ddim(device, m, 3)
    _armed_refusal(d5, lambda: d5.sample(batch_size=2, seed=1, n_composed=0), device)                      # _sample_ddim
    mh, _ = build_unet(device, 8, 8)
    dh = cindm_amd.GaussianDiffusion1D(mh, image_size=4, conditioned_steps=4, timesteps=1000, sampling_timesteps=3,
                                       loss_type="l1").to(device)
    cond = (torch.rand((2, 4, 8), generator=torch.Generator().manual_seed(1)) - 0.5).to(device)
    _armed_refusal(dh, lambda: dh.autoregress_time_compose_sample(2, cond, 1, seed=1), device)             # _sample_autoregress
    _armed_refusal(dh, lambda: dh.composing_time_sample((2, 4, 8), cond, n_composed=1, seed=1), device)    # _sample_timecompose
    m8, m4 = build_unet(device, U.HZ, 8)[0], build_unet(device, U.HZ, 4)[0]
    N = 1000
    du = cindm_amd.GaussianDiffusion1D(m8, image_size=U.R, conditioned_steps=U.LC, timesteps=1000, sampling_timesteps=1000,
                                       loss_type="l1", betas_inference=U.linear_beta_schedule(N)).to(device)
    du.model_unconditioned = m4
    x = torch.randn((2, U.HZ, U.F), generator=torch.Generator().manual_seed(2)).to(device)
    scalar = U.scalar_for_gradient(U.linear_beta_schedule(N))
    _armed_refusal(du, lambda: du.sample_step_ULA(x, torch.tensor([731, 731]), 1, 4, N, scalar, seed=1), device)   # _sample_ula


def test_2d_entries_refuse_armed_tables(device):
    unet2d = build_unet2d(device)
    sd = O.synth_state_dict_2d(O.force_unet_param_shapes(), 7)
    force = cindm_amd.ForceUnet(dim=64, dim_mults=(1, 2, 4, 8), channels=4)
    force.load_state_dict(sd, strict=True)
    force = force.to(device)
    shape = (1, 2, CH, HW, HW)
    fn = _force_objective(force, 1, 2)
    d = _diff2(device, unet2d, 1000)
    _armed_refusal(d, lambda: d.p_sample_loop(shape, seed=1, t_stop=998), device)                          # cindm_ddpm2d_sample
    _armed_refusal(d, lambda: d.p_sample_loop(shape, fn, "standard-alpha", seed=1, t_stop=998), device)    # _sample_force
    d2 = _diff2(device, unet2d, 2)
    _armed_refusal(d2, lambda: d2.ddim_sample(shape, seed=1), device)                                      # _sample_ddim
    _armed_refusal(d2, lambda: d2.ddim_sample(shape, fn, "standard-alpha", seed=1), device)                # _sample_ddim_force
