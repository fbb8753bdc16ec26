"""The grid of the 1-D step tail, shared by tests/test_step1d_f64_host.py (the fp32 oracle against the float64 statement) and
tests/test_gpu_step1d_f64.py (the library against it).  No GPU and no library call in here: states, draws, tables and the list of cases.

Shapes are the smallest at which each branch is distinct: one window of 24 rows, or two with compose_start_step = 16 (Ltot = 40,
mean-inside; the DDPM forms only -- a DDIM chain's state is one window); 2, 3 and 4 bodies (P = 1, 3, 6 pairs); B = 2, or 3 where
per-design and shared tables must differ.  B * Ltot * F is 384, 864, 1152, 1440 or 1920: none a multiple of the update's 256 threads.

What is discontinuous in the inputs is a condition asserted here on the float64 values (``check_conditions``), not a tolerance:
every L2 denominator that counts is >= 0.05; every weighted pair has r >= 0.05 or r == 0 exactly, and r differs from lo and from hi by
more than 1e-3 r.  ``inputs`` tries the seeds ``SEED_STRIDE * k + index`` for k = 0, 1, .. and takes the first that holds them, so
that no element has to be left out; the CPU file asserts that every case finds one within ``SEED_TRIES``."""
import torch

import cindm_amd
import f64_reference as R

WINDOW, CS = 24, 16
X_SCALE = 0.7
ROWS_FIXED = 4                      # rows 0 .. 3: the initial_state_overwrite and the inpainting condition
DDIM_S = 10
DDIM_STEPS = (0, 5, 9)              # the first pair (kappa = 0), a middle one, the last (time_next < 0)
DDPM_T = (600, 30, 1, 0)
KINDS = R.DESIGN_KINDS
LINEAR_KINDS = ("point-L2square", "table-L2square", "quadratic", "tc")      # gradient linear in the state: the two-evaluation cases
OBJECTIVES = ("pred_noise", "pred_x0", "pred_v")
MIN_DEN, MIN_R, MIN_GAP = 0.05, 0.05, 1e-3
SEED_STRIDE, SEED_TRIES = 1000, 64
POINT_TARGET, POINT_ROWS = (0.25, -0.5), 3
# (B, windows, bodies)
LAYOUTS = {"b2w1n2": (2, 1, 2), "b3w2n3": (3, 2, 3), "b3w1n4": (3, 1, 4), "b3w1n3": (3, 1, 3), "b3w2n4": (3, 2, 4)}
DDPM_LAYOUTS = ("b2w1n2", "b3w2n3", "b3w1n4", "b3w2n4")
DDIM_LAYOUTS = ("b2w1n2", "b3w1n3", "b3w1n4")


class Case:
    def __init__(self, index, entry, layout, kind, **kw):
        self.index, self.entry, self.layout, self.kind = index, entry, layout, kind
        self.alpha, self.tc, self.rec, self.t = kw.get("alpha", False), kw.get("tc", 0.0), kw.get("rec", 0), kw.get("t")
        self.step, self.eta, self.objective = kw.get("step"), kw.get("eta", 0.0), kw.get("objective", "pred_noise")
        self.iso, self.inpaint, self.ms, self.frozen = kw.get("iso", False), kw.get("inpaint", False), kw.get("ms", False), kw.get("frozen", False)
        self.B, self.W, self.nb = LAYOUTS[layout]
        self.L, self.F = WINDOW + (self.W - 1) * CS, 4 * self.nb
        assert (self.B * self.L * self.F) % 256 != 0

    @property
    def guidance(self):
        g = "standard-alpha" if self.alpha else "standard"
        return g + (f"-recurrence-{self.rec}" if self.rec else "")

    @property
    def name(self):
        where = f"t{self.t}" if self.entry == "ddpm" else f"s{self.step}-eta{self.eta}"
        bits = [self.entry, self.layout, self.kind or "unguided", self.guidance if self.kind else "", f"tc{self.tc}" if self.kind else "", where,
                self.objective, "iso" if self.iso else "", "inp" if self.inpaint else "", "ms" if self.ms else "", "frozen" if self.frozen else ""]
        return "-".join(b for b in bits if b)

    def desc(self):
        """The compose descriptor of the case: plain for the unguided DDIM chain (it ignores the compose keywords), else mean-inside."""
        mode = "plain" if (self.entry == "ddim" and self.kind is None) else "mean-inside"
        return R.ComposeCase(mode, self.nb, self.W, CS if self.W > 1 else 0, WINDOW, 0, self.objective, True)


def ddim_times():
    """[(time, time_next)] of the S = 10 chain: 999, 899, .., 99, -1."""
    times = list(reversed(torch.linspace(-1, 999, steps=DDIM_S + 1).int().tolist()))
    return list(zip(times[:-1], times[1:]))


def _cases():
    out = []
    add = lambda *a, **k: out.append(Case(len(out), *a, **k))
    # guided DDPM, one evaluation: every kind x guidance scaling x tc x t; recurrence 0 / 1, the layout, the overwrite and the
    # inpainting rows cycle with periods 2, 4, 2 (shifted) and 3, so that every kind meets every one of them at every t
    k = 0
    for kind in KINDS:
        for alpha in (False, True):
            for tc in (0.0, 0.5):
                for t in DDPM_T:
                    add("ddpm", DDPM_LAYOUTS[(k + k // 4) % 4], kind, alpha=alpha, tc=tc, t=t, rec=(k + k // 8) % 2, iso=(k // 2 + k // 16) % 2 == 0,
                        inpaint=k % 3 == 0)
                    k += 1
    # pred_x0 / pred_v on the guided point cases
    for obj in ("pred_x0", "pred_v"):
        for j, t in enumerate(DDPM_T):
            add("ddpm", DDPM_LAYOUTS[j % 2], KINDS[j % 2], alpha=j % 2 == 1, tc=0.5 * (j // 2), t=t, rec=j % 2, objective=obj, iso=j == 1)
    # the unguided DDPM tail with the inpainting rows (the unguided step itself: tests/test_gpu_compose_f64.py)
    for j, t in enumerate(DDPM_T):
        add("ddpm", DDPM_LAYOUTS[j % 2], None, t=t, inpaint=True)
    # the relaxation: two evaluations on the frozen model, gradients linear in the state
    for j, kind in enumerate(LINEAR_KINDS):
        for alpha in (False, True):
            for t in DDPM_T:
                add("ddpm", DDPM_LAYOUTS[(j + t) % 2 + (2 if kind == "quadratic" else 0)], kind, alpha=alpha, tc=0.5 if (kind == "tc" or (j + alpha) % 2) else 0.0,
                    t=t, rec=2, iso=(t in (600, 1)) != alpha, frozen=True)
    # guided DDIM, one evaluation: every kind x scaling x step x eta; tc, the layout, the overwrite, the inpainting rows cycle; the
    # multistep solver (eta = 0 only) on half of those
    k = 0
    for kind in KINDS:
        for alpha in (False, True):
            for step in DDIM_STEPS:
                for eta in (0.0, 0.5):
                    add("ddim", DDIM_LAYOUTS[(k + k // 6) % 3], kind, alpha=alpha, tc=0.5 * ((k // 2 + k // 12) % 2), step=step, eta=eta, rec=1,
                        iso=(k // 3) % 2 == 0, inpaint=(k % 4 == 1 or k % 12 == 8), ms=(eta == 0.0 and (k // 2) % 2 == 0))
                    k += 1
    for obj in ("pred_x0", "pred_v"):
        for j, step in enumerate(DDIM_STEPS):
            add("ddim", DDIM_LAYOUTS[j], KINDS[j % 2], alpha=j == 1, tc=0.5 * (j % 2), step=step, eta=0.5 * (j % 2), rec=1, objective=obj, ms=False)
    # guided DDIM through a relaxation (frozen model)
    for j, kind in enumerate(LINEAR_KINDS):
        for step in (0, 5):
            add("ddim", DDIM_LAYOUTS[(j + step) % 3], kind, alpha=step == 5, tc=0.5 if (kind == "tc" or j % 2) else 0.0, step=step, eta=0.0, rec=2,
                iso=j % 2 == 0, ms=step == 5, frozen=True)
    # unguided DDIM (plain, 8 features: the fused update and compose_update_kernel): objective x step x eta, the solver, the inpainting rows
    k = 0
    for obj in OBJECTIVES:
        for step in DDIM_STEPS:
            for eta in (0.0, 0.5):
                add("ddim", "b2w1n2", None, step=step, eta=eta, objective=obj, ms=(eta == 0.0 and k % 4 == 0), inpaint=k % 3 == 2)
                k += 1
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def select(entry, **kw):
    return [c for c in CASES if c.entry == entry and all(getattr(c, k) == v for k, v in kw.items())]


def frozen_state_dict(sd):
    """The same U-Net with an output that does not depend on its input: eps[b, l, f] = bias[f], distinct per feature."""
    sd = {k: v.clone() for k, v in sd.items()}
    F = sd["final_conv.1.bias"].numel()
    sd["final_conv.1.weight"] = torch.zeros_like(sd["final_conv.1.weight"])
    sd["final_conv.1.bias"] = torch.tensor([0.45 * (f + 1) / F * (-1) ** f for f in range(F)], dtype=torch.float32)
    return sd


# ------------------------------------------------------------------ objectives
def make_objective(case, x, seed, cls=None):
    """The cindm_amd objective of a case, its tables made for the state ``x`` (the pair bands follow tests/test_gpu_pairdist.py's
    recipe: apart / within / at in turn, a quarter of them active on x, a fifth of the weights zero).  Gradients are of the order of
    the state's own update: under standard-alpha the scale is 100 times larger (eta_t is 1e-4 .. 1e-2)."""
    kind, B, L, nb, F = case.kind, case.B, case.L, case.nb, case.F
    g = torch.Generator().manual_seed(seed + 7)
    amp = 100.0 if case.alpha else 1.0
    rnd = lambda *s: torch.rand(s, generator=g)
    if kind in ("point-L2", "point-L2square"):
        return (cls or cindm_amd.PointObjective)(list(POINT_TARGET), POINT_ROWS, coef=0.6 * amp, time_consistency_coef=case.tc,
                                                 design_fn_mode=kind.split("-")[1])
    if kind in ("table-L2", "table-L2square", "tc"):
        per_target = case.index % 2 == 0
        target = rnd(B, L, nb, 2) * 1.6 - 0.8
        weight = (0.1 + 0.3 * rnd(B, L, nb)) * (rnd(B, L, nb) > 0.3)
        if kind == "tc":
            weight = torch.zeros_like(weight)
        return (cls or cindm_amd.WaypointObjective)(target if per_target else target[0], weight[0] if per_target else weight, coef=amp,
                                                    time_consistency_coef=case.tc, design_fn_mode="L2" if kind == "table-L2" else "L2square")
    if kind == "quadratic":
        per_S = case.index % 2 == 0
        M = (rnd(B, L, F, F) * 2 - 1) * (0.3 * amp / F ** 0.5)
        S = (M + M.transpose(-1, -2)) * 0.5
        h = (rnd(B, L, F) * 2 - 1) * 0.2 * amp
        return (cls or cindm_amd.QuadraticObjective)(S if per_S else S[0], h[0] if per_S else h, time_consistency_coef=case.tc)
    assert kind == "pair", kind
    P = nb * (nb - 1) // 2
    pos = x.double().reshape(B, L, nb, 4)[..., :2]
    r0 = torch.stack([(pos[:, :, i] - pos[:, :, j]).square().sum(-1).sqrt() for i, j in R.compose_pairs(nb)], dim=-1).float()
    lo, hi, w = torch.zeros((B, L, P)), torch.full((B, L, P), float("inf")), torch.zeros((B, L, P))
    for b in range(B):
        k = b
        for l in sorted(set(range(0, L, 2)) | {COINCIDENT_ROW, L - 1}):
            for p in range(P):
                active = (k // 3) % 4 == 0
                if k % 3 == 0:
                    lo[b, l, p] = float(r0[b, l, p]) * (1.3 if active else 0.4)
                elif k % 3 == 1:
                    lo[b, l, p], hi[b, l, p] = 0.0, float(r0[b, l, p]) * (0.7 if active else 2.5)
                else:
                    lo[b, l, p] = hi[b, l, p] = float(r0[b, l, p]) * (1.3 if active else 0.7)
                w[b, l, p] = 0.0 if k % 5 == 4 else (0.5 + float(rnd())) * 0.5 / nb * amp
                k += 1
    w[0, COINCIDENT_ROW, 0] = 0.4 * amp                 # the coincident pair counts: its term must be exactly 0
    per_band = case.index % 2 == 0
    if not per_band:                                    # a band shared by every design: made for design 0's distances
        lo, hi = lo[0], hi[0]
    return (cls or cindm_amd.PairDistanceObjective)(lo, hi, w, time_consistency_coef=case.tc)


COINCIDENT_ROW = 5


def tables_of(obj):
    """(kind, tables) of ``f64_reference.design_grad_f64`` for a cindm_amd objective: the fp32 tables the object holds."""
    if isinstance(obj, cindm_amd.PointObjective):
        return "point-" + obj.design_fn_mode, {"target": obj.pos_target, "last_n_step": obj.last_n_step, "coef": obj.coef}
    if isinstance(obj, cindm_amd.WaypointObjective):
        return "table-" + obj.design_fn_mode, {"target": obj.target, "scale": obj.scale}
    if isinstance(obj, cindm_amd.QuadraticObjective):
        return "quadratic", {"S": obj.S, "h": obj.h}
    return "pair", {"lo": obj.lo, "hi": obj.hi, "weight": obj.weight}


def check_conditions(case, x, obj):
    """None when the state and the tables hold the module's conditions, else what fails."""
    kind, tables = tables_of(obj)
    c = R.design_conditions_f64(kind, x, tables, n_bodies=case.nb)
    if "min_den" in c and not c["min_den"] >= MIN_DEN:
        return f"L2 denominator {c['min_den']:.4f}"
    if kind == "pair":
        if not (c["min_r"] >= MIN_R and c["min_gap"] > MIN_GAP):
            return f"pair r {c['min_r']:.4f}, gap {c['min_gap']:.2e}"
        if c["coincident"] < 1 or c["active"] < 8:
            return f"pair: {c['coincident']} coincident, {c['active']} active"
    return None


# ------------------------------------------------------------------ states and draws
_INPUTS = {}


def inputs(case, cls=None):
    """{"x", "z", "rz" [rec, ..], "iso", "cond", "zc", "hist", "obj", "tries"}: the state (normal x 0.7; under the pair objective
    bodies 0 and 1 of design 0 coincide exactly at COINCIDENT_ROW), the step draw, the relaxation draws, the overwrite rows, the
    inpainting condition and its draw, the multistep history, and the objective -- from the first seed that holds the conditions."""
    if cls is None and case.index in _INPUTS:
        return _INPUTS[case.index]
    why = None
    for k in range(SEED_TRIES):
        seed = SEED_STRIDE * k + case.index
        g = torch.Generator().manual_seed(seed)
        shape = (case.B, case.L, case.F)
        x = torch.randn(shape, generator=g) * X_SCALE
        if case.kind == "pair":
            x[0, COINCIDENT_ROW, 4:6] = x[0, COINCIDENT_ROW, 0:2]
        d = {"x": x, "z": torch.randn(shape, generator=g), "rz": torch.randn((max(case.rec, 1),) + shape, generator=g),
             "iso": torch.randn((case.B, ROWS_FIXED, case.F), generator=g) * 0.3 if case.iso else None,
             "cond": torch.rand((case.B, ROWS_FIXED, case.F), generator=g) * 2 - 1 if case.inpaint else None,
             "zc": torch.randn((case.B, ROWS_FIXED, case.F), generator=g) if case.inpaint else None,
             "hist": torch.rand(shape, generator=g) * 2 - 1 if case.ms else None, "obj": None, "tries": k + 1, "seed": seed}
        if case.kind is not None:
            d["obj"] = make_objective(case, x, seed, cls)
            why = check_conditions(case, x, d["obj"])
            if why is not None:
                continue
        if cls is None:
            _INPUTS[case.index] = d
        return d
    raise AssertionError(f"{case.name}: no seed in {SEED_TRIES} holds the conditions ({why})")


# ------------------------------------------------------------------ the float64 statement of a case
def case_times(case):
    """(t, time_next | None)."""
    return (case.t, None) if case.entry == "ddpm" else ddim_times()[case.step]


def statement(case, d, E, tab, row=None, mut=None):
    """{"state": (value, A, n_e), "x_start": value, "clamped": share of x_start at +-1} of a case from the U-Net outputs ``E``
    ([W, P, B, window, 8]; plain: [1, 1, B, L, F]) that the judged side evaluated on ``R.compose_rows`` of the case's state: the
    iterations of the guidance (the relaxed state of iteration r is the state of iteration r + 1; E is the same in all of them --
    one iteration, or the frozen model), then the DDPM tail or the DDIM update with ``row`` = fp32 (sqrt(alpha_next), c, sigma, kappa).

    The unguided DDIM chain hands clip_x_start = clip_denoised to model_predictions (:1755): under pred_x0 / pred_v its pred_noise is
    re-derived from the CLAMPED x_start (:1018-1027), not p_mean_variance's unclamped one that the guided chain's DDIM return carries."""
    desc = case.desc()
    t, tn = case_times(case)
    kind, tables = tables_of(d["obj"]) if case.kind else (None, None)
    n = R.compose_roundings(desc.mode, desc.n_bodies, R.compose_cover(desc).double().view(1, -1, 1), desc.objective)
    mean, x0, eps, A = R.compose_predict_f64(tab, desc, d["x"], None, t, E.double())
    cur = (d["x"].double(), d["x"].double().abs(), torch.zeros(()))
    iters = max(case.rec, 1)
    assert iters == 1 or (case.frozen and case.kind in LINEAR_KINDS)
    g = Ag = None
    ng = 0
    for r in range(iters):
        if r > 0:
            mean, x0, eps, A, n = R.compose_repredict_f64(tab, desc, cur[0], cur[1], cur[2], t, E.double())
        if kind:
            g, Ag, ng = R.design_grad_f64(kind, cur[0], tables, n_bodies=case.nb, tc=case.tc, _mut=mut)
            if r > 0:       # linear in the state: its magnitude at the magnitude of the state, its count on top of the state's
                Ag, ng = R.design_grad_f64(kind, cur[1], tables, n_bodies=case.nb, tc=case.tc, _mut=mut)[1], ng + float(cur[2].max())
        if r < iters - 1:
            cur = R.step1d_update_f64("guided", mean, A["mean"], n["mean"], tab=tab, t=t, g=g, A_g=Ag, n_g=ng, alpha=case.alpha, iso=d["iso"],
                                      relax_z=d["rz"][r], _mut=mut)
    if case.entry == "ddpm":
        st = R.step1d_update_f64("guided", mean, A["mean"], n["mean"], tab=tab, t=t, g=g, A_g=Ag, n_g=ng, alpha=case.alpha, iso=d["iso"],
                                 z=d["z"], cond=d["cond"], z_cond=d["zc"], _mut=mut)
    else:
        e, Ae, ne = eps, A["pred_noise"], n["pred_noise"]
        if kind is None and case.objective != "pred_noise":
            e, Ae, ne = R.rederive_eps_f64(tab, t, d["x"], x0, A["x_start"], n["x_start"])
        st = R.step1d_update_f64("ddim", x0, A["x_start"], n["x_start"], tab=tab, t=t, eps=e, A_eps=Ae, n_eps=ne, g=g, A_g=Ag, n_g=ng,
                                 alpha=case.alpha, row=row, z=d["z"], last=tn < 0, hist=d["hist"], cond=d["cond"], z_cond=d["zc"], time_next=tn,
                                 _mut=mut)
    return {"state": st, "x_start": x0, "clamped": float((x0.abs() == 1.0).double().mean())}


def ratio(got, st):
    """(largest |got - ref| / ((n_e + 4) 2^-24 A_e), its index) over every element; an element that is exact on both sides counts 0."""
    ref, A, n = st
    got = got.detach().cpu()
    assert got.shape == ref.shape and bool(torch.isfinite(got).all()), (tuple(got.shape), tuple(ref.shape))
    err = (got.double() - ref).abs()
    q = torch.where(err == 0, torch.zeros_like(err), err / R.step1d_bound(n, A))
    i = int(q.argmax())
    return float(q.flatten()[i]), [int(v) for v in torch.unravel_index(torch.tensor(i), q.shape)]
