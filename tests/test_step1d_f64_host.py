"""CPU: the float64 statement of the 1-D step tail in oracle/f64_reference.py (``design_grad_f64``, ``step1d_update_f64``,
``compose_repredict_f64``) is proven before it judges a kernel.

Over the whole grid of tests/step1d_cases.py -- the one tests/test_gpu_step1d_f64.py runs the library on -- the fp32 oracle lies within
(n_e + 4) * 2^-24 * A_e of the statement element by element, the statement evaluated on the oracle's OWN U-Net outputs (a recorder
around ``Diffusion1D.model``): ``cindm_oracle.p_sample_compose_inside`` with the objective differentiated by autograd for the guided
DDPM step and its relaxations, followed by ``q_sample`` on the inpainting rows as ``p_sample_loop`` does; the body of
``cindm_oracle.ddim_sample``'s loop for one DDIM pair (``test_ddim_body_is_the_oracles`` holds that restatement to ``ddim_sample``
itself bit for bit over a whole chain), with the multistep term of cindm_amd/diffusion1d.py's Python loop in torch.  The oracle is
pinned to the reference project by tests/golden/ddim_1d.npz and its siblings.  The two-evaluation cases run the oracle's U-Net with the
frozen output (``step1d_cases.frozen_state_dict``), as the GPU file does.

Thirteen mutations of the statement each leave the bound by more than FLOOR = 100 x on the cases listed for them.  The smallest multiple
each reaches over its cases (MUTATION_FACTORS): grad_sign 5.1e3, eta_ac 8.8e2 (DDPM at t = 600; the DDIM pair at t = 499 reaches only 70 x
-- beta there is 4e-3 -- so its cases are the pair at t = 999), relax_swap 8.5e5, ddim_no_g 3.3e5, lap_Ltot 3.3e3, lap_no_ends 7.4e4,
point_rows 1.4e5, design0 3.4e5, band_hi 1.7e5, ms_after_inpaint 9.2e5, iso_after_relax 2.3e2 (on the DDPM step the overwritten rows
reach the result only through the Laplacian of row 4; 1.6e5 on the DDIM pairs), inpaint_tnext 4.7e5, noise_t0 4.6e5; the un-mutated
statement stays at 0.2505 or below over the whole grid (244 cases).  ``noise_t0`` adds the draw at the level of t = 1: with the table's own entry at t = 0 (the clipped
log-variance, sigma = 1e-10) a draw added there is below every bound, which is the table's purpose."""
import types

import pytest
import torch

import cindm_oracle as O
import f64_reference as R
import step1d_cases as S
from cindm_amd.schedule import ddim_schedule, multistep_kappa

TAB = {obj: O.make_schedule("cosine", 1000, obj) for obj in S.OBJECTIVES}
_SD = {}
_GOT = {}


def _sd(F, frozen):
    if (F, frozen) not in _SD:
        sd = O.synth_state_dict(O.unet1d_param_shapes(S.WINDOW, F, attention=True), seed=0)
        _SD[(F, frozen)] = S.frozen_state_dict(sd) if frozen else sd
    return _SD[(F, frozen)]


def ddim_row(case):
    """fp32 (sqrt(alpha_next), c, sigma, kappa) of the case's pair, as the library's chain is handed them."""
    shim = types.SimpleNamespace(num_timesteps=1000, sampling_timesteps=S.DDIM_S, ddim_sampling_eta=case.eta, alphas_cumprod=TAB["pred_noise"]["alphas_cumprod"])
    kap = multistep_kappa(shim)[case.step] if case.ms else torch.zeros(())
    return torch.cat([ddim_schedule(shim)[1][case.step], kap.reshape(1)])


def _ddim_body(od, img, cond, t, tn, eta, z, zc, *, design_fn=None, kap=None, hist=None, **kw):
    """One pass of the loop of cindm_oracle.ddim_sample (-> img, x_start), with the multistep term of GaussianDiffusion1D.ddim_sample's
    Python loop ahead of the inpainting rows."""
    if design_fn is None:
        pred_noise, x_start = O.model_predictions(od, img, cond, t, clip_x_start=True)
    else:
        pred_noise, x_start = O.p_sample_compose_inside(od, img, cond, t, None, design_fn=design_fn, ddim_return=True, **kw)
    san, c, sigma = O.ddim_coefs(od, t, tn, eta)
    img = x_start * san + c * pred_noise + sigma * z
    if tn < 0:
        return x_start, x_start
    if kap is not None and float(kap) != 0.0:
        img = img + kap * (x_start - hist)
    if cond is not None:
        img = img.clone()
        img[:, :cond.shape[1], :] = O.q_sample(od, cond, t, zc)
    return img, x_start


def oracle(case):
    """(state, x_start, E) of the fp32 oracle on a case; E [W, P, B, window, 8] (plain: [1, 1, B, L, F]) are its U-Net's outputs."""
    if case.index in _GOT:
        return _GOT[case.index]
    d = S.inputs(case)
    sd = _sd(8, case.frozen)
    od = O.Diffusion1D(sd, image_size=S.WINDOW, conditioned_steps=0, objective=case.objective)
    seen = []

    def model(x, t):
        seen.append(O.unet1d_forward(sd, x, t))
        return seen[-1]
    od.model = model
    t, tn = S.case_times(case)
    kw = dict(design_guidance=case.guidance, compose_mode="mean-inside", n_composed=case.W - 1, compose_start_step=S.CS,
              single_model_step=S.WINDOW, compose_n_bodies=case.nb, initial_state_overwrite=d["iso"], recur_noise=d["rz"])
    if case.entry == "ddpm":
        out, x0 = O.p_sample_compose_inside(od, d["x"].clone(), None, t, d["z"], design_fn=d["obj"], **kw)
        if case.inpaint:
            out = out.clone()
            out[:, :S.ROWS_FIXED] = O.q_sample(od, d["cond"], t, d["zc"])
    else:
        row = ddim_row(case)
        out, x0 = _ddim_body(od, d["x"].clone(), d["cond"], t, tn, case.eta, d["z"], d["zc"], design_fn=d["obj"],
                             kap=row[3] if case.ms else None, hist=d["hist"], **kw)
    per = 1 if case.desc().mode == "plain" else case.W * (case.nb * (case.nb - 1) // 2)
    assert len(seen) == per * max(case.rec, 1)
    for k in range(per, len(seen)):                   # the frozen model: every evaluation gives the same bits
        assert torch.equal(seen[k], seen[k % per])
    E = torch.stack(seen[:per])
    E = E.view(1, 1, case.B, case.L, case.F) if per == 1 and case.desc().mode == "plain" else E.view(case.W, -1, case.B, S.WINDOW, 8)
    _GOT[case.index] = (out, x0, E)
    return _GOT[case.index]


def case_ratio(case, mut=None):
    out, x0, E = oracle(case)
    st = S.statement(case, S.inputs(case), E, TAB[case.objective], row=ddim_row(case) if case.entry == "ddim" else None, mut=mut)
    return S.ratio(out, st["state"])[0], st


# ------------------------------------------------------------------ the grid, the fp32 oracle
GROUPS = sorted({(c.entry, c.kind or "unguided", c.rec) for c in S.CASES})


@pytest.mark.parametrize("entry,kind,rec", GROUPS, ids=[f"{e}-{k}-r{r}" for e, k, r in GROUPS])
def test_oracle_within_bound(entry, kind, rec):
    cases = [c for c in S.CASES if (c.entry, c.kind or "unguided", c.rec) == (entry, kind, rec)]
    assert cases
    for c in cases:
        r, st = case_ratio(c)
        print(f"{c.name}: err/bound {r:.4f}, clamped {st['clamped']:.3f}, seed try {S.inputs(c)['tries']}")
        assert r <= 1.0, (c.name, r)


def test_grid_covers_the_axes():
    """What the issue's grid asks for is in CASES, and every case found a seed that holds the input conditions."""
    C = S.CASES
    assert len(C) == 244 and all(S.inputs(c)["tries"] <= S.SEED_TRIES for c in C)
    ddpm, ddim = S.select("ddpm"), S.select("ddim")
    for kind in S.KINDS:
        for alpha in (False, True):
            for tc in (0.0, 0.5):
                assert {c.t for c in ddpm if (c.kind, c.alpha, c.tc, c.frozen) == (kind, alpha, tc, False) and c.objective == "pred_noise"} == set(S.DDPM_T)
            assert {(c.step, c.eta) for c in ddim if (c.kind, c.alpha, c.frozen) == (kind, alpha, False) and c.objective == "pred_noise"} == \
                {(s, e) for s in S.DDIM_STEPS for e in (0.0, 0.5)}
        sub = [c for c in C if c.kind == kind]
        assert {c.iso for c in sub} == {False, True} and {c.inpaint for c in sub} == {False, True} and {c.tc for c in sub} == {0.0, 0.5}
        assert {c.rec for c in sub if c.entry == "ddpm"} >= {0, 1} and {c.nb for c in sub} == {2, 3, 4} and {c.W for c in sub} == {1, 2}
    assert {c.B * c.L * c.F for c in C} >= {384, 1440}
    assert {(c.objective, c.step, c.eta) for c in ddim if c.kind is None} == {(o, s, e) for o in S.OBJECTIVES for s in S.DDIM_STEPS for e in (0.0, 0.5)}
    assert {c.objective for c in C if c.kind and c.kind.startswith("point")} == set(S.OBJECTIVES)
    assert any(c.ms and c.step == 5 for c in ddim) and any(c.ms and c.step == 0 for c in ddim) and any(c.ms and c.step == 9 for c in ddim)
    assert {c.kind for c in C if c.rec == 2} == set(S.LINEAR_KINDS) and all(c.frozen for c in C if c.rec == 2)
    pairs = [c for c in C if c.kind == "pair"]
    for c in pairs:
        cond = R.design_conditions_f64("pair", S.inputs(c)["x"], S.tables_of(S.inputs(c)["obj"])[1], n_bodies=c.nb)
        assert cond["coincident"] >= 1 and cond["min_r"] >= S.MIN_R and cond["min_gap"] > S.MIN_GAP
        w = S.inputs(c)["obj"].weight
        assert 0.1 < float((w == 0).float().mean()) and {3, 6} >= {w.shape[-1]} - {1}


def test_coincident_pair_is_exactly_zero():
    """The row where two bodies coincide: the pair's term is 0.0 in the statement and in the objective's autograd, with weight > 0."""
    c = next(k for k in S.CASES if k.kind == "pair" and k.nb == 2 and k.tc == 0.0)
    d = S.inputs(c)
    g, A, _ = R.design_grad_f64("pair", d["x"], S.tables_of(d["obj"])[1], n_bodies=2)
    assert float(d["obj"].weight[0, S.COINCIDENT_ROW, 0]) > 0
    assert float(g[0, S.COINCIDENT_ROW].abs().max()) == 0.0 and float(A[0, S.COINCIDENT_ROW].abs().max()) == 0.0
    x = d["x"].clone().requires_grad_()
    ga = torch.autograd.grad(d["obj"](x), x)[0]
    assert float(ga[0, S.COINCIDENT_ROW].abs().max()) == 0.0 and bool(torch.isfinite(ga).all())


def test_ddim_body_is_the_oracles():
    """``_ddim_body`` restates the loop of cindm_oracle.ddim_sample: a guided S = 10 chain with inpainting rows, step by step, bit for bit."""
    c = next(k for k in S.CASES if k.entry == "ddim" and k.kind == "point-L2" and k.layout == "b2w1n2" and not k.frozen)
    d = S.inputs(c)
    g = torch.Generator().manual_seed(3)
    shape, S10 = tuple(d["x"].shape), S.DDIM_S
    cond = torch.rand((c.B, S.ROWS_FIXED, c.F), generator=g) * 2 - 1
    tape = {"init": d["x"], "step": torch.randn((S10,) + shape, generator=g), "recur": torch.randn((S10, 1) + shape, generator=g),
            "cond": torch.randn((S10,) + tuple(cond.shape), generator=g)}
    od = O.Diffusion1D(_sd(8, False), image_size=S.WINDOW, conditioned_steps=0)
    states = {}
    kw = dict(design_guidance="standard-recurrence-1", compose_mode="mean-inside", n_composed=0, compose_start_step=S.CS, compose_n_bodies=c.nb)
    O.ddim_sample(od, shape, cond, tape, sampling_timesteps=S10, eta=0.5, design_fn=d["obj"], record=lambda i, img: states.__setitem__(i, img.clone()), **kw)
    img = d["x"].clone()
    for i, (t, tn) in enumerate(S.ddim_times()):
        img, _ = _ddim_body(od, img, cond, t, tn, 0.5, tape["step"][i], tape["cond"][i], design_fn=d["obj"], single_model_step=S.WINDOW,
                            initial_state_overwrite=None, recur_noise=tape["recur"][i], **kw)
        assert torch.equal(img, states[i]), i


# ------------------------------------------------------------------ the bound means something
def _pick(n=3, **kw):
    frozen = kw.pop("frozen", False)
    pred = kw.pop("where", lambda c: True)
    out = [c for c in S.CASES if c.frozen == frozen and c.objective == "pred_noise" and all(getattr(c, k) == v for k, v in kw.items()) and pred(c)]
    assert out, kw
    return out[:n]


# mutation -> the cases of the grid on which it must show
MUTATIONS = {
    "grad_sign": lambda: _pick(entry="ddpm", kind="point-L2") + _pick(entry="ddpm", kind="pair", alpha=True) + _pick(entry="ddpm", kind="quadratic", rec=2, frozen=True),
    "eta_ac": lambda: _pick(entry="ddpm", alpha=True, t=600) + _pick(entry="ddim", alpha=True, step=0),
    "relax_swap": lambda: _pick(entry="ddpm", rec=2, frozen=True, n=4) + _pick(entry="ddim", rec=2, frozen=True, n=2),
    "ddim_no_g": lambda: _pick(entry="ddim", kind="point-L2square", where=lambda c: c.step < 9) + _pick(entry="ddim", kind="pair", where=lambda c: c.step < 9),
    "lap_Ltot": lambda: _pick(entry="ddpm", tc=0.5, kind="table-L2", alpha=False) + _pick(entry="ddpm", tc=0.5, kind="quadratic", alpha=False) + _pick(entry="ddim", tc=0.5, alpha=False, where=lambda c: c.step < 9, n=2),
    "lap_no_ends": lambda: _pick(entry="ddpm", tc=0.5, iso=False, alpha=False) + _pick(entry="ddim", tc=0.5, where=lambda c: c.step < 9 and not c.inpaint, n=2),
    "point_rows": lambda: _pick(entry="ddpm", kind="point-L2") + _pick(entry="ddpm", kind="point-L2square") + _pick(entry="ddim", kind="point-L2", where=lambda c: c.step < 9, n=2),
    "design0": lambda: _pick(entry="ddpm", kind="table-L2") + _pick(entry="ddpm", kind="quadratic") + _pick(entry="ddpm", kind="pair"),
    "band_hi": lambda: _pick(entry="ddpm", kind="pair") + _pick(entry="ddim", kind="pair", where=lambda c: c.step < 9, n=2),
    "ms_after_inpaint": lambda: _pick(entry="ddim", ms=True, inpaint=True, step=5, n=2),
    "iso_after_relax": lambda: _pick(entry="ddpm", rec=2, iso=True, tc=0.5, alpha=False, t=600, frozen=True) + _pick(entry="ddim", rec=2, iso=True, frozen=True, n=4),
    "inpaint_tnext": lambda: _pick(entry="ddim", inpaint=True, where=lambda c: c.step < 9, n=4),
    "noise_t0": lambda: _pick(entry="ddpm", t=0, n=4),
}
FLOOR = 100.0


@pytest.mark.parametrize("mut", list(MUTATIONS))
def test_mutation_leaves_the_bound(mut):
    """``grad_sign`` the gradient added; ``eta_ac`` eta_t from alphas_cumprod; ``relax_swap`` the relaxation's two coefficients swapped;
    ``ddim_no_g`` DDIM fed eps without g; ``lap_Ltot`` the Laplacian over Ltot; ``lap_no_ends`` no one-sided ends; ``point_rows`` the
    point objective's rows off by one; ``design0`` a per-design table read at design 0; ``band_hi`` hi where lo belongs;
    ``ms_after_inpaint`` the multistep term after the inpainting rows; ``iso_after_relax`` the overwrite after the relaxation;
    ``inpaint_tnext`` the inpainting level time_next; ``noise_t0`` a draw added at t = 0.  Each puts the fp32 oracle outside the
    mutated statement's bound on every case listed for it, by FLOOR = 100 x at least."""
    cases = MUTATIONS[mut]()
    worst = float("inf")
    for c in cases:
        good, bad = case_ratio(c)[0], case_ratio(c, (mut,))[0]
        print(f"{mut} {c.name}: good {good:.3f}, mutated {bad:.3e}")
        assert good <= 1.0 and bad > FLOOR, (mut, c.name, good, bad)
        worst = min(worst, bad)
    print(f"{mut}: smallest factor {worst:.3e}")


# For the record (asserted is FLOOR): the smallest err / bound each mutation reaches over its cases, rounded down.
MUTATION_FACTORS = {"grad_sign": 5.1e3, "eta_ac": 8.8e2, "relax_swap": 8.5e5, "ddim_no_g": 3.3e5, "lap_Ltot": 3.3e3, "lap_no_ends": 7.4e4,
                    "point_rows": 1.4e5, "design0": 3.4e5, "band_hi": 1.7e5, "ms_after_inpaint": 9.2e5, "iso_after_relax": 2.3e2,
                    "inpaint_tnext": 4.7e5, "noise_t0": 4.6e5}


def test_roundings_by_hand():
    one = torch.ones((1, 6, 8), dtype=torch.float64)
    tab = TAB["pred_noise"]
    assert R.design_grad_f64("point-L2", one, {"target": torch.tensor([0.25, -0.5]), "last_n_step": 3, "coef": 2.0}, n_bodies=2)[2] == 8
    assert R.design_grad_f64("point-L2square", one, {"target": torch.tensor([0.25, -0.5]), "last_n_step": 3, "coef": 2.0}, n_bodies=2, tc=0.5)[2] == 6
    assert R.design_grad_f64("quadratic", one, {"S": torch.zeros(6, 8, 8), "h": torch.zeros(6, 8)}, n_bodies=2)[2] == 10
    assert R.design_grad_f64("pair", one, {k: torch.ones(6, 1) for k in ("lo", "hi", "weight")}, n_bodies=2)[2] == 10
    g = R.design_grad_f64("point-L2square", one, {"target": torch.tensor([0.25, -0.5]), "last_n_step": 3, "coef": 3.0}, n_bodies=2)[0]
    assert float(g[0, 2].abs().max()) == 0.0 and float(g[0, 3, 0]) == 1.5 and float(g[0, 3, 1]) == 3.0 and float(g[0, 3, 2]) == 0.0
    st = R.step1d_update_f64("guided", one, one, 8, tab=tab, t=5, g=one, A_g=one, n_g=4, alpha=True, z=one)
    assert float(st[2].max()) == 8 + 1 + 4 and float(st[2].min()) == 13
    st = R.step1d_update_f64("guided", one, one, 8, tab=tab, t=0, g=one, A_g=one, n_g=12, iso=torch.zeros(1, 2, 8), z=one)
    assert float(st[2][0, 0, 0]) == 0 and float(st[2][0, 2, 0]) == 13 and float(st[0][0, 0, 0]) == 0.0 and float(st[0][0, 2, 0]) == 0.0
    st = R.step1d_update_f64("relax", one, one, 9, tab=tab, t=30, relax_z=one)
    assert float(st[2].max()) == 13
    st = R.step1d_update_f64("ddim", one, one, 6, tab=tab, t=499, eps=one, A_eps=one, n_eps=9, row=torch.tensor([1.0, 1.0, 0.0, 0.5]), z=one, hist=one)
    assert float(st[2].max()) == 15 and float(st[0].max()) == 2.0
    st = R.step1d_update_f64("inpaint", one, one, 9, tab=tab, t=30, cond=torch.zeros(1, 4, 8), z_cond=torch.zeros(1, 4, 8))
    assert float(st[2][0, 3, 0]) == 3 and float(st[2][0, 4, 0]) == 9 and float(st[0][0, 3, 0]) == 0.0
    assert R.BOUND_SLACK == 4 and R.U24 == 2.0 ** -24
