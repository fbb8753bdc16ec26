"""The cases of the sum of built-in objectives (cindm_amd.SumObjective, descriptor mode 7), shared by tests/test_sum_objective_host.py
(``closed_form_grad`` in fp32 against the float64 statement) and tests/test_gpu_sum_objective.py (the library against it).  No GPU and
no library call in here.

Shapes, states, draws and every term's tables are tests/step1d_cases.py's: a case here is one of its ``Case``s whose kind is "sum", and
term j of the sum is what ``step1d_cases.make_objective`` makes for the same case with that term's kind and the index ``index + j`` (so
per-design and shared tables mix inside one sum).  The time-consistency coefficient of a case is split in halves over the first two
terms: the sum carries their total and the statement takes the term once.

The float64 statement of the sum's gradient (``sum_grad_f64``) is the sum over the terms of ``f64_reference.design_grad_f64(kind, ..,
tc=0)``: g and A_g add; n_g = max_k n_k + (terms - 1), one rounding per addition on top of the longest term; with a time-consistency
term (``design_grad_f64`` of a table objective whose scale is 0 everywhere: that term alone) max(n_g, 5) + 1, as for a single kind."""
import copy

import torch

import cindm_amd
import f64_reference as R
import step1d_cases as S

# the kinds of a sum's terms in kernel order, as step1d_cases names them ("table": table-L2 or table-L2square by the case's norm)
TERM_SETS = {"qwp": ("quadratic", "table", "pair"), "qw": ("quadratic", "table"), "qp": ("quadratic", "pair"), "wp": ("table", "pair")}
SEED_BASE = 50000          # apart from the seeds step1d_cases.inputs tries for its own grid


class SumCase(S.Case):
    def __init__(self, index, entry, layout, terms, norm, **kw):
        super().__init__(index, entry, layout, "sum", **kw)
        self.terms, self.norm = terms, norm

    @property
    def term_kinds(self):
        return tuple(f"table-{self.norm}" if k == "table" else k for k in TERM_SETS[self.terms])

    @property
    def name(self):
        return super().name.replace("-sum-", f"-sum.{self.terms}.{self.norm}-")

    def term_case(self, j):
        """The step1d_cases case whose objective is term j: that kind, index + j, and its share of the time-consistency coefficient."""
        c = copy.copy(self)
        c.kind, c.index = self.term_kinds[j], self.index + j
        c.tc = 0.5 * self.tc if j < 2 else 0.0
        return c


def _cases():
    """40 cases: the four term sets x (guided DDPM step without recurrence, with -recurrence-1, guided DDIM update at steps 0 / 5 / 9,
    the DDIM update with the multistep solver); both norms, both guidance scalings, tc 0 / 0.5, the overwrite on half of them, and the
    layouts of step1d_cases in turn."""
    out = []
    k = 0
    for terms in TERM_SETS:
        for entry, rec, ms in (("ddpm", 0, False), ("ddpm", 1, False), ("ddim", 1, False), ("ddim", 1, True)):
            reps = 2 if entry == "ddpm" else 3
            for r in range(reps):
                kw = dict(alpha=(k // 2) % 2 == 1, tc=0.5 * (k % 2), rec=rec, iso=(k // 3) % 2 == 0, ms=ms)
                norm = "L2" if (k + k // 4) % 2 == 0 else "L2square"
                if entry == "ddpm":
                    kw["t"] = S.DDPM_T[(k + r) % 4]
                    layout = S.DDPM_LAYOUTS[k % 4]
                else:
                    kw["step"], kw["eta"] = S.DDIM_STEPS[r], 0.0 if ms else 0.5 * (k % 2)
                    layout = S.DDIM_LAYOUTS[k % 3]
                out.append(SumCase(len(out), entry, layout, terms, norm, **kw))
                k += 1
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES) == 40


def make_sum(case, x, seed, cls=None):
    """(SumObjective of the case for the state x, its terms in kernel order)."""
    terms = [S.make_objective(case.term_case(j), x, seed + 11 * j) for j in range(len(case.term_kinds))]
    return (cls or cindm_amd.SumObjective)(*terms), terms


def check_conditions(case, x, terms):
    for j, t in enumerate(terms):
        why = S.check_conditions(case.term_case(j), x, t)
        if why is not None:
            return f"term {j} ({case.term_kinds[j]}): {why}"
    return None


_INPUTS = {}


def inputs(case):
    """step1d_cases.inputs for a sum: the same recipe (state normal x 0.7, the coincident pair where a pair term is present, draws,
    overwrite rows, history), the objective the case's sum, from the first seed that holds every term's conditions."""
    if case.index in _INPUTS:
        return _INPUTS[case.index]
    why = None
    for k in range(S.SEED_TRIES):
        seed = SEED_BASE + S.SEED_STRIDE * k + case.index
        g = torch.Generator().manual_seed(seed)
        shape = (case.B, case.L, case.F)
        x = torch.randn(shape, generator=g) * S.X_SCALE
        if "pair" in case.term_kinds:
            x[0, S.COINCIDENT_ROW, 4:6] = x[0, S.COINCIDENT_ROW, 0:2]
        d = {"x": x, "z": torch.randn(shape, generator=g), "rz": torch.randn((max(case.rec, 1),) + shape, generator=g),
             "iso": torch.randn((case.B, S.ROWS_FIXED, case.F), generator=g) * 0.3 if case.iso else None, "cond": None, "zc": None,
             "hist": torch.rand(shape, generator=g) * 2 - 1 if case.ms else None, "tries": k + 1, "seed": seed}
        d["obj"], d["terms"] = make_sum(case, x, seed)
        why = check_conditions(case, x, d["terms"])
        if why is not None:
            continue
        d["obj"].check_state(*shape[:2], case.nb)
        _INPUTS[case.index] = d
        return d
    raise AssertionError(f"{case.name}: no seed in {S.SEED_TRIES} holds the conditions ({why})")


def sum_grad_f64(terms, x, nb, tc, *, mut=None, drop=None, tc_per_term=False):
    """(g, A_g, n_g) of the sum of ``terms`` (table objectives in kernel order) at x, with the total time-consistency coefficient
    ``tc`` taken once.  The host test's mutations: ``mut`` is handed to design_grad_f64 (``design0``), ``drop`` leaves term j out,
    ``tc_per_term`` takes the time-consistency term once per term."""
    g = A = None
    ns = []
    for j, t in enumerate(terms):
        if j == drop:
            continue
        kind, tables = S.tables_of(t)
        gj, Aj, nj = R.design_grad_f64(kind, x, tables, n_bodies=nb, tc=0.0, _mut=mut)
        g, A = (gj, Aj) if g is None else (g + gj, A + Aj)
        ns.append(nj)
    n = max(ns) + (len(ns) - 1)
    if R._as_f32(tc) > 0 and x.shape[1] > 1:
        L = x.shape[1]
        none = {"target": torch.zeros((L, nb, 2)), "scale": torch.zeros((L, nb))}
        gt, At, _ = R.design_grad_f64("table-L2square", x, none, n_bodies=nb, tc=tc)
        times = len(terms) if tc_per_term else 1
        g, A = g + times * gt, A + times * At
        n = max(n, 5) + 1
    return g, A, n


def statement(case, d, E, tab, row=None):
    """step1d_cases.statement for a one-evaluation sum case: {"state": (value, A, n_e), "x_start": value} from the U-Net outputs E."""
    desc = case.desc()
    t, tn = S.case_times(case)
    assert max(case.rec, 1) == 1
    n = R.compose_roundings(desc.mode, desc.n_bodies, R.compose_cover(desc).double().view(1, -1, 1), desc.objective)
    mean, x0, eps, A = R.compose_predict_f64(tab, desc, d["x"], None, t, E.double())
    terms = d["obj"].table_terms(case.L, case.nb)
    g, Ag, ng = sum_grad_f64(terms, d["x"].double(), case.nb, d["obj"].time_consistency_coef)
    if case.entry == "ddpm":
        st = R.step1d_update_f64("guided", mean, A["mean"], n["mean"], tab=tab, t=t, g=g, A_g=Ag, n_g=ng, alpha=case.alpha, iso=d["iso"],
                                 z=d["z"], cond=None, z_cond=None)
    else:
        st = R.step1d_update_f64("ddim", x0, A["x_start"], n["x_start"], tab=tab, t=t, eps=eps, A_eps=A["pred_noise"], n_eps=n["pred_noise"],
                                 g=g, A_g=Ag, n_g=ng, alpha=case.alpha, row=row, z=d["z"], last=tn < 0, hist=d["hist"], cond=None, z_cond=None,
                                 time_next=tn)
    return {"state": st, "x_start": x0, "clamped": float((x0.abs() == 1.0).double().mean())}
