"""Host side of the sum of built-in objectives (cindm_amd.SumObjective, descriptor mode 7): no device.

``closed_form_grad`` restates compose_update_sum_kernel in torch, operation for operation: each present term exactly as its own
objective's ``closed_form_grad`` (without the time-consistency term), g = the first present term, g = g + next in the order quadratic,
waypoint, pair-distance -- position features only; the velocity features see the quadratic term alone -- and the time-consistency term
last, once, with the sum of the terms' coefficients.

1. In float64 it is autograd of ``__call__`` (1e-12 relative) for every non-empty subset of {waypoint-L2 | waypoint-L2square, quadratic,
   pair-distance}, shared and per-design tables, 2 / 3 / 4 bodies, tc 0 / 0.5.
2. In fp32 it stays within the float64 statement's bound on every element,
       |fp32 - f64|  <=  (n_g + BOUND_SLACK) * 2^-24 * A_g,
   with (g, A_g, n_g) the sum over the terms of ``f64_reference.design_grad_f64(kind, .., tc=0)`` (tests/sum_cases.py:
   A_g = sum A_k, n_g = max_k n_k + (terms - 1): one rounding per addition on top of the longest term; with tc max(., 5) + 1).  The
   bound is derived, not tuned.  States and tables are step1d_cases' recipe, its conditions (MIN_DEN, MIN_R, MIN_GAP) asserted per term.
3. Mutations of the statement -- each term dropped in turn, the time-consistency term once per term, a per-design table read at
   design 0 -- leave that bound by more than 100 x.
4. Bit identities, refusals, the descriptor, sharding, the header text."""
import itertools
import math
import os

import pytest
import torch

import cindm_amd
import f64_reference as R
import step1d_cases as S
import sum_cases as SC
from cindm_amd import PairDistanceObjective as PD
from cindm_amd import PointObjective as PT
from cindm_amd import QuadraticObjective as QD
from cindm_amd import SumObjective
from cindm_amd import WaypointObjective as WP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLOOR = 100.0


def _say(name, v):
    print(f"[sum] {name}: {v:.3e}")
    return v


# ------------------------------------------------------------------ 1. float64: the closed form is autograd
def _terms64(seed, B, L, nb, kinds, per, tc):
    """Terms of the given kinds on random tables ([B, ..] when ``per`` else shared), tc split over the terms; positions such that every
    pair is apart."""
    g = torch.Generator().manual_seed(seed)
    F, P = 4 * nb, nb * (nb - 1) // 2
    lead = (B,) if per else ()
    rnd = lambda *s: torch.rand(lead + s, generator=g)
    share = tc / len(kinds)
    out = []
    for kind in kinds:
        if kind.startswith("waypoint"):
            out.append(WP(rnd(L, nb, 2) * 1.6 - 0.8, rnd(L, nb) * (rnd(L, nb) > 0.3), coef=1.5, time_consistency_coef=share,
                          design_fn_mode=kind.split("-")[1]))
        elif kind == "quadratic":
            M = rnd(L, F, F) * 2 - 1
            out.append(QD((M + M.transpose(-1, -2)) * 0.5, rnd(L, F) * 2 - 1, time_consistency_coef=share))
        else:
            d = rnd(L, P) * 1.2 + 0.2
            k = torch.arange(d.numel()).reshape(d.shape) % 3
            out.append(PD(torch.where(k == 1, torch.zeros_like(d), d), torch.where(k == 0, torch.full_like(d, float("inf")), d),
                          (rnd(L, P) + 0.5) * (rnd(L, P) > 0.2), time_consistency_coef=share))
    while True:
        pos = torch.rand((B, L, F), generator=g, dtype=torch.float64) * 2 - 1
        x = pos.reshape(B, L, nb, 4)[..., :2]
        if all(float((x[:, :, i] - x[:, :, j]).norm(dim=-1).min()) > 1e-3 for i, j in R.compose_pairs(nb)):
            return out, pos


SUBSETS = [c for r in (1, 2, 3) for c in itertools.combinations(("waypoint-L2", "waypoint-L2square", "quadratic", "pair"), r)
           if not {"waypoint-L2", "waypoint-L2square"} <= set(c)]


@pytest.mark.parametrize("kinds", SUBSETS, ids=["+".join(c) for c in SUBSETS])
def test_closed_form_is_autograd_in_float64(kinds):
    assert len(SUBSETS) == 11
    k = 0
    for nb in (2, 3, 4):
        for per in (False, True):
            for tc in (0.0, 0.5):
                terms, pos = _terms64(300 + k, 3, 6, nb, kinds, per, tc)
                k += 1
                obj = SumObjective(*reversed(terms))
                assert obj.per_design == (3 if per else None) and math.isclose(obj.time_consistency_coef, tc)
                x = pos.clone().requires_grad_()
                want = torch.autograd.grad(obj(x), x)[0]
                got = obj.closed_form_grad(pos)
                assert got.dtype == torch.float64 and got.shape == pos.shape
                rel = float((got - want).abs().max() / want.abs().max())
                assert float(want.abs().max()) > 0.05 and rel <= 1e-12, (kinds, nb, per, tc, rel)
                if "quadratic" not in kinds:
                    assert float(got.reshape(3, 6, nb, 4)[..., 2:].abs().max()) == 0.0          # velocities: the quadratic term only


# ------------------------------------------------------------------ 2. fp32: within the float64 statement's bound
def _ratio(got, g, A, n):
    err = (got.double() - g).abs()
    q = torch.where(err == 0, torch.zeros_like(err), err / R.step1d_bound(n, A))
    return float(q.max())


def test_grid():
    C = SC.CASES
    assert len(C) == 40 and all(SC.inputs(c)["tries"] <= S.SEED_TRIES for c in C)
    assert {c.terms for c in C} == set(SC.TERM_SETS) and {c.norm for c in C} == {"L2", "L2square"}
    assert {c.nb for c in C} == {2, 3, 4} and {c.alpha for c in C} == {False, True} and {c.tc for c in C} == {0.0, 0.5}
    for terms in SC.TERM_SETS:
        sub = [c for c in C if c.terms == terms]
        assert {(c.entry, c.rec, c.ms) for c in sub} == {("ddpm", 0, False), ("ddpm", 1, False), ("ddim", 1, False), ("ddim", 1, True)}
        assert {c.step for c in sub if c.entry == "ddim"} == set(S.DDIM_STEPS) and {c.iso for c in sub} == {False, True}
    # every multi-term sum mixes per-design and shared tables
    for c in C:
        d = SC.inputs(c)
        dims = {(name, getattr(t, name).dim() == rank + 1) for t in d["terms"] for name, rank in t._TABLES}
        assert {per for _, per in dims} == {False, True}, c.name


@pytest.mark.parametrize("terms", list(SC.TERM_SETS))
def test_fp32_closed_form_within_the_float64_statement(terms):
    worst = 0.0
    for c in (c for c in SC.CASES if c.terms == terms):
        d = SC.inputs(c)
        for j, t in enumerate(d["terms"]):
            assert S.check_conditions(c.term_case(j), d["x"], t) is None
        obj = d["obj"]
        assert math.isclose(obj.time_consistency_coef, c.tc)
        g, A, n = SC.sum_grad_f64(d["terms"], d["x"].double(), c.nb, obj.time_consistency_coef)
        got = obj.closed_form_grad(d["x"])
        assert got.dtype == torch.float32
        r = _ratio(got, g, A, n)
        worst = max(worst, r)
        assert r <= 1.0, (c.name, r)
    _say(f"{terms}: largest err / bound", worst)


def test_rounding_counts_by_hand():
    """n_g of a sum: the longest term, one addition per further term, the time-consistency term as for a single kind."""
    c = next(c for c in SC.CASES if c.terms == "qwp" and c.norm == "L2" and c.tc == 0.0)
    d = SC.inputs(c)
    x = d["x"].double()
    n_pair, n_quad, n_way = 9 + (c.nb - 1), c.F + 2, 7
    assert SC.sum_grad_f64(d["terms"], x, c.nb, 0.0)[2] == max(n_pair, n_quad, n_way) + 2
    assert SC.sum_grad_f64(d["terms"], x, c.nb, 0.5)[2] == max(max(n_pair, n_quad, n_way) + 2, 5) + 1
    assert SC.sum_grad_f64(d["terms"][1:2], x, c.nb, 0.0)[2] == n_way and R.BOUND_SLACK == 4


# ------------------------------------------------------------------ 3. mutations of the statement
def _mutation_ratio(c, **mut):
    d = SC.inputs(c)
    got = d["obj"].closed_form_grad(d["x"])
    g, A, n = SC.sum_grad_f64(d["terms"], d["x"].double(), c.nb, d["obj"].time_consistency_coef, **mut)
    return _ratio(got, g, A, n)


@pytest.mark.parametrize("terms", list(SC.TERM_SETS))
def test_mutations_leave_the_bound(terms):
    cases = [c for c in SC.CASES if c.terms == terms]
    for c in cases:
        for j in range(len(c.term_kinds)):
            assert _say(f"{c.name}: drop term {j}", _mutation_ratio(c, drop=j)) > FLOOR
        assert _say(f"{c.name}: design 0's tables", _mutation_ratio(c, mut=("design0",))) > FLOOR
        if c.tc > 0:
            assert _say(f"{c.name}: tc once per term", _mutation_ratio(c, tc_per_term=True)) > FLOOR
    assert any(c.tc > 0 for c in cases)


# ------------------------------------------------------------------ 4. bit identities
def _three(seed=7, B=3, L=24, nb=3, tc=0.25):
    c = next(c for c in SC.CASES if c.terms == "qwp" and c.nb == 3 and c.L == 24)
    d = SC.inputs(c)
    q, w, p = d["terms"]
    return d["x"], q, w, p


def test_one_term_sum_is_the_term():
    x, q, w, p = _three()
    for t in (q, w, p, QD(q.S, q.h, time_consistency_coef=0.5), WP(w.target, None, _scale=w.scale, time_consistency_coef=0.5, design_fn_mode="L2square"),
              PD(p.lo, p.hi, p.weight, time_consistency_coef=0.5)):
        for pos in (x, x.double()):
            assert torch.equal(SumObjective(t).closed_form_grad(pos), t.closed_form_grad(pos))
        assert float(SumObjective(t)(x.double())) == float(t(x.double()))


def test_point_term_is_its_table_form():
    x, q, w, p = _three()
    B, L, F = x.shape
    for mode in ("L2", "L2square"):
        pt = PT([0.25, -0.5], 3, coef=0.6, time_consistency_coef=0.5, design_fn_mode=mode)
        tab = WP.from_point([0.25, -0.5], 3, L, F // 4, coef=0.6, time_consistency_coef=0.5, design_fn_mode=mode)
        a, b = pt + p, tab + p
        assert isinstance(a, SumObjective) and torch.equal(a.closed_form_grad(x), b.closed_form_grad(x))
        assert float(a(x.double())) == float(b(x.double()))
        ta, tb = a.table_terms(L, F // 4)[0], b.table_terms(L, F // 4)[0]
        assert torch.equal(ta.scale, tb.scale) and torch.equal(ta.target, tb.target) and ta.design_fn_mode == mode
        assert a.descriptor("standard").last_n_step == (1 if mode == "L2" else 2)
        assert a.table_terms(L, F // 4)[0] is ta          # made once per (L, n_bodies): its device tables are cached


def test_addition_flattens_and_keeps_the_kernel_order():
    x, q, w, p = _three()
    a, b = (p + q) + w, w + (q + p)
    for s in (a, b, SumObjective(SumObjective(w), SumObjective(p, q)), p + (w + q)):
        assert [type(t) for t in s.terms] == [QD, WP, PD] and all(not isinstance(t, SumObjective) for t in s.terms)
        assert s.terms[0] is q and s.terms[1] is w and s.terms[2] is p
        assert torch.equal(s.closed_form_grad(x), a.closed_form_grad(x))
    assert float(a(x.double())) == float(b(x.double()))


def test_scalar_multiples():
    x, q, w, p = _three()
    w32 = torch.tensor(0.3, dtype=torch.float32)
    for obj, names in ((w, ("scale",)), (q, ("S", "h")), (p, ("weight",))):
        for o in (0.3 * obj, obj * 0.3):
            assert type(o) is type(obj) and o is not obj
            for name in names:
                assert torch.equal(getattr(o, name), w32 * getattr(obj, name))          # one fp32 product per entry
            assert o.time_consistency_coef == 0.3 * obj.time_consistency_coef
    assert torch.equal((0.3 * w).target, w.target) and torch.equal((0.3 * p).lo, p.lo) and torch.equal((0.3 * p).hi, p.hi)
    pt = PT([0.25, -0.5], 3, coef=0.6, time_consistency_coef=0.5)
    assert (2 * pt).coef == float(torch.tensor(2.0) * torch.tensor(0.6)) and (2 * pt).time_consistency_coef == 1.0 and pt.coef == 0.6
    assert torch.equal((-1 * QD(q.S, q.h)).S, -q.S)
    s = 0.5 * (q + w + p)
    assert isinstance(s, SumObjective) and torch.equal(s.terms[1].scale, torch.tensor(0.5) * w.scale)
    for bad in (-1.0, float("nan"), float("inf")):
        for obj in (w, p, pt):
            with pytest.raises(ValueError, match="multiple"):
                bad * obj
    for bad in (float("nan"), float("inf"), -float("inf")):
        with pytest.raises(ValueError, match="multiple"):
            bad * q
    with pytest.raises(ValueError, match="overflows"):
        3e38 * (3e38 * QD(q.S, q.h))


# ------------------------------------------------------------------ 5. refusals
def test_refusals():
    x, q, w, p = _three()
    B, L, F = x.shape
    pt = PT([0.25, -0.5], 3)
    for a, b, kind in ((w, w, "waypoint"), (pt, w, "waypoint"), (w, pt, "waypoint"), (pt, pt, "waypoint"), (q, q, "quadratic"), (p, p, "pair-distance")):
        with pytest.raises(ValueError, match=f"two {kind} terms"):
            a + b
    with pytest.raises(ValueError, match="two quadratic terms"):
        (q + w) + (p + q)
    for foreign in (3, "x", lambda v: v.sum()):
        with pytest.raises(TypeError, match="a term is a"):
            SumObjective(w, foreign)
    with pytest.raises(TypeError):
        w + 3
    with pytest.raises(ValueError, match="no terms"):
        SumObjective()
    short = QD(q.S[..., :L - 1, :, :], q.h[..., :L - 1, :])
    with pytest.raises(ValueError, match=r"disagree on \(L, n_bodies\)"):
        short + w
    with pytest.raises(ValueError, match=r"disagree on \(L, n_bodies\)"):
        PD.apart(0.5, torch.ones((L, 1))) + w                  # two bodies against three
    per = lambda n: WP(w.target.reshape(-1, L, F // 4, 2)[:1].expand(n, -1, -1, -1), None, _scale=w.scale.reshape(-1, L, F // 4)[0])
    qper = QD(q.S.reshape(-1, L, F, F)[:1].expand(2, -1, -1, -1), q.h.reshape(-1, L, F)[0])
    with pytest.raises(ValueError, match="different numbers of designs"):
        per(3) + qper
    s = per(3) + p
    with pytest.raises(ValueError, match="per-design tables for 3 designs, the batch has 2"):
        s.check_state(2, L, F // 4)
    with pytest.raises(ValueError, match="rows, the state has"):
        (q + w).check_state(B, L + 1, F // 4)
    with pytest.raises(ValueError, match="last_n_step"):
        (PT([0.0, 0.0], L + 1) + p).check_state(B, L, F // 4)


# ------------------------------------------------------------------ 6. descriptor, sharding, header
def test_descriptor():
    x, q, w, p = _three()
    d = (q + w + p).descriptor("standard-alpha-recurrence-3")
    assert (d.mode, d.alpha, d.recurrence, d.last_n_step) == (7, 1, 3, 1 if w.design_fn_mode == "L2" else 2)
    assert d.time_consistency_coef == q.time_consistency_coef + w.time_consistency_coef + p.time_consistency_coef
    w2 = WP(w.target, None, _scale=w.scale, design_fn_mode="L2square")
    assert (w2 + p).descriptor("standard").last_n_step == 2 and (q + p).descriptor("standard").last_n_step == 0
    assert (q + p).descriptor("standard").recurrence == 0
    for g in ("universal-forward", "universal-backward-recurrence-2", "standard-recurrence-0"):
        assert (q + w + p).descriptor(g) is None


def test_shard():
    c = next(c for c in SC.CASES if c.terms == "qwp" and c.B == 3)
    d = SC.inputs(c)
    obj = d["obj"]
    part = obj.shard(1, 3)
    assert isinstance(part, SumObjective) and part.per_design == 2 and obj.per_design == 3
    for t, s in zip(obj.terms, part.terms):
        assert type(t) is type(s)
        for name, rank in t._TABLES:
            a, b = getattr(t, name), getattr(s, name)
            if a.dim() == rank + 1:
                assert torch.equal(b, a[1:3])
            else:
                assert b is a
    x = d["x"]
    assert torch.equal(part.closed_form_grad(x[1:3]), obj.closed_form_grad(x)[1:3])
    pt = PT([0.25, -0.5], 3) + obj.terms[2]
    assert pt.shard(0, 2).terms[0] is pt.terms[0]
    assert cindm_amd.SumObjective is SumObjective and "SumObjective" in cindm_amd.__all__


def test_header_names_mode_7():
    text = open(os.path.join(ROOT, "include", "cindm_hip.h")).read()
    assert "Mode 7 is the sum of every kind of table armed on the handle" in text and "7 = the sum of the tables armed" in text
    assert "it names the waypoint term's norm, 1 = \"L2\", 2 = \"L2square\"" in text
    assert "#define CINDM_ABI_VERSION 4" in text
