"""Host side of the pair-distance objective (cindm_amd.PairDistanceObjective, cindm_ddpm1d_set_design_pairdist): no device.

``closed_form_grad`` restates the gradient of compose_update_pair_kernel in torch, operation for operation.  In float64 it is held
against autograd of ``__call__`` (1e-12 relative); in fp32 against the float64 gradient with the bound of its rounding count.

The fp32 bound.  u = 2^-24, inputs exact.  One term of body i against body o, with (w, lo, hi) the pair's entry, is
    d = x_i - x_o  (1 rounding, and d' likewise);  r = sqrt(d d + d' d')  (products 1 each, sum 1, root 1);
    e = r - bound  (1);  term = (((w 2) e) d) / r  (w 2 is exact; product 1, product 1, quotient 1).
First order, relative: d carries u; d d carries 2u + u; the sum of the two non-negative squares 3u + u; the root half of that + u: r
carries 3u.  e has the ABSOLUTE error 3u r + u |e| <= 4u (r + bound): the subtraction cancels, so the term is measured by its absolute
form  A = 2 w (r + bound) |d| / r,  not by its value.  Against A the term carries 4 (from e) + 1 (w2 e) + 1 (d) + 1 (the product)
+ 3 (r below the bar) + 1 (the quotient) = 11 roundings.  The sum over the nb - 1 other bodies starts from 0.f (its first addition is
exact) and rounds nb - 2 times, each within u sum_o A.  An entry whose r is within 3u r of its bound may be taken for active on one
side and inactive on the other: the term it then lacks is below 2 w 3u r |d| / r <= 3u A, inside the 11.  One more u covers the
second-order terms ((1 + u)^11 - 1 < 11 u (1 + 6u)).  Count: 11 + (nb - 2) + 1 = nb + 10; the bound asserted per position element is

    (nb + 10) * 2^-24 * sum_{o != i} A(i, o),      bound = lo where r < lo, hi where r > hi, r in between (A = 4 w |d|), A = 0 where w = 0.

The fp32 cases run without the time-consistency term (it is the other objectives' expression, held by their files); the float64
cases run with it."""
import ctypes as C
import os
import re

import pytest
import torch

import cindm_amd
from cindm_amd import _ffi
from cindm_amd.objectives import pair_index

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24
PD = cindm_amd.PairDistanceObjective
INF = float("inf")


def _pairs(nb):
    return [(i, j) for i in range(nb) for j in range(i + 1, nb)]


def _case(seed, B, L, nb, per_band, per_w, tc=0.0, dtype=torch.float32):
    """Mixed relations: entry k of a table is apart / within / at by k % 3, a fifth of the weights are 0; positions in [-1, 1]
    redrawn until every pair of every row is more than 1e-3 apart.  Distances of such positions spread over 0 .. 2.8 and the bounds
    over 0.2 .. 1.4, so active and inactive entries both occur (asserted)."""
    g = torch.Generator().manual_seed(seed)
    P = nb * (nb - 1) // 2
    bs = ((B,) if per_band else ()) + (L, P)
    d = torch.rand(bs, generator=g) * 1.2 + 0.2
    kind = torch.arange(d.numel()).reshape(bs) % 3
    lo = torch.where(kind == 1, torch.zeros_like(d), d)
    hi = torch.where(kind == 0, torch.full_like(d, INF), d)
    ws = ((B,) if per_w else ()) + (L, P)
    w = (torch.rand(ws, generator=g) + 0.5) * (torch.rand(ws, generator=g) > 0.2)
    while True:
        pos = torch.rand((B, L, 4 * nb), generator=g) * 2 - 1
        x = pos.reshape(B, L, nb, 4)[..., :2].double()
        if all(float((x[:, :, i] - x[:, :, j]).norm(dim=-1).min()) > 1e-3 for i, j in _pairs(nb)):
            break
    return PD(lo, hi, w, time_consistency_coef=tc), pos.to(dtype)


def _f64_grad(obj, pos):
    x = pos.double().clone().requires_grad_()
    return torch.autograd.grad(obj(x), x)[0]


def _bound(obj, pos):
    B, L, F = pos.shape
    nb = F // 4
    x = pos.double().reshape(B, L, nb, 4)[..., :2]
    lo, hi, w = (v.double().unsqueeze(-1) for v in (obj.lo, obj.hi, obj.weight))
    A = torch.zeros_like(x)
    for i in range(nb):
        for o in range(nb):
            if o != i:
                p = pair_index(min(i, o), max(i, o), nb)
                d = x[:, :, i] - x[:, :, o]
                r = d.norm(dim=-1, keepdim=True)
                bound = torch.minimum(hi[..., p, :], torch.maximum(lo[..., p, :], r))
                A[:, :, i] += 2.0 * w[..., p, :] * (r + bound) * d.abs() / r
    out = torch.zeros((B, L, nb, 4), dtype=torch.float64)
    out[..., :2] = (nb + 10) * U * A
    return out.reshape(B, L, F)


def _active_share(obj, pos):
    """(share of the weighted entries that are active, number of weighted entries) at pos."""
    B, L, F = pos.shape
    nb = F // 4
    x = pos.double().reshape(B, L, nb, 4)[..., :2]
    I, J = (torch.tensor(v) for v in zip(*_pairs(nb)))
    r = (x[:, :, I] - x[:, :, J]).norm(dim=-1)
    on = (obj.weight > 0).expand(r.shape)
    act = on & ((r < obj.lo.double()) | (r > obj.hi.double()))
    return float(act.sum()) / float(on.sum()), int(on.sum())


# ------------------------------------------------------------------ 1. the gradient
@pytest.mark.parametrize("per_band,per_w", [(False, False), (True, True), (True, False), (False, True)])
@pytest.mark.parametrize("nb", [2, 3, 4])
def test_closed_form_is_autograd_in_float64(nb, per_band, per_w):
    for k, tc in enumerate((0.0, 0.5)):
        obj, pos = _case(100 + 10 * nb + k, 3, 6, nb, per_band, per_w, tc, dtype=torch.float64)
        share, n = _active_share(obj, pos)
        assert 0.0 < share < 1.0 and n >= 6, (share, n)          # active and inactive entries both occur
        assert {bool(torch.isinf(obj.hi).any()), bool((obj.lo == 0).any()), bool((obj.lo == obj.hi).any())} == {True}
        got, want = obj.closed_form_grad(pos), _f64_grad(obj, pos)
        assert got.dtype == torch.float64 and got.shape == pos.shape
        rel = float((got - want).abs().max() / want.abs().max())
        print(f"[pairdist] float64 nb={nb} per_band={per_band} per_w={per_w} tc={tc}: max err / max |grad| = {rel:.2e}")
        assert float(want.abs().max()) > 0.1 and rel <= 1e-12
        assert float(got.reshape(3, 6, nb, 4)[..., 2:].abs().max()) == 0.0          # velocities get no term


@pytest.mark.parametrize("per_band,per_w", [(False, False), (True, True), (True, False), (False, True)])
@pytest.mark.parametrize("nb", [2, 3, 4, 8])
def test_fp32_closed_form_within_its_rounding_count(nb, per_band, per_w):
    obj, pos = _case(200 + nb, 3, 7, nb, per_band, per_w)
    want, bound = _f64_grad(obj, pos), _bound(obj, pos)
    got = obj.closed_form_grad(pos)
    assert got.dtype == torch.float32 and got.shape == pos.shape
    err = (got.double() - want).abs()
    posf = (torch.arange(4 * nb) % 4) < 2
    on = bound[..., posf] > 0
    print(f"[pairdist] fp32 nb={nb} per_band={per_band} per_w={per_w}: max err / bound = "
          f"{float((err[..., posf][on] / bound[..., posf][on]).max()):.3f} (count {nb + 10})")
    assert bool((err <= bound).all())
    assert float(want.abs().max()) > 0.1


def test_ascending_sum_and_pair_order():
    """Three bodies on one row, one relation per pair: the gradient of body 1 is term(1, 0) + term(1, 2) with the entries of pairs
    (0, 1) = 0 and (1, 2) = 2 -- a table read in another pair order gives another number."""
    assert [pair_index(i, j, 4) for i, j in _pairs(4)] == list(range(6)) and pair_index(1, 2, 3) == 2
    pos = torch.zeros((1, 1, 12), dtype=torch.float64)
    pos[0, 0, 0], pos[0, 0, 4], pos[0, 0, 8], pos[0, 0, 9] = -1.0, 0.0, 0.0, 2.0        # body 0 (-1, 0), body 1 (0, 0), body 2 (0, 2)
    lo = torch.tensor([[2.0, 0.0, 0.0]])
    hi = torch.tensor([[INF, INF, 1.0]])
    w = torch.tensor([[1.0, 0.0, 0.5]])
    g = PD(lo, hi, w).closed_form_grad(pos).reshape(3, 4)
    # pair (0, 1): r = 1 < 2: 2 (1 - 2) d / 1 with d = +1 on body 1's x; pair (1, 2): r = 2 > 1: 0.5 2 (2 - 1) d / 2 with d = -2 on body 1's y
    assert g[1].tolist() == [-2.0, -1.0, 0.0, 0.0] and g[0].tolist() == [2.0, 0.0, 0.0, 0.0] and g[2].tolist() == [0.0, 1.0, 0.0, 0.0]
    assert torch.equal(g.reshape(1, 1, 12), _f64_grad(PD(lo, hi, w), pos))


def test_coincident_bodies_have_a_finite_value_and_a_zero_gradient():
    obj, pos = _case(300, 2, 5, 2, False, False, dtype=torch.float64)
    obj = PD.apart(0.7, torch.ones((5, 1)))
    pos[1, 3, 4:6] = pos[1, 3, 0:2]                                     # bodies 0 and 1 of design 1 coincide at row 3
    v = obj(pos)
    assert bool(torch.isfinite(v))
    lone = pos.clone()
    lone[1, 3, 4:6] += 5.0
    assert abs(float(v - obj(lone)) - 0.7 ** 2) < 1e-6                  # r = 0 < lo: the pair counts with w lo^2, a constant
    for dtype in (torch.float64, torch.float32):
        g = obj.closed_form_grad(pos.to(dtype))
        assert float(g[1, 3].abs().max()) == 0.0 and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0.0
        x = pos.to(dtype).clone().requires_grad_()
        ga = torch.autograd.grad(obj(x), x)[0]
        assert bool(torch.isfinite(ga).all()) and float(ga[1, 3].abs().max()) == 0.0
    # with three bodies only the coincident pair drops out
    o3 = PD.at(0.5, torch.ones((1, 3)))
    p3 = torch.tensor([[[0.0, 0.0, 0, 0, 0.0, 0.0, 0, 0, 2.0, 0.0, 0, 0]]], dtype=torch.float64)
    g3 = o3.closed_form_grad(p3).reshape(3, 4)
    assert g3[0].tolist() == g3[1].tolist() == [-3.0, 0.0, 0.0, 0.0] and g3[2].tolist() == [6.0, 0.0, 0.0, 0.0]
    assert torch.equal(g3.reshape(1, 1, 12), _f64_grad(o3, p3))


def test_constructors_are_the_explicit_bands():
    g = torch.Generator().manual_seed(4)
    d, w = torch.rand((5, 3), generator=g) + 0.1, torch.rand((2, 5, 3), generator=g)
    for made, lo, hi in ((PD.apart(d, w), d, torch.full_like(d, INF)), (PD.within(d, w), torch.zeros_like(d), d), (PD.at(d, w), d, d)):
        want = PD(lo, hi, w)
        assert torch.equal(made.lo, want.lo) and torch.equal(made.hi, want.hi) and torch.equal(made.weight, want.weight)
        assert (made.rows, made.n_bodies, made.per_design) == (5, 3, 2)
    o = PD.apart(0.4, torch.ones((5, 6)), time_consistency_coef=0.25)       # a number broadcasts; hi = inf is accepted
    assert o.lo.shape == (5, 6) and bool((o.lo == torch.tensor(0.4)).all()) and bool(torch.isinf(o.hi).all())
    assert (o.n_bodies, o.per_design, o.time_consistency_coef) == (4, None, 0.25)
    dB = torch.rand((2, 5, 3), generator=g)
    assert PD.within(dB, torch.ones((5, 3))).per_design == 2
    # device tables: (lo, hi) interleaved; lo and hi share one flag, the weight has its own
    band, wt = PD(dB, torch.full((5, 3), INF), torch.ones((5, 3))).tables("cpu")
    assert band.shape == (2, 5, 3, 2) and wt.shape == (5, 3) and band.is_contiguous()
    assert torch.equal(band[..., 0], dB) and bool(torch.isinf(band[..., 1]).all())
    band, wt = PD.at(d, w).tables("cpu")
    assert band.shape == (5, 3, 2) and wt.shape == (2, 5, 3) and torch.equal(band[..., 0], d) and torch.equal(band[..., 1], d)


@pytest.mark.parametrize("nb", [2, 3])
def test_at_zero_is_the_quadratic_objective_of_the_differences(nb):
    B, L, F = 2, 5, 4 * nb
    g = torch.Generator().manual_seed(5)
    P = nb * (nb - 1) // 2
    # (weights are multiples of 1/8: the quadratic tables hold sums of them and are cast to fp32 once -- these sums are exact there)
    w = torch.randint(4, 13, (L, P), generator=g).float() / 8 * (torch.rand((L, P), generator=g) > 0.3)
    rows, A, wt = [], [], []
    for l in range(L):
        for p, (i, j) in enumerate(_pairs(nb)):
            for c in (0, 1):
                a = torch.zeros(F, dtype=torch.float64)
                a[4 * i + c], a[4 * j + c] = 1.0, -1.0
                rows.append(l); A.append(a); wt.append(2.0 * float(w[l, p]))      # 1/2 (2 w) res^2 = w res^2
    quad = cindm_amd.QuadraticObjective.from_residuals(rows, torch.stack(A), torch.zeros(len(rows)), torch.tensor(wt), L, F,
                                                       time_consistency_coef=0.5)
    obj = PD.at(0.0, w, time_consistency_coef=0.5)
    pos = torch.rand((B, L, F), generator=g, dtype=torch.float64) * 2 - 1
    a, b = _f64_grad(obj, pos), _f64_grad(quad, pos)
    assert float(b.abs().max()) > 0.1 and float((a - b).abs().max()) <= 1e-12 * float(b.abs().max())
    assert float((obj.closed_form_grad(pos) - quad.closed_form_grad(pos)).abs().max()) <= 1e-12 * float(b.abs().max())
    assert abs(float(obj(pos) - quad(pos))) <= 1e-12 * abs(float(quad(pos)))


# ------------------------------------------------------------------ 2. refusals and shape logic
def test_constructor_refusals():
    lo, hi, w = torch.full((5, 3), 0.5), torch.full((5, 3), 1.0), torch.ones((5, 3))
    bad = lambda t, v: (lambda c: (c.__setitem__((1, 2), v), c)[1])(t.clone())
    for args, why in (((bad(lo, -0.1), hi, w), "lo must be"), ((bad(lo, INF), torch.full((5, 3), INF), w), "lo must be"),
                      ((bad(lo, float("nan")), hi, w), "lo must be"), ((lo, bad(hi, 0.25), w), "hi must be"),
                      ((lo, bad(hi, float("nan")), w), "hi must be"), ((lo, hi, bad(w, -1.0)), "weight must be"),
                      ((lo, hi, bad(w, INF)), "weight must be"), ((lo, hi, bad(w, float("nan"))), "weight must be")):
        with pytest.raises(ValueError, match=why):
            PD(*args)
    for P in (2, 4, 5, 36, 0):
        with pytest.raises(ValueError):
            PD(torch.zeros((5, P)), torch.ones((5, P)), torch.ones((5, P)))
    for args, why in (((torch.zeros((3,)), hi, w), r"\[L, P\]"), ((lo, torch.ones((1, 2, 5, 3)), w), r"\[L, P\]"),
                      ((lo, hi, torch.ones((4, 3))), "disagree"), ((lo, torch.ones((5, 6)), w), "disagree"),
                      ((lo.expand(2, 5, 3), hi, w.expand(3, 5, 3)), "number of designs"),
                      ((lo.expand(2, 5, 3), hi.expand(4, 5, 3), w), "number of designs"),
                      ((torch.zeros((0, 3)), torch.zeros((0, 3)), torch.zeros((0, 3))), r"\[L, P\]")):
        with pytest.raises(ValueError, match=why):
            PD(*args)
    ok = PD(lo, hi, w, time_consistency_coef=0.25)
    assert (ok.rows, ok.n_bodies, ok.per_design, ok.time_consistency_coef) == (5, 3, None, 0.25)
    for B, L, nb in ((1, 6, 3), (1, 5, 2), (1, 5, 4)):
        with pytest.raises(ValueError, match="PairDistanceObjective"):
            ok.check_state(B, L, nb)
    ok.check_state(7, 5, 3)
    with pytest.raises(ValueError, match="designs"):
        PD(lo.expand(2, 5, 3), hi, w).check_state(3, 5, 3)
    PD(torch.zeros((2, 28)), torch.ones((2, 28)), torch.ones((2, 28)))          # 8 bodies is the largest
    assert "PairDistanceObjective" in cindm_amd.__all__


def test_descriptor():
    o = PD.apart(0.5, torch.ones((5, 1)), time_consistency_coef=0.25)
    d = o.descriptor("standard")
    assert (d.mode, d.alpha, d.recurrence) == (6, 0, 0) and d.time_consistency_coef == 0.25
    d = o.descriptor("standard-alpha")
    assert (d.mode, d.alpha, d.recurrence) == (6, 1, 0)
    d = o.descriptor("standard-recurrence-10")
    assert (d.mode, d.alpha, d.recurrence) == (6, 0, 10)
    d = o.descriptor("standard-alpha-recurrence-1")
    assert (d.mode, d.alpha, d.recurrence) == (6, 1, 1)
    assert (d.last_n_step, d.coef, d.pos_target[0], d.pos_target[1]) == (0, 0.0, 0.0, 0.0)       # not read in mode 6
    for g in ("universal-forward", "universal-backward", "universal-forward-recurrence-2", "standard-recurrence-0",
              "standard-alpha-recurrence-0", "unknown", "unknown-recurrence-2", "standard-beta"):
        assert o.descriptor(g) is None, g


def test_shard_slices_per_design_tables_only():
    B, L, P = 6, 4, 3
    g = torch.Generator().manual_seed(2)
    loB, wB = torch.rand((B, L, P), generator=g), torch.rand((B, L, P), generator=g)
    lo1, w1 = torch.rand((L, P), generator=g), torch.rand((L, P), generator=g)
    both = PD(loB, loB + 0.5, wB).shard(2, 5)
    assert torch.equal(both.lo, loB[2:5]) and torch.equal(both.hi, loB[2:5] + 0.5) and torch.equal(both.weight, wB[2:5])
    assert both.per_design == 3 and both.lo.is_contiguous() and both.weight.is_contiguous()
    assert both.tables("cpu")[0].shape == (3, L, P, 2)
    mixed = PD(lo1, lo1 + 0.5, wB).shard(0, 2)
    assert torch.equal(mixed.lo, lo1) and torch.equal(mixed.weight, wB[:2]) and mixed.per_design == 2
    mixed = PD(loB, torch.full((L, P), INF), w1).shard(4, 6)
    assert torch.equal(mixed.lo, loB[4:6]) and mixed.hi.shape == (L, P) and torch.equal(mixed.weight, w1) and mixed.per_design == 2
    assert mixed.tables("cpu")[0].shape == (2, L, P, 2)
    part = PD(lo1, lo1 + 0.5, w1, time_consistency_coef=0.5).shard(3, 6)
    assert torch.equal(part.lo, lo1) and part.per_design is None and part.time_consistency_coef == 0.5
    pos = torch.rand((B, L, 12), generator=g, dtype=torch.float64)
    whole = PD(loB, loB + 0.5, wB)
    assert abs(float(whole.shard(0, 2)(pos[:2]) + whole.shard(2, 6)(pos[2:])) - float(whole(pos))) < 1e-12 * abs(float(whole(pos)))
    with pytest.raises(ValueError, match="designs"):
        whole(pos[:4])


# ------------------------------------------------------------------ 3. the C entry
def test_c_entry_is_declared_bound_and_exported():
    name = "cindm_ddpm1d_set_design_pairdist"
    header = open(os.path.join(ROOT, "include", "cindm_hip.h")).read()
    assert re.search(r"int\s+" + name + r"\(cindm_ddpm1d\* h, const float\* band, int32_t band_per_design,\s*const float\* weight, "
                     r"int32_t weight_per_design,\s*int32_t rows, int32_t n_bodies, int64_t batch\);", header)
    assert re.search(r"#define\s+CINDM_ABI_VERSION\s+4\b", header)
    assert re.search(r"6 = pair-distance tables", header)
    assert name in _ffi.SIGNATURES and len(_ffi.SIGNATURES[name][1]) == 8
    assert _ffi.SIGNATURES[name] == _ffi.SIGNATURES["cindm_ddpm1d_set_design_quadratic"]
    L = _ffi.lib()
    assert L.cindm_abi_version() == _ffi.ABI_VERSION == 4
    buf = (C.c_float * 64)()
    assert getattr(L, name)(None, buf, 0, buf, 0, 2, 2, 1) != 0
    assert b"null handle" in L.cindm_last_error()
    assert getattr(L, name)(None, None, 0, None, 0, 0, 0, 0) != 0          # disarming needs a handle too
    assert L.cindm_last_error()
