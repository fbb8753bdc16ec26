"""Host side of the quadratic objective (cindm_amd.QuadraticObjective, cindm_ddpm1d_set_design_quadratic): no device.

``closed_form_grad`` restates the gradient of compose_update_quad_kernel in torch, operation for operation, in fp32.  It is held
against the float64 gradient of the value with the bound of its summation order.  With u = 2^-24, M[b, l, f] = sum_f' |S[l, f, f']|
|x[b, l, f']| + |h[l, f]|:  every product is rounded once, the sum runs from 0.f in ascending f' (its first addition is exact), so after
F terms the accumulator is within ((1 + u)^F - 1) sum |S||x| of the exact sum; the subtraction of h rounds once more, u |acc - h| <=
u (1 + F u) M.  To first order that is (F + 1) u M; the bound asserted is (F + 1) 2^-23 M = twice that, which covers the second-order
terms and, for autograd of ``__call__`` (another summation order, 1/2 (S x + S^T x), one addition more), the same first-order count + 1.

Time consistency: the bound has no term for the time-consistency gradient T = (2 tc) lap / (L - 1), whose own rounding is
E_tc <= u (4 k (|d1| + |d2|) + 3 |T|) + u M with k = 2 tc / (L - 1) and d1, d2 the two row differences (each difference, the sum of the
two, the product, the quotient and the final g + T round once; tc is a power of two here, so fp32(tc) = tc).  The tc > 0 cases therefore
use tables with an entry on every row and |h| >= 1.5, and ``_tc_fits`` asserts per element that E_tc is inside the bound's spare half,
0.9 (F + 1) u M: a case that does not leave that room fails there, by its own inputs, not by the code under test."""
import ctypes as C
import os
import re

import pytest
import torch

import cindm_amd
from cindm_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24
Q = cindm_amd.QuadraticObjective


def _sym(S):
    return ((S + S.transpose(-1, -2)) * 0.5).contiguous()          # (a + b == b + a and the halving are exact: symmetric bit for bit)


def _case(seed, B, L, nb, per_S, per_h, tc, dtype=torch.float32):
    """Dense tables of order 1 on every row, |h| in 1.5 .. 2.5 with random signs, pos in [-1, 1]."""
    g = torch.Generator().manual_seed(seed)
    F = 4 * nb
    S = _sym(torch.rand(((B,) if per_S else ()) + (L, F, F), generator=g) * 2 - 1)
    hs = ((B,) if per_h else ()) + (L, F)
    h = (torch.rand(hs, generator=g) + 1.5) * (torch.randint(0, 2, hs, generator=g) * 2 - 1)
    pos = (torch.rand((B, L, F), generator=g) * 2 - 1).to(dtype)
    return Q(S, h, time_consistency_coef=tc), pos


def _M(obj, pos):
    S, h = obj.S.double().abs(), obj.h.double().abs()
    return (S @ pos.double().abs().unsqueeze(-1)).squeeze(-1) + h


def _bound(obj, pos):
    return (pos.shape[-1] + 1) * 2.0 ** -23 * _M(obj, pos)


def _tc_fits(obj, pos):
    """The precondition of a tc > 0 case (module docstring): the time-consistency term's own rounding fits the bound's spare half."""
    B, L, F = pos.shape
    x = pos.double()
    k = 2.0 * obj.time_consistency_coef / (L - 1)
    d = (x[:, 1:] - x[:, :-1]).abs()
    dsum = torch.zeros_like(x)
    dsum[:, 1:] += d
    dsum[:, :-1] += d
    e_tc = U * (4 * k * dsum + 3 * k * dsum) + U * _M(obj, pos)
    posf = (torch.arange(F) % 4) < 2
    return bool((e_tc[..., posf] <= 0.9 * (F + 1) * U * _M(obj, pos)[..., posf]).all())


def _f64_grad(obj, pos):
    x = pos.double().clone().requires_grad_()
    return torch.autograd.grad(obj(x), x)[0]


def _autograd(obj, pos):
    x = pos.clone().requires_grad_()
    return torch.autograd.grad(obj(x), x)[0]


# ------------------------------------------------------------------ 1. gradient bound
@pytest.mark.parametrize("tc", [0.0, 0.5])
@pytest.mark.parametrize("per_S,per_h", [(False, False), (True, True), (True, False), (False, True)])
def test_gradient_bound(tc, per_S, per_h):
    for seed, (B, L, nb) in enumerate([(3, 7, 2), (2, 5, 4), (2, 9, 1), (1, 2, 8)]):
        obj, pos = _case(200 + seed, B, L, nb, per_S, per_h, tc)
        if tc > 0:
            assert _tc_fits(obj, pos), (B, L, nb)
        want, bound = _f64_grad(obj, pos), _bound(obj, pos)
        got = obj.closed_form_grad(pos)
        assert got.shape == pos.shape and got.dtype == torch.float32
        err = (got.double() - want).abs()
        print(f"[quadratic] closed form B={B} L={L} F={4 * nb} tc={tc}: max err / bound = {float((err / bound).max()):.3f}")
        assert bool((err <= bound).all())
        err = (_autograd(obj, pos).double() - want).abs()
        print(f"[quadratic] autograd    B={B} L={L} F={4 * nb} tc={tc}: max err / bound = {float((err / bound).max()):.3f}")
        assert bool((err <= bound).all())
        # velocities are pulled: the first built-in objective whose gradient reaches them
        assert float(got.reshape(B, L, nb, 4)[..., 2:].abs().min()) > 0.0


def test_gradient_is_exact_in_float64_and_sparse_rows_stay_zero():
    """In float64 the closed form and autograd differ by float64 rounding only; a row without terms has an exactly zero gradient."""
    obj, pos = _case(210, 2, 6, 2, True, True, 0.0, dtype=torch.float64)
    S, h = obj.S.clone(), obj.h.clone()
    S[:, 2], h[:, 2] = 0.0, 0.0
    obj = Q(S, h)
    got, want = obj.closed_form_grad(pos), _f64_grad(obj, pos)
    assert got.dtype == torch.float64 and float((got - want).abs().max()) < 1e-13
    assert float(got[:, 2].abs().max()) == 0.0 and float(want[:, 2].abs().max()) == 0.0


# ------------------------------------------------------------------ 2. from_residuals
def _residual_case(seed, B, L, F, M, per_A, per_r, per_w):
    g = torch.Generator().manual_seed(seed)
    rows = torch.randint(0, L, (M,), generator=g)
    rows[0], rows[-1] = 0, L - 1
    A = torch.randn(((B,) if per_A else ()) + (M, F), generator=g, dtype=torch.float64)
    r = torch.rand(((B,) if per_r else ()) + (M,), generator=g, dtype=torch.float64) * 1.2 - 0.6
    w = torch.rand(((B,) if per_w else ()) + (M,), generator=g, dtype=torch.float64) + 0.5
    w[..., 1::3] *= -0.25                                              # "keep apart": a negative weight
    return rows, A, r, w


@pytest.mark.parametrize("per_A,per_r,per_w", [(False, False, False), (True, True, True), (False, True, False), (False, False, True),
                                               (True, False, False)])
def test_from_residuals(per_A, per_r, per_w):
    B, L, F, M = 3, 6, 8, 11
    rows, A, r, w = _residual_case(300, B, L, F, M, per_A, per_r, per_w)
    obj = Q.from_residuals(rows, A, r, w, L, F, time_consistency_coef=0.0)
    assert torch.equal(obj.S, obj.S.transpose(-1, -2)) and obj.S.dtype == torch.float32 and obj.h.dtype == torch.float32
    assert (obj.S.dim() == 4) == (per_A or per_w) and (obj.h.dim() == 3) == (per_A or per_r or per_w)
    assert (obj.rows, obj.features) == (L, F) and obj.per_design == (B if (per_A or per_r or per_w) else None)
    pos = torch.rand((B, L, F), generator=torch.Generator().manual_seed(301), dtype=torch.float64) * 2 - 1
    Ab, rb, wb = (v.expand((B,) + tuple(v.shape[-n:])) for v, n in ((A, 2), (r, 1), (w, 1)))
    res = torch.einsum("bmf,bmf->bm", Ab, pos[:, rows]) - rb
    want = 0.5 * (wb * res.square()).sum() - 0.5 * (wb * rb.square()).sum()
    # the tables were cast to fp32 once: every entry moved by at most u relative, so the value moved by at most
    # u sum (1/2 |x|^T |S| |x| + |h|^T |x|) <= sum_f |x_f| u M_f -- inside sum_f |x_f| bound_f, "the same bound" contracted with |x|
    tol = float((pos.abs() * _bound(obj, pos)).sum())
    print(f"[quadratic] from_residuals: |value - direct| / tol = {abs(float(obj(pos)) - float(want)) / tol:.3f}")
    assert abs(float(obj(pos)) - float(want)) <= tol
    # the gradient of the direct form, likewise
    x = pos.clone().requires_grad_()
    resx = torch.einsum("bmf,bmf->bm", Ab, x[:, rows]) - rb
    gd = torch.autograd.grad(0.5 * (wb * resx.square()).sum(), x)[0]
    assert bool(((obj.closed_form_grad(pos) - gd).abs() <= _bound(obj, pos)).all())


def test_from_residuals_keeps_a_negative_weight():
    L, F = 4, 8
    a = torch.zeros((1, F), dtype=torch.float64)
    a[0, 0], a[0, 4] = 1.0, -1.0                                       # x position of body 0 minus x position of body 1
    obj = Q.from_residuals([2], a, [0.0], [-0.75], L, F)
    assert float(obj.S[2, 0, 0]) == -0.75 == float(obj.S[2, 4, 4]) and float(obj.S[2, 0, 4]) == 0.75 == float(obj.S[2, 4, 0])
    assert float(obj.S.abs().sum()) == 3.0 and float(obj.h.abs().sum()) == 0.0
    pos = torch.zeros((1, L, F), dtype=torch.float64)
    pos[0, 2, 0], pos[0, 2, 4] = 0.5, -0.5
    assert float(obj(pos)) == -0.375                                   # 1/2 * -0.75 * (0.5 - -0.5)^2: apart is lower
    g = obj.closed_form_grad(pos)
    assert float(g[0, 2, 0]) == -0.75 and float(g[0, 2, 4]) == 0.75    # descending it pushes the two further apart
    for bad in (dict(rows=[4]), dict(A=torch.zeros((1, 7))), dict(r=[0.0, 1.0]), dict(weight=torch.ones((2, 2)))):
        kw = dict(rows=[2], A=a, r=[0.0], weight=[1.0])
        kw.update(bad)
        with pytest.raises(ValueError):
            Q.from_residuals(kw["rows"], kw["A"], kw["r"], kw["weight"], L, F)
    with pytest.raises(ValueError, match="number of designs"):
        Q.from_residuals([2], a.expand(2, 1, F), torch.zeros((3, 1)), [1.0], L, F)


# ------------------------------------------------------------------ 3. refusals and shape logic
def test_constructor_refusals():
    S, h = torch.zeros((5, 8, 8)), torch.ones((5, 8))
    ns = S.clone(); ns[1, 2, 3] = 1e-30                                 # not symmetric by the smallest of margins
    with pytest.raises(ValueError, match="symmetric"):
        Q(ns, h)
    for bad_S, bad_h in ((S + float("nan"), h), (S, h * float("inf")), (S + float("inf"), h), (S, h * float("nan"))):
        with pytest.raises(ValueError, match="finite"):
            Q(bad_S, bad_h)
    for F in (6, 36, 2, 0):
        with pytest.raises(ValueError):
            Q(torch.zeros((5, F, F)), torch.zeros((5, F)))
    for SS, hh in ((torch.zeros((5, 8, 4)), h), (torch.zeros((8, 8)), h), (S, torch.ones((8,))), (S, torch.ones((4, 8))),
                   (S, torch.ones((5, 4))), (torch.zeros((3, 5, 8, 8)), torch.ones((4, 5, 8))), (torch.zeros((0, 8, 8)), torch.ones((0, 8)))):
        with pytest.raises(ValueError):
            Q(SS, hh)
    ok = Q(S, h, time_consistency_coef=0.25)
    assert (ok.rows, ok.features, ok.per_design, ok.time_consistency_coef) == (5, 8, None, 0.25)
    for B, L, nb in ((1, 6, 2), (1, 5, 3)):
        with pytest.raises(ValueError, match="QuadraticObjective"):
            ok.check_state(B, L, nb)
    ok.check_state(7, 5, 2)
    Q(torch.zeros((5, 32, 32)), torch.zeros((5, 32)))                   # F = 32 is the largest
    assert cindm_amd.QuadraticObjective is Q and "QuadraticObjective" in cindm_amd.__all__


def test_descriptor():
    o = Q(torch.zeros((5, 8, 8)), torch.ones((5, 8)), time_consistency_coef=0.25)
    d = o.descriptor("standard")
    assert (d.mode, d.alpha, d.recurrence) == (5, 0, 0) and d.time_consistency_coef == 0.25
    d = o.descriptor("standard-alpha")
    assert (d.mode, d.alpha, d.recurrence) == (5, 1, 0)
    d = o.descriptor("standard-recurrence-10")
    assert (d.mode, d.alpha, d.recurrence) == (5, 0, 10)
    d = o.descriptor("standard-alpha-recurrence-1")
    assert (d.mode, d.alpha, d.recurrence) == (5, 1, 1)
    assert (d.last_n_step, d.coef, d.pos_target[0], d.pos_target[1]) == (0, 0.0, 0.0, 0.0)       # not read in mode 5
    for g in ("universal-forward", "universal-backward", "universal-forward-recurrence-2", "standard-recurrence-0",
              "standard-alpha-recurrence-0", "unknown", "unknown-recurrence-2", "standard-beta"):
        assert o.descriptor(g) is None, g


def test_shard_slices_per_design_tables_only():
    B, L, F = 6, 4, 8
    g = torch.Generator().manual_seed(2)
    Sb, hb = _sym(torch.rand((B, L, F, F), generator=g)), torch.rand((B, L, F), generator=g)
    S1, h1 = _sym(torch.rand((L, F, F), generator=g)), torch.rand((L, F), generator=g)
    both = Q(Sb, hb).shard(2, 5)
    assert torch.equal(both.S, Sb[2:5]) and torch.equal(both.h, hb[2:5]) and both.per_design == 3
    assert both.S.is_contiguous() and both.h.is_contiguous()
    mixed = Q(S1, hb).shard(0, 2)
    assert torch.equal(mixed.S, S1) and torch.equal(mixed.h, hb[:2]) and mixed.per_design == 2
    mixed = Q(Sb, h1).shard(4, 6)
    assert torch.equal(mixed.S, Sb[4:6]) and torch.equal(mixed.h, h1) and mixed.per_design == 2
    part = Q(S1, h1, time_consistency_coef=0.5).shard(3, 6)
    assert torch.equal(part.S, S1) and torch.equal(part.h, h1) and part.per_design is None and part.time_consistency_coef == 0.5
    pos = torch.rand((B, L, F), generator=g, dtype=torch.float64)
    whole = Q(Sb, hb)
    assert abs(float(whole.shard(0, 2)(pos[:2]) + whole.shard(2, 6)(pos[2:])) - float(whole(pos))) < 1e-12 * abs(float(whole(pos)))
    with pytest.raises(ValueError, match="designs"):
        whole(pos[:4])


# ------------------------------------------------------------------ 4. the C entry
def test_c_entry_is_declared_bound_and_exported():
    name = "cindm_ddpm1d_set_design_quadratic"
    header = open(os.path.join(ROOT, "include", "cindm_hip.h")).read()
    assert re.search(r"int\s+" + name + r"\(cindm_ddpm1d\* h, const float\* S, int32_t S_per_design,\s*const float\* hvec, "
                     r"int32_t h_per_design,\s*int32_t rows, int32_t features, int64_t batch\);", header)
    assert re.search(r"#define\s+CINDM_ABI_VERSION\s+4\b", header)
    assert name in _ffi.SIGNATURES and len(_ffi.SIGNATURES[name][1]) == 8
    L = _ffi.lib()
    assert L.cindm_abi_version() == _ffi.ABI_VERSION == 4
    buf = (C.c_float * 64)()
    assert getattr(L, name)(None, buf, 0, buf, 0, 2, 4, 1) != 0
    assert b"null handle" in L.cindm_last_error()
    assert getattr(L, name)(None, None, 0, None, 0, 0, 0, 0) != 0          # disarming needs a handle too
    assert L.cindm_last_error()
