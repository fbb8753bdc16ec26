"""Host side of the waypoint objective (cindm_amd.WaypointObjective, cindm_ddpm1d_set_design_tables): no device.

``closed_form_grad`` restates the update kernel's table branch in torch, operation for operation; here it is held against autograd of
``__call__`` in fp64, where the two differ by rounding only (bound 1e-12 relative to the gradient's largest entry: a gradient entry is
a handful of fp64 operations on values of order 1 .. 100, each exact to 1.1e-16)."""
import ctypes as C
import os
import re

import pytest
import torch

import cindm_amd
from cindm_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp(min=1e-300))


def _autograd(obj, pos):
    x = pos.clone().requires_grad_()
    return torch.autograd.grad(obj(x), x)[0]


def _random_case(seed, B, L, nb, per_design_target, per_design_weight, **kw):
    g = torch.Generator().manual_seed(seed)
    target = torch.rand(((B,) if per_design_target else ()) + (L, nb, 2), generator=g) * 2 - 1
    wshape = ((B,) if per_design_weight else ()) + (L, nb)
    weight = torch.rand(wshape, generator=g) * 3
    weight = weight * (torch.rand(wshape, generator=g) > 0.4)          # some entries carry no waypoint
    weight.view(-1)[0], weight.view(-1)[-1] = 0.0, 1.25
    assert bool((weight == 0).any()) and bool((weight > 0).any())
    pos = (torch.rand((B, L, 4 * nb), generator=g, dtype=torch.float64) * 2 - 1)
    return cindm_amd.WaypointObjective(target, weight, **kw), pos


@pytest.mark.parametrize("mode", ["L2", "L2square"])
@pytest.mark.parametrize("tc", [0.0, 0.5])
@pytest.mark.parametrize("ptarget,pweight", [(False, False), (True, True), (True, False), (False, True)])
def test_closed_form_gradient_is_the_gradient_of_the_value(mode, tc, ptarget, pweight):
    for seed, (B, L, nb) in enumerate([(3, 7, 2), (2, 5, 4), (1, 2, 1)]):
        obj, pos = _random_case(100 + seed, B, L, nb, ptarget, pweight, coef=1.7, time_consistency_coef=tc, design_fn_mode=mode)
        got, want = obj.closed_form_grad(pos), _autograd(obj, pos)
        assert got.shape == pos.shape and got.dtype == torch.float64
        assert _rel(got, want) < 1e-12
        assert float(got.reshape(B, L, nb, 4)[..., 2:].abs().max()) == 0.0          # velocities are not pulled


@pytest.mark.parametrize("mode", ["L2", "L2square"])
@pytest.mark.parametrize("tc", [0.0, 0.5])
def test_from_point_restates_the_point_objective(mode, tc):
    """The scale table holds fp32(coef) / fp32(n), the division the kernel's point branch does.  Where that quotient is exact (n a power
    of two) the table form is held against the PointObjective of the same arguments; for n = 3, coef = 100 the table is asserted
    exactly and the comparison is against the PointObjective whose Python-float coef / n IS that fp32 quotient (coef = scale * 3:
    exact in fp64, and exact again when divided by 3).  Bound 1e-12 throughout."""
    L, nb, B = 9, 3, 2
    pos = torch.rand((B, L, 4 * nb), generator=torch.Generator().manual_seed(5), dtype=torch.float64) * 2 - 1
    for n, coef in ((1, 100), (2, 100), (4, 2.5), (8, 3), (3, 100)):
        wp = cindm_amd.WaypointObjective.from_point([0.25, -0.5], n, L, nb, coef=coef, time_consistency_coef=tc, design_fn_mode=mode)
        assert tuple(wp.target.shape) == (L, nb, 2) and tuple(wp.scale.shape) == (L, nb)
        want = torch.tensor(float(coef), dtype=torch.float32) / torch.tensor(float(n), dtype=torch.float32)
        assert bool((wp.scale[L - n:] == want).all()) and bool((wp.scale[:L - n] == 0).all())
        pt_coef = coef if n != 3 else float(want) * n
        assert pt_coef / n == float(want)
        pt = cindm_amd.PointObjective([0.25, -0.5], n, coef=pt_coef, time_consistency_coef=tc, design_fn_mode=mode)
        assert abs(float(wp(pos)) - float(pt(pos))) <= 1e-12 * abs(float(pt(pos)))
        assert _rel(_autograd(wp, pos), _autograd(pt, pos)) <= 1e-12
        assert _rel(wp.closed_form_grad(pos), _autograd(pt, pos)) <= 1e-12
    with pytest.raises(ValueError):
        cindm_amd.WaypointObjective.from_point([0.25, -0.5], L + 1, L, nb)


@pytest.mark.parametrize("mode", ["L2", "L2square"])
def test_zero_scale_entry_on_its_target_contributes_nothing(mode):
    L, nb, B = 4, 2, 2
    g = torch.Generator().manual_seed(9)
    target = torch.rand((L, nb, 2), generator=g)
    weight = torch.ones((L, nb)); weight[2, 1] = 0
    pos = torch.rand((B, L, 4 * nb), generator=g, dtype=torch.float64)
    pos[:, 2, 4:6] = target[2, 1].double()                   # pos == target exactly at the entry without a waypoint
    moved = target.clone(); moved[2, 1] += 0.375
    for tc in (0.0, 0.5):
        a = cindm_amd.WaypointObjective(target, weight, coef=2.0, time_consistency_coef=tc, design_fn_mode=mode)
        b = cindm_amd.WaypointObjective(moved, weight, coef=2.0, time_consistency_coef=tc, design_fn_mode=mode)
        for grad in (lambda o: _autograd(o, pos), lambda o: o.closed_form_grad(pos)):
            ga, gb = grad(a), grad(b)
            assert bool(torch.isfinite(ga).all())
            assert torch.equal(ga, gb)
        assert float(a(pos)) == float(b(pos))
        if tc == 0.0:
            assert float(_autograd(a, pos)[:, 2, 4:6].abs().max()) == 0.0 and float(a.closed_form_grad(pos)[:, 2, 4:6].abs().max()) == 0.0


def test_descriptor():
    t, w = torch.zeros((5, 2, 2)), torch.ones((5, 2))
    l2 = cindm_amd.WaypointObjective(t, w, coef=3.0, time_consistency_coef=0.25)
    sq = cindm_amd.WaypointObjective(t, w, design_fn_mode="L2square")
    d = l2.descriptor("standard")
    assert (d.mode, d.alpha, d.recurrence) == (3, 0, 0) and d.time_consistency_coef == 0.25
    d = sq.descriptor("standard-alpha")
    assert (d.mode, d.alpha, d.recurrence) == (4, 1, 0) and d.time_consistency_coef == 0.0
    d = l2.descriptor("standard-recurrence-10")
    assert (d.mode, d.alpha, d.recurrence) == (3, 0, 10)
    d = sq.descriptor("standard-alpha-recurrence-3")
    assert (d.mode, d.alpha, d.recurrence) == (4, 1, 3)
    assert (d.last_n_step, d.coef, d.pos_target[0], d.pos_target[1]) == (0, 0.0, 0.0, 0.0)       # not read in the table modes
    for g in ("universal-forward", "universal-backward", "universal-forward-recurrence-2", "standard-recurrence-0",
              "standard-alpha-recurrence-0"):
        assert l2.descriptor(g) is None, g
    with pytest.raises(ValueError):
        cindm_amd.WaypointObjective(t, w, design_fn_mode="L1")


def test_shard_slices_per_design_tables_only():
    B, L, nb = 6, 4, 2
    g = torch.Generator().manual_seed(2)
    tb, wb = torch.rand((B, L, nb, 2), generator=g), torch.rand((B, L, nb), generator=g)
    t1, w1 = torch.rand((L, nb, 2), generator=g), torch.rand((L, nb), generator=g)
    both = cindm_amd.WaypointObjective(tb, wb, coef=2.0).shard(2, 5)
    assert torch.equal(both.target, tb[2:5]) and torch.equal(both.scale, 2.0 * wb[2:5]) and both.per_design == 3
    assert both.target.is_contiguous() and both.scale.is_contiguous()
    mixed = cindm_amd.WaypointObjective(t1, wb).shard(0, 2)
    assert torch.equal(mixed.target, t1) and torch.equal(mixed.scale, wb[:2]) and mixed.per_design == 2
    shared = cindm_amd.WaypointObjective(t1, w1, time_consistency_coef=0.5, design_fn_mode="L2square")
    part = shared.shard(3, 6)
    assert torch.equal(part.target, t1) and torch.equal(part.scale, w1) and part.per_design is None
    assert (part.time_consistency_coef, part.design_fn_mode) == (0.5, "L2square")
    # the value of a shard is the value on its designs
    pos = torch.rand((B, L, 4 * nb), generator=g, dtype=torch.float64)
    whole = cindm_amd.WaypointObjective(tb, wb)
    assert abs(float(whole.shard(0, 2)(pos[:2]) + whole.shard(2, 6)(pos[2:])) - float(whole(pos))) < 1e-12 * float(whole(pos))
    with pytest.raises(ValueError, match="designs"):
        whole(pos[:4])


def test_constructor_refusals():
    t, w = torch.zeros((5, 2, 2)), torch.ones((5, 2))
    W = cindm_amd.WaypointObjective
    for bad in (-w, w * float("nan"), w * float("inf")):
        with pytest.raises(ValueError):
            W(t, bad)
    with pytest.raises(ValueError):
        W(t * float("nan"), w)
    for tt, ww in ((torch.zeros((5, 2, 3)), w), (torch.zeros((5, 2)), w), (t, torch.ones((5,))), (t, torch.ones((4, 2))),
                   (t, torch.ones((5, 3))), (torch.zeros((3, 5, 2, 2)), torch.ones((4, 5, 2))), (torch.zeros((0, 2, 2)), torch.ones((0, 2)))):
        with pytest.raises(ValueError):
            W(tt, ww)
    with pytest.raises(ValueError):
        W(t, w, coef=-1.0)                       # the scale table must stay >= 0
    ok = W(t, w)
    for B, L, nb in ((1, 6, 2), (1, 5, 3)):
        with pytest.raises(ValueError):
            ok.check_state(B, L, nb)
    ok.check_state(7, 5, 2)
    assert cindm_amd.WaypointObjective is W and "WaypointObjective" in cindm_amd.__all__


def test_c_entry_is_declared_bound_and_exported():
    name = "cindm_ddpm1d_set_design_tables"
    header = open(os.path.join(ROOT, "include", "cindm_hip.h")).read()
    assert re.search(r"int\s+" + name + r"\(cindm_ddpm1d\* h, const float\* target, int32_t target_per_design,", header)
    assert re.search(r"#define\s+CINDM_ABI_VERSION\s+4\b", header)
    assert name in _ffi.SIGNATURES and len(_ffi.SIGNATURES[name][1]) == 8
    L = _ffi.lib()
    assert L.cindm_abi_version() == _ffi.ABI_VERSION == 4
    buf = (C.c_float * 16)()
    assert getattr(L, name)(None, buf, 0, buf, 0, 2, 2, 1) != 0
    assert b"null handle" in L.cindm_last_error()
    assert getattr(L, name)(None, None, 0, None, 0, 0, 0, 0) != 0          # disarming needs a handle too
    assert L.cindm_last_error()
