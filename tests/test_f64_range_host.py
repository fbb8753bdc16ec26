"""CPU: the cases of tests/range_cases.py -- the edges of the split-fp16 range rule -- before they run on the GPU.

1. ``to_edge`` puts a tensor exactly on an edge of the window, or one fp32 number beyond it.
2. The plane model (``split_planes``) states what the window promises: at max|w| = 2^-12, with fp16 subnormals kept, every element is
   carried to 2^-24 of the tensor's maximum; with subnormals flushed the loss is 2^-13 (low plane only) or a quarter of the tensor
   (both planes).  A weight-standardised tensor of a checkpoint whose ``.proj.`` weights are x 2^-24 folds to a maximum of
   4.7e-7 .. 8.5e-7 and loses 1.7e-5 .. 3.1e-5 of it with subnormals KEPT: outside the window, which is why the rule looks at the
   folded tensors.
3. Yardsticks: at every case's own inputs the fp32 oracle and the float64 reference are finite at every tap, and the taps whose
   e32 is under the 2e-7 floor of ``_hold`` are exactly those pinned in ``range_cases.BELOW_FLOOR`` -- at most three per case, all at
   the first level.
4. Bite: the planes of one lower-edge convolution flushed inside the oracle move that block's tap by more than 10 x M x e32; with
   only the low plane flushed, eps stays under the older tests' 2e-5 in their whole-tensor norm (measured: tap 15 .. 17 x M x e32,
   eps 6e-6 .. 7e-6)."""
import numpy as np
import pytest
import torch

import cindm_oracle as O
import f64_reference as R
import range_cases as C

TOL_FWD = 2e-5            # tests/test_gpu_parity.py (not imported: that module needs the HIP library)
FLOOR = 2e-7              # tests/test_gpu_f64_budget.py::_hold
NOT_BLOCKS = ("temb", "mid")


# ------------------------------------------------------------------ to_edge
@pytest.mark.parametrize("edge", [C.LO, C.HI])
@pytest.mark.parametrize("outside", [False, True])
@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_to_edge(edge, outside, sign):
    w = torch.randn((7, 5, 3), generator=torch.Generator().manual_seed(2)) * 0.37 * sign
    i = int(w.abs().argmax())
    e = C.to_edge(w, edge, outside)
    assert e.dtype == torch.float32 and e.shape == w.shape
    top = float(e.abs().max())
    if outside:
        nb = np.nextafter(np.float32(edge), np.float32(0.0)) if edge < 1 else np.nextafter(np.float32(edge), np.float32(np.inf))
        assert top == float(nb) and top != edge and (top < edge) == (edge < 1)
    else:
        assert top == edge
    assert int(e.abs().argmax()) == i and float(e.flatten()[i]) == top * float(w.flatten()[i].sign())
    assert int((e.abs() == top).sum()) == 1                     # no other element reaches it (none goes beyond: top is the max)
    rest = torch.ones_like(w, dtype=torch.bool).flatten()
    rest[i] = False
    want = (w.double() * (edge / float(w.abs().max().double()))).float().flatten()
    assert torch.equal(e.flatten()[rest], want[rest].clamp(-top, top))


def test_window_neighbours():
    assert C.beyond(C.LO) < C.LO and C.beyond(C.HI) > C.HI
    assert C.beyond(C.LO) == float(np.float32(C.LO) * (1 - np.float32(2.0) ** -24))
    assert C.beyond(C.HI) == C.HI * (1 + 2.0 ** -23)


# ------------------------------------------------------------------ the plane model
def test_planes_at_the_lower_edge():
    sd = C.CASES_1D["1d-lo-in"][0]()
    names = C.gauge_1d(sd) + ["final_conv.1.weight"]
    assert len(names) == 34          # 16 blocks x 2 convolutions, final_conv.0, final_conv.1
    for k in names:
        assert float(sd[k].abs().max()) == C.LO, k
        hi, lo = C.split_planes(sd[k], False)
        assert float((hi.abs() < C.FP16_MIN_NORMAL).double().mean()) > 0.2 and float((lo.abs() < C.FP16_MIN_NORMAL).double().mean()) > 0.5, k
        assert C.plane_error(sd[k], False) <= 2.0 ** -24, k
        assert C.plane_error(sd[k], "lo") >= 1e-4, k
        assert C.plane_error(sd[k], True) >= 1e-4, k


def test_planes_at_the_upper_edge():
    sd = C.CASES_1D["1d-hi-in"][0]()
    for k in C.gauge_1d(sd) + ["final_conv.1.weight"]:
        assert float(sd[k].abs().max()) == C.HI and C.plane_error(sd[k], False) <= 2.0 ** -24, k
    out = C.CASES_1D["1d-hi-out"][0]()[C.DEEP_1D]
    assert float(out.abs().max()) == C.beyond(C.HI)


def test_folded_tiny_weights_are_outside_the_window():
    for base in (C.base_2d(), C.base_force()):
        unit = [C.ws_folded(v) for k, v in base.items() if k.endswith(".proj.weight")]
        tiny = [C.ws_folded(v) for k, v in C.ws_tiny(base).items() if k.endswith(".proj.weight")]
        assert len(unit) == len(tiny) >= 18
        for u, f in zip(unit, tiny):
            assert 1.0 < float(u.abs().max()) < 4.0 and C.plane_error(u, False) <= 2.0 ** -23       # O(1) at unit scale (what the old comment relied on): 2^-24 of the binade's upper end
            assert 2e-7 < float(f.abs().max()) < 2e-6 < C.LO
            assert C.plane_error(f, False) >= 1e-5


def test_ruled_lists():
    sd = C.base_1d()
    r = C.ruled_1d(sd)
    assert all(sd[k].dim() >= 2 and "time_mlp" not in k for k in r) and "final_conv.1.weight" in r and "downs.0.2.fn.fn.to_qkv.weight" in r
    assert set(C.gauge_1d(sd)) == {k for k in sd if k.endswith(".block.0.weight")} and set(C.SINGLE_1D + [C.DEEP_1D]) <= set(r)
    for base in (C.base_2d(), C.base_force()):
        r2 = C.ruled_2d(base)
        assert all(base[k].dim() == 4 and ".proj." not in k for k in r2) and "init_conv.weight" in r2
        assert {k for k, v in base.items() if v.dim() == 4} - set(r2) == {k for k in base if k.endswith(".proj.weight")}
    assert "downs.1.3.weight" in C.ruled_2d(C.base_2d()) and "final_conv.weight" in C.ruled_2d(C.base_2d())


# ------------------------------------------------------------------ yardsticks
def _taps(fwd32, fwd64, sd, x, t):
    tt = torch.full((x.shape[0],), t, dtype=torch.long)
    t32, t64 = {}, {}
    t32["eps"], t64["eps"] = fwd32(sd, x, tt, taps=t32), fwd64(sd, x, tt, taps=t64)
    return {k: v for k, v in t32.items() if k not in NOT_BLOCKS}, {k: v for k, v in t64.items() if k not in NOT_BLOCKS}


def _force_flat(run):
    out, dx, act, grad = run
    return {"out": out, "dx": dx, **act, **{"grad:" + k: v for k, v in grad.items()}}


def _yardsticks(case):
    """-> [(rows or images, fp32 taps, float64 taps)] of one case, one entry per size it runs at."""
    if case in C.CASES_1D:
        mk, rows, _, amp, *seed = C.CASES_1D[case]
        sd, res = mk(), []
        for B in rows:
            x = C.input_1d(B, amp, *seed)[C.rows_compared(B)]
            t32, t64 = _taps(O.unet1d_forward, R.unet1d_forward_f64, sd, x, C.T_1D)
            res.append((B, t32, t64))
    elif case in C.CASES_2D:
        mk, size, _ = C.CASES_2D[case]
        res = [(size,) + _taps(O.unet2d_forward, R.unet2d_forward_f64, mk(), C.input_2d(size), C.T_2D)]
    else:
        sd, x, res = C.CASES_FORCE[case][0](), C.input_force(), []
        runs = [[_force_flat(f(sd, x[i:i + 1], C.LAMBDA_FORCE)) for i in range(max(C.IMAGES_FORCE))]      # each image alone, as
                for f in (R.force_unet_blocks, R.force_unet_f64)]                                          # tests/test_gpu_f64_budget_force.py does
        for n in C.IMAGES_FORCE:
            res.append((n,) + tuple({k: torch.cat([r[k] for r in run[:n]]) for k in run[0]} for run in runs))
    return res


ALL_CASES = list(C.CASES_1D) + list(C.CASES_2D) + list(C.CASES_FORCE)


@pytest.mark.parametrize("case", ALL_CASES)
def test_yardsticks(case):
    res = _yardsticks(case)
    low = {}
    for size, t32, t64 in res:
        assert set(t32) == set(t64) and len(t64) == (31 if case in C.CASES_1D else 22 if case in C.CASES_2D else 42)
        for k, ref in t64.items():
            assert bool(torch.isfinite(ref).all()) and bool(torch.isfinite(t32[k]).all()), (case, size, k)
            e = R.e32(t32[k], ref)
            assert 0 < e < 2e-5, (case, size, k, e)
            if e < FLOOR:
                low[k] = min(low.get(k, 1.0), e)
    print(f"{case}: taps under {FLOOR:g}: " + (", ".join(f"{k} {v:.2e}" for k, v in low.items()) or "none"))
    if case in C.CASES_FORCE:
        pinned = set(C.BELOW_FLOOR_FORCE) | set(C.DEGENERATE.get(case, ()))
    else:
        pinned = set(C.BELOW_FLOOR.get(case, ()))
    if case in C.DEGENERATE:
        assert set(low) <= pinned and {"out", "grad:mid_attn"} <= set(low), (case, low)
    else:
        assert set(low) == pinned, (case, low)
    # the condition of range_cases.BELOW_FLOOR
    own = set(C.BELOW_FLOOR.get(case, ()))
    assert len(own) <= 3 and all(k == "init_conv" or k.startswith("downs.0.") for k in own), (case, own)
    if case in C.DEGENERATE:
        # ... and the one case outside it: the bottleneck no longer depends on the image
        g = res[-1][2]["grad:mid_attn"]
        assert float(R.row_err(g[1:], g[:1].expand_as(g[1:])).max()) < 1e-6, case
    if case in C.CASES_FORCE:
        out = res[-1][2]["out"]
        assert float((out[:, 0].abs() / out.abs().max()).min()) >= 1e-3, ("the sign of |out0| is in question at this seed", case)


def test_below_floor_names_cases_of_the_tables():
    assert set(C.BELOW_FLOOR) <= set(C.CASES_1D) | set(C.CASES_2D) and set(C.DEGENERATE) <= set(C.CASES_FORCE)


# ------------------------------------------------------------------ bite, on the host
@pytest.fixture(scope="module")
def lo_in_17():
    sd = C.CASES_1D["1d-lo-in"][0]()
    x = C.input_1d(17)
    return (sd, x) + _taps(O.unet1d_forward, R.unet1d_forward_f64, sd, x, C.T_1D)


@pytest.mark.parametrize("flush", ["lo", True], ids=["low-plane", "both-planes"])
@pytest.mark.parametrize("layer", ["downs.3.0.blocks.0", "mid_block1.blocks.0", "downs.0.0.blocks.1"])
def test_budget_sees_flushed_planes_at_the_lower_edge(monkeypatch, lo_in_17, layer, flush):
    """The mechanism of test_budget_sees_a_lost_fp16_plane: one convolution of the float64 forward reads the plane model of its
    weights, subnormals flushed."""
    sd, x, t32, t64 = lo_in_17
    orig, key = O.conv1d_block, layer + ".block.0.weight"
    assert float(sd[key].abs().max()) == C.LO

    def lossy(sdx, p, xx, n_groups=8):
        if p == layer:
            sdx = dict(sdx)
            sdx[key] = C.planes_value(sd[key], flush).to(xx.dtype)
        return orig(sdx, p, xx, n_groups)

    monkeypatch.setattr(O, "conv1d_block", lossy)
    _, bad = _taps(O.unet1d_forward, R.unet1d_forward_f64, sd, x, C.T_1D)
    monkeypatch.undo()
    block = layer.split(".blocks")[0]
    worst = float(R.row_err(bad[block], t64[block]).max())
    budget = R.M * max(R.e32(t32[block], t64[block]), 2.0 ** -23)
    whole = float((bad["eps"] - t64["eps"]).abs().max() / t64["eps"].abs().max())
    print(f"{layer} flush={flush}: row_err at {block} {worst:.3e} = {worst / budget:.1f} x M x e32; eps moves by {whole:.3e} (TOL_FWD {TOL_FWD:g})")
    assert worst >= 10 * budget, (layer, worst, budget)
    if flush == "lo":
        assert whole < TOL_FWD              # the old bound is blind to it ...
        assert float(R.row_err(bad["eps"], t64["eps"]).max()) > R.M * max(R.e32(t32["eps"], t64["eps"]), 2.0 ** -23)      # ... the new one is not
    # the planes with subnormals kept are inside the budget with room to spare
    monkeypatch.setattr(O, "conv1d_block", lambda sdx, p, xx, n_groups=8: orig({**sdx, key: C.planes_value(sd[key], False).to(xx.dtype)} if p == layer else sdx, p, xx, n_groups))
    _, kept = _taps(O.unet1d_forward, R.unet1d_forward_f64, sd, x, C.T_1D)
    monkeypatch.undo()
    assert float(R.row_err(kept[block], t64[block]).max()) < 0.1 * budget
