"""CPU: the host statement of the n-body re-simulation rule (tests/nbody_cases.py) against closed forms and invariants, the
float64 restatement of the reference script's report, and the refusals of cindm_amd.simulation / design_report, which need no device.
The kernel is held to the same statement in tests/test_gpu_nbody_sim.py."""
import math

import numpy as np
import pytest
import torch

import cindm_amd
import nbody_cases as N


@pytest.mark.parametrize("speed", [100.0, 20000.0])
def test_wall_bounce_is_the_triangle_wave(speed):
    feat, closed = N.wall_case(speed)
    out, status, events, _ = N.simulate(feat, 92)
    assert status[0] == 0
    want = np.stack([closed(i) for i in range(92)])
    assert np.abs(out[0, :, 0, :2] - want[:, :2]).max() <= 1e-9
    assert np.array_equal(out[0, :, 0, 2:], want[:, 2:])               # reflections only change signs
    per_frame = events[0] / 91.0
    if speed == 20000.0:
        assert 2.0 <= per_frame <= 3.0, per_frame
    else:
        assert events[0] >= 1


def test_head_on_pair_swaps_velocities_at_the_contact_time():
    feat, t_c = N.head_on_case()
    out, status, events, _ = N.simulate(feat, 60)
    assert status[0] == 0 and events[0] == 1
    k = int(math.floor(t_c / N.DT)) + 1                                # the first frame after the contact
    assert np.array_equal(out[0, k - 1, :, 2], [60.0, -40.0])
    assert np.abs(out[0, k, :, 2] - [-40.0, 60.0]).max() <= 1e-12 and np.abs(out[0, k, :, 3]).max() == 0.0
    t = k * N.DT
    want_x = [50.0 + 60.0 * t_c - 40.0 * (t - t_c), 151.0 - 40.0 * t_c + 60.0 * (t - t_c)]
    assert np.abs(out[0, k, :, 0] - want_x).max() <= 1e-9


def test_glancing_pair_exchanges_the_normal_component():
    feat, t_c, v0, v1 = N.glancing_case()
    out, status, events, _ = N.simulate(feat, 70)
    assert status[0] == 0 and events[0] >= 1
    k = int(math.floor(t_c / N.DT)) + 1
    assert np.abs(out[0, k, 0, 2:] - v0).max() <= 1e-9 and np.abs(out[0, k, 1, 2:] - v1).max() <= 1e-9
    p0 = np.array([40.0 + 80.0 * t_c, 100.0]) + v0 * (k * N.DT - t_c)
    assert np.abs(out[0, k, 0, :2] - p0).max() <= 1e-9


def test_three_in_a_line_hand_the_momentum_through():
    feat, t1, t2 = N.line_case()
    out, status, events, _ = N.simulate(feat, 40)
    assert status[0] == 0
    k1, k2 = int(math.floor(t1 / N.DT)) + 1, int(math.floor(t2 / N.DT)) + 1
    assert k1 < k2
    assert np.abs(out[0, k1, :, 2] - [0.0, 90.0, 0.0]).max() <= 1e-12
    assert np.abs(out[0, k2, :, 2] - [0.0, 0.0, 90.0]).max() <= 1e-12
    assert np.abs(out[0, k2, :, 0] - [30.0 + 90.0 * t1, 86.0 + 90.0 * (t2 - t1), 144.0 + 90.0 * (k2 * N.DT - t2)]).max() <= 1e-9


@pytest.mark.parametrize("nb", [2, 4, 8])
def test_generator_cases_keep_the_invariants(nb):
    feats = N.generator_cases(nb, 40)
    assert feats.dtype == np.float32 and not feats.flags.writeable
    out, status, events, gap = N.simulate(feats, 92)
    assert (status == 0).all()
    ke = 0.5 * (out[..., 2:] ** 2).sum((2, 3))
    drift = np.abs(ke / ke[:, :1] - 1.0).max()
    d = np.sqrt(((out[:, :, :, None, :2] - out[:, :, None, :, :2]) ** 2).sum(-1)) + np.eye(nb) * 1e9
    print(f"nb={nb}: energy drift {drift:.2e}, smallest gap {gap.min():.2e} s, most events {events.max()}, closest pair {d.min():.6f}")
    assert drift <= 1e-12
    assert d.min() >= 2 * N.RADIUS - 1e-6
    assert out[..., :2].min() >= N.LO - 1e-9 and out[..., :2].max() <= N.HI + 1e-9
    assert gap.min() >= 1e-7                                           # the order of events does not hang on a rounding
    assert events.max() >= 1


def test_defined_edge_behaviour():
    E = N.edge_cases()
    out, status, events, _ = N.simulate(E["overlap_approaching"], 2)
    assert status[0] == 1 and events[0] == 1
    assert np.array_equal(out[0, 1, :, 2], [-30.0, 30.0])              # collided at t = 0
    assert np.abs(out[0, 1, :, 0] - [80.0 - 30.0 * N.DT, 110.0 + 30.0 * N.DT]).max() <= 1e-12
    out, status, events, _ = N.simulate(E["overlap_separating"], 2)
    assert status[0] == 1 and events[0] == 0                           # passes freely
    assert np.array_equal(out[0, 1, :, 2], [-30.0, 30.0])
    out, status, events, _ = N.simulate(E["outside_outbound"], 2)
    assert status[0] == 1 and events[0] == 1
    assert out[0, 1, 0, 2] == -50.0 and abs(out[0, 1, 0, 0] - (185.0 - 50.0 * N.DT)) <= 1e-12
    out, status, events, _ = N.simulate(E["fast"], 20, max_events=1)
    assert status[0] & 2 and np.isfinite(out).all() and events[0] <= 19
    out, status, events, _ = N.simulate(E["coincident"], 3)
    assert status[0] == 1 | 4 and events[0] == 0 and np.isfinite(out).all()
    bad = np.concatenate([E["overlap_separating"], E["overlap_separating"]]).copy()
    bad[0, 1, 2] = np.nan
    out, status, events, _ = N.simulate(bad, 3)
    assert status[0] == 8 and events[0] == 0 and np.isnan(out[0]).all()
    assert status[1] == 1 and np.isfinite(out[1]).all()


def test_sensitivity_is_small_and_positive():
    feats = N.generator_cases(8, 40)
    s = N.sensitivity(feats[0], 92)
    assert 0.0 < s < 1e-8, s


# ---- design_report against a float64 restatement of inference/inverse_design_diffusion_1d.py:316-340 ------------------------------
def _ballistic(features, n_steps):
    """A stand-in simulator: straight lines, float64 [B, n_steps, nb, 4] like the reference's."""
    f = features.detach().cpu().to(torch.float64)
    t = torch.arange(n_steps, dtype=torch.float64).reshape(1, -1, 1, 1) / 60.0
    pos = f[:, None, :, :2] + f[:, None, :, 2:] * t
    return torch.cat([pos, f[:, None, :, 2:].expand(-1, n_steps, -1, -1)], -1)


def _eval_fn(x):
    return (x[:, -1, :2] - 0.5).square().sum(-1).sqrt().mean()


def _eval_fn_std(x):
    return (x[:, -1, :2] - 0.5).square().sum(-1).sqrt().std()


@pytest.mark.parametrize("start_eval_t", [0, 2])
def test_design_report_restates_the_script(start_eval_t):
    g = torch.Generator().manual_seed(3)
    B, nb, output_steps = 6, 2, 5
    pred = torch.rand((B, start_eval_t + output_steps, nb * 4), generator=g)
    rep = cindm_amd.design_report(pred, _eval_fn, nb, start_eval_t, output_steps, eval_fn_std=_eval_fn_std, simulation=_ballistic)
    # the script, in float64 numpy
    p = pred.numpy().astype(np.float64)
    cond = (pred[:, start_eval_t].numpy() * np.float32(200.0)).astype(np.float64).reshape(B, nb, 4)      # eval_simu scales in pred's dtype
    n_steps = (output_steps - 1) * 4
    t = np.arange(n_steps).reshape(1, -1, 1, 1) / 60.0
    sim = np.concatenate([cond[:, None, :, :2] + cond[:, None, :, 2:] * t, np.broadcast_to(cond[:, None, :, 2:], (B, n_steps, nb, 2))], -1)
    simu = sim.reshape(B, n_steps, -1)[:, 3::4] / 200.0
    dist = np.sqrt(((simu[:, -1, :2] - 0.5) ** 2).sum(-1))
    full = np.concatenate([p[:, :start_eval_t + 1], simu], 1)
    diff = full - p
    rms = np.sqrt((diff ** 2).mean((1, 2)))
    mae = np.abs(diff).mean((1, 2))
    want = {"design_obj_simu": dist.mean(), "design_obj_simu_CI": dist.std(ddof=1) * 1.96 / np.sqrt(B), "RMSE": rms.mean(),
            "RMSE_CI": rms.std(ddof=1) * 1.96 / np.sqrt(B), "MAE": np.abs(diff).mean(), "MAE_CI": mae.std(ddof=1) * 1.96 / np.sqrt(B)}
    assert rep["pred_simu"].dtype == torch.float64 and tuple(rep["pred_simu"].shape) == (B, output_steps - 1, nb * 4)
    assert np.abs(rep["pred_simu"].numpy() - simu).max() <= 1e-14
    for k, v in want.items():
        assert abs(float(rep[k]) - v) <= 1e-13 * max(1.0, abs(v)), (k, float(rep[k]), v)
    assert rep["n_flagged"] is None                                     # a foreign simulator reports no status
    assert set(rep) == set(want) | {"pred_simu", "n_flagged"}
    assert "design_obj_simu_CI" not in cindm_amd.design_report(pred, _eval_fn, nb, start_eval_t, output_steps, simulation=_ballistic)


def test_design_report_refuses_a_wrong_shape():
    pred = torch.zeros((3, 6, 8))
    with pytest.raises(ValueError):
        cindm_amd.design_report(pred, _eval_fn, 3, 0, 6, simulation=_ballistic)
    with pytest.raises(ValueError):
        cindm_amd.design_report(pred, _eval_fn, 2, 1, 6, simulation=_ballistic)


# ---- refusals of cindm_amd.simulation: all before any device work ----------------------------------------------------------------
def test_simulation_is_public_and_keeps_the_reference_signature():
    import inspect
    assert "simulation" in cindm_amd.__all__ and "design_report" in cindm_amd.__all__
    names = list(inspect.signature(cindm_amd.simulation).parameters)
    assert names[:7] == ["features", "n_steps", "filename", "width", "height", "radius", "mass"]       # utils.py:1071
    sig = inspect.signature(cindm_amd.simulation).parameters
    assert [sig[n].default for n in names[2:7]] == [None, 200, 200, 20, 1]
    assert all(sig[n].kind is inspect.Parameter.KEYWORD_ONLY for n in names[7:])
    assert sig["wall_radius"].default == 1.0 and sig["dt"].default == 1 / 60 and sig["max_events_per_frame"].default == 64


def test_simulation_refusals(monkeypatch):
    ok = torch.tensor(N.generator_cases(2, 3))
    with pytest.raises(NotImplementedError):
        cindm_amd.simulation(ok, 4, filename="out")
    for bad in (ok[0], ok[:, :, :3], torch.zeros((2, 9, 4)), torch.zeros((0, 2, 4)), torch.zeros((2, 2, 4), dtype=torch.int64)):
        with pytest.raises(ValueError):
            cindm_amd.simulation(bad, 4)
    for kw in (dict(width=40), dict(height=42.0), dict(width=-200), dict(radius=0), dict(radius=-1), dict(mass=0), dict(mass=-2.0),
               dict(mass=float("nan")), dict(mass=[1.0, 2.0]), dict(dt=0), dict(dt=float("inf")), dict(wall_radius=-1.0),
               dict(max_events_per_frame=0), dict(max_events_per_frame=4097), dict(max_events_per_frame=1.5)):
        with pytest.raises(ValueError):
            cindm_amd.simulation(ok, 4, **kw)
    for n in (0, -1, 65536, 2.5):
        with pytest.raises(ValueError):
            cindm_amd.simulation(ok, n)
    # no ROCm device: the usual error, after the argument checks
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(ValueError):
        cindm_amd.simulation(ok, 0)
    with pytest.raises(cindm_amd.CindmError, match="no CPU execution path"):
        cindm_amd.simulation(ok, 4)
    with pytest.raises(cindm_amd.CindmError, match="no CPU execution path"):
        cindm_amd.eval_simu(torch.zeros((2, 1, 8)), _eval_fn, 2, 3, simulation=cindm_amd.simulation)


def test_c_entry_refuses_bad_arguments_before_any_launch():
    import ctypes as C
    from cindm_amd import _ffi
    L = _ffi.lib()
    assert C.sizeof(_ffi.NBodyDesc) == 48
    buf = (C.c_double * 64)()
    ist = (C.c_int32 * 4)()
    p, s = C.cast(buf, C.c_void_p), C.cast(ist, C.c_void_p)

    def call(desc=None, B=1, nb=2, n_steps=1, feats=p, out=p, status=s, events=s):
        d = _ffi.NBodyDesc(200.0, 200.0, 20.0, 1.0, 1 / 60, 64) if desc is None else _ffi.NBodyDesc(*desc)
        return L.cindm_nbody_simulate(C.byref(d), feats, B, nb, n_steps, out, status, events, None)

    for kw in (dict(feats=None), dict(out=None), dict(status=None), dict(events=None), dict(nb=0), dict(nb=9), dict(n_steps=0),
               dict(n_steps=65536), dict(B=0), dict(B=(1 << 22) + 1), dict(desc=(42.0, 200.0, 20.0, 1.0, 1 / 60, 64)),
               dict(desc=(200.0, 42.0, 20.0, 1.0, 1 / 60, 64)), dict(desc=(200.0, 200.0, 20.0, 1.0, 0.0, 64)),
               dict(desc=(200.0, 200.0, 20.0, 1.0, 1 / 60, 0)), dict(desc=(200.0, 200.0, 20.0, 1.0, 1 / 60, 4097)),
               dict(desc=(200.0, 200.0, float("nan"), 1.0, 1 / 60, 64))):
        assert call(**kw) != 0, kw
        assert b"cindm_nbody_simulate" in L.cindm_last_error()
