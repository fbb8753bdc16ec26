"""GPU (MI355X): nbody_simulate_kernel (cindm_nbody_simulate, cindm_amd.simulation) against the host statement of the rule in
tests/nbody_cases.py, which tests/test_nbody_sim_host.py proves first.

Tolerance per case: max(1e-9 px, 64 * (events + n_steps) * s_case), s_case = the statement's own largest deviation under a +-2^-52
relative perturbation of every input (four sign patterns).  The margin counts rounding sites -- each rounded operation perturbs one
state variable by at most one ulp, the input perturbation measures how such a perturbation grows over the longest horizon.  status and
events must match exactly.  The library is built without contraction and float64 division and square root are correctly rounded, so
the measured deviation is expected to be far inside the tolerance; the largest ratio deviation / s_case is printed."""
import functools

import numpy as np
import pytest
import torch

import cindm_amd
import nbody_cases as N
from test_gpu_parity import build_unet

pytestmark = pytest.mark.gpu

B_MAX = 67


@functools.lru_cache(maxsize=None)
def _reference(nb, n_steps):
    """The statement on the B_MAX generator cases of this body count, with each case's s_case: computed once, read-only."""
    feats = N.generator_cases(nb, B_MAX)
    out, status, events, _ = N.simulate(feats, n_steps)
    s = np.array([N.sensitivity(feats[i], n_steps, base=out[i]) for i in range(B_MAX)])
    for a in (out, status, events, s):
        a.setflags(write=False)
    return feats, out, status, events, s


def _tolerance(events, n_steps, s):
    return np.maximum(1e-9, 64.0 * (events.astype(np.float64) + n_steps) * s)


def _run(feats, n_steps, device, **kw):
    out, (status, events) = cindm_amd.simulation(torch.tensor(np.array(feats)).to(device), n_steps, return_status=True, **kw)
    torch.cuda.synchronize()
    assert out.dtype == torch.float64 and out.device.type == "cuda" and status.dtype == events.dtype == torch.int32
    return out.cpu().numpy(), status.cpu().numpy(), events.cpu().numpy()


def _hold(got, want, events, n_steps, s, what):
    dev = np.abs(got - want).reshape(got.shape[0], -1).max(1)
    tol = _tolerance(events, n_steps, s)
    ratio = float((dev / np.maximum(s, 1e-300)).max()) if (s > 0).all() else float("nan")
    print(f"[nbody] {what}: largest deviation {dev.max():.3e} px, largest deviation / s_case {ratio:.3g}, smallest tolerance {tol.min():.3e}")
    assert (dev <= tol).all(), (what, dev.max(), tol[dev.argmax()])


@pytest.mark.parametrize("n_steps", [1, 92])
@pytest.mark.parametrize("B", [1, 5, B_MAX])
@pytest.mark.parametrize("nb", [1, 2, 3, 4, 8])
def test_kernel_against_the_host_statement(device, nb, B, n_steps):
    feats, want, status, events, s = _reference(nb, n_steps)
    got, st, ev = _run(feats[:B], n_steps, device)
    assert got.shape == (B, n_steps, nb, 4)
    assert np.array_equal(st, status[:B]) and np.array_equal(ev, events[:B])
    assert np.array_equal(got[:, 0], feats[:B].astype(np.float64))                 # frame 0 is the input
    _hold(got, want[:B], events[:B], n_steps, s[:B], f"nb={nb} B={B} n_steps={n_steps}")


def _against_statement(feat, n_steps, device, **kw):
    hkw = {("max_events" if k == "max_events_per_frame" else k): v for k, v in kw.items()}
    want, status, events, _ = N.simulate(feat, n_steps, **hkw)
    got, st, ev = _run(feat, n_steps, device, **kw)
    assert np.array_equal(st, status) and np.array_equal(ev, events), (st, status, ev, events)
    finite = np.isfinite(feat).all((1, 2))
    assert np.isnan(got[~finite]).all() and np.isnan(want[~finite]).all()
    if finite.any():
        s = np.array([N.sensitivity(f, n_steps, **hkw) for f in feat[finite]])
        _hold(got[finite], want[finite], events[finite], n_steps, s, "case")
    return got, st, ev


def test_analytic_cases(device):
    for speed in (100.0, 20000.0):
        feat, closed = N.wall_case(speed)
        got, st, _ = _against_statement(feat, 92, device)
        want = np.stack([closed(i) for i in range(92)])
        assert st[0] == 0 and np.abs(got[0, :, 0, :2] - want[:, :2]).max() <= 1e-9 and np.array_equal(got[0, :, 0, 2:], want[:, 2:])
    feat, t_c = N.head_on_case()
    got, st, ev = _against_statement(feat, 60, device)
    k = int(t_c / N.DT) + 1
    assert st[0] == 0 and ev[0] == 1 and np.abs(got[0, k, :, 2] - [-40.0, 60.0]).max() <= 1e-12
    feat, t_c, v0, v1 = N.glancing_case()
    got, st, _ = _against_statement(feat, 70, device)
    k = int(t_c / N.DT) + 1
    assert st[0] == 0 and np.abs(got[0, k, 0, 2:] - v0).max() <= 1e-9 and np.abs(got[0, k, 1, 2:] - v1).max() <= 1e-9
    feat, t1, t2 = N.line_case()
    got, st, _ = _against_statement(feat, 40, device)
    k2 = int(t2 / N.DT) + 1
    assert st[0] == 0 and np.abs(got[0, k2, :, 2] - [0.0, 0.0, 90.0]).max() <= 1e-12


def test_defined_edge_behaviour(device):
    E = N.edge_cases()
    got, st, ev = _against_statement(E["overlap_approaching"], 2, device)
    assert st[0] == 1 and ev[0] == 1 and np.array_equal(got[0, 1, :, 2], [-30.0, 30.0])
    got, st, ev = _against_statement(E["overlap_separating"], 2, device)
    assert st[0] == 1 and ev[0] == 0 and np.array_equal(got[0, 1, :, 2], [-30.0, 30.0])
    got, st, ev = _against_statement(E["outside_outbound"], 2, device)
    assert st[0] == 1 and ev[0] == 1 and got[0, 1, 0, 2] == -50.0
    got, st, ev = _against_statement(E["fast"], 20, device, max_events_per_frame=1)
    assert st[0] & 2 and np.isfinite(got).all()
    # a NaN marks its own design only, wherever it sits in the workgroup's four designs
    feats = np.array(N.generator_cases(2, 6), dtype=np.float64)
    feats[1, 1, 2] = np.nan
    feats[4, 0, 0] = np.inf
    got, st, ev = _against_statement(feats, 5, device)
    assert list(st) == [0, 8, 0, 0, 8, 0] and ev[1] == ev[4] == 0
    assert np.isnan(got[[1, 4]]).all() and np.isfinite(got[[0, 2, 3, 5]]).all()
    # coincident centres: the pair event is skipped and flagged, the state stays finite
    got, st, ev = _against_statement(E["coincident"], 3, device)
    assert st[0] == 1 | 4 and ev[0] == 0 and np.isfinite(got).all()
    # another box, radius and frame length
    feat = np.array([[[30.0, 40.0, 70.0, -55.0], [90.0, 60.0, -35.0, 20.0], [60.0, 100.0, 10.0, 80.0]]])
    _against_statement(feat, 50, device, width=120, height=140, radius=9, wall_radius=0.5, dt=1 / 30)


def test_input_forms_agree(device):
    feats = N.generator_cases(4, 9)
    want, status, events, _ = N.simulate(feats, 30)
    f32 = torch.tensor(feats)
    wide = torch.zeros((9, 8, 8), dtype=torch.float32, device=device)
    wide[:, ::2, 1:5] = f32.to(device)
    forms = {"fp32 on the host": f32, "fp32": f32.to(device), "fp64": f32.to(device).double(), "strided": wide[:, ::2, 1:5]}
    assert not forms["strided"].is_contiguous()
    base = None
    for name, f in forms.items():
        out, (st, ev) = cindm_amd.simulation(f, 30, return_status=True)
        assert out.device.type == "cuda" and out.dtype == torch.float64
        base = out if base is None else base
        assert torch.equal(out, base), name
        assert np.array_equal(st.cpu().numpy(), status) and np.array_equal(ev.cpu().numpy(), events)
    assert torch.equal(cindm_amd.simulation(features=f32, n_steps=30), base)          # the reference's keyword call
    assert np.abs(base.cpu().numpy() - want).max() <= 1e-9


def test_a_call_on_a_side_stream_is_ordered_after_the_producer(device):
    feats = torch.tensor(N.generator_cases(8, 33)).to(device)
    want = cindm_amd.simulation(feats, 40)
    torch.cuda.synchronize()
    big = torch.randn((2048, 2048), device=device)
    side = torch.cuda.Stream(device)
    side.wait_stream(torch.cuda.current_stream(device))
    with torch.cuda.stream(side):
        slow = big
        for _ in range(8):
            slow = (slow @ big) * 1e-3                                              # the producer takes a while on the side stream
        made = feats + 0.0 * slow[:33, :8, None].clamp(-1.0, 1.0).nan_to_num()     # features exist only once it has finished
        got = cindm_amd.simulation(made, 40)
    side.synchronize()                                                              # the side stream alone
    assert torch.equal(got, want)


def _objective(x):
    return (x[:, -1, :2] - 0.5).square().sum(-1).sqrt().mean()


def _objective_std(x):
    return (x[:, -1, :2] - 0.5).square().sum(-1).sqrt().std()


def test_sample_resimulate_score_on_the_device(device):
    """Sample, re-simulate, score (inference/inverse_design_diffusion_1d.py:303-340) with nothing but device tensors, against the same
    calls fed with the host statement."""
    m, _ = build_unet(device)
    diff = cindm_amd.GaussianDiffusion1D(m, image_size=24, conditioned_steps=0).to(device)
    out = diff.sample(batch_size=5, n_composed=0, seed=5, t_stop=996)               # four DDPM steps, 2 bodies
    assert tuple(out.shape) == (5, 24, 8) and bool(torch.isfinite(out).all())
    seen = {}

    def host_simulation(features, n_steps):
        f = features.detach().cpu().numpy().astype(np.float64)
        o, st, ev, _ = N.simulate(f, n_steps)
        seen.update(events=ev, n_steps=n_steps, status=st,
                    s=np.array([N.sensitivity(f[i], n_steps, base=o[i]) for i in range(f.shape[0])]))
        return torch.tensor(o)

    pred_simu, obj = cindm_amd.eval_simu(out[:, :4], _objective, 2, 20, simulation=cindm_amd.simulation)
    ref_simu, ref_obj = cindm_amd.eval_simu(out[:, :4], _objective, 2, 20, simulation=host_simulation)
    assert pred_simu.device.type == "cuda" and pred_simu.dtype == torch.float64 and tuple(pred_simu.shape) == (5, 20, 8)
    tol = _tolerance(seen["events"], seen["n_steps"], seen["s"]) / 200.0
    dev = (pred_simu - ref_simu).abs().reshape(5, -1).max(1).values.cpu().numpy()
    print(f"[nbody] end to end: deviation {dev.max():.3e}, tolerance {tol.min():.3e}, status {seen['status']}, events {seen['events']}")
    assert (dev <= tol).all() and abs(float(obj) - float(ref_obj)) <= tol.max()
    rep = cindm_amd.design_report(out, _objective, 2, 3, 21, eval_fn_std=_objective_std)
    ref = cindm_amd.design_report(out, _objective, 2, 3, 21, eval_fn_std=_objective_std, simulation=host_simulation)
    tol = float((_tolerance(seen["events"], seen["n_steps"], seen["s"]) / 200.0).max())
    assert rep["pred_simu"].device.type == "cuda" and rep["RMSE"].device.type == "cuda"
    assert float((rep["pred_simu"] - ref["pred_simu"]).abs().max()) <= tol
    for k in ("design_obj_simu", "design_obj_simu_CI", "RMSE", "RMSE_CI", "MAE", "MAE_CI"):
        assert abs(float(rep[k]) - float(ref[k])) <= tol, k
    assert rep["n_flagged"] == int((seen["status"] != 0).sum()) and ref["n_flagged"] is None
