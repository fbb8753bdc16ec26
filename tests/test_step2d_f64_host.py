"""CPU: the float64 statement of the 2-D reverse step in oracle/f64_reference.py (``step2d_predict_f64``, ``step2d_update_f64``) is
proven before it judges a kernel.

Over the whole grid of tests/step2d_cases.py -- the one tests/test_gpu_step2d_f64.py runs the library on -- the fp32 oracle
(``cindm_oracle.model_predictions_2d``, ``p_sample_2d``, and for DDIM the combine of ``ddim_coefs`` the older DDIM tests use) lies
within (n_e + 4) * 2^-24 * A_e of the statement element by element, on a model output both sides share: a pixel-wise toy model
(``step2d_cases.toy_model``; evaluated in float64 and rounded) stands in for the U-Net.  The reference project's own execution of
``model_predictions``, ``p_mean_variance`` and ``p_sample`` on that toy (tests/golden/step2d_grid.npz, oracle/make_golden_step2d.py:
1440 records, every option combination at every (B, nb)) is held to the same bound, and nine mutations of the statement each leave it
by more than 100 x on the cases they touch.

The reference's 2-D ``ddim_sample`` cannot run: the DDIM form is the project's own definition (the docstring of
``cindm_amd.GaussianDiffusion.ddim_sample``), and what stands in for a reference is the oracle's model_predictions_2d followed by the
three-term combine in fp32."""
import os

import numpy as np
import pytest
import torch

import cindm_oracle as O
import f64_reference as R
import step2d_cases as S

C, H = S.CHANNELS, S.HOST_SIZE
TAB = {obj: O.make_schedule(S.BETA_SCHEDULE, 1000, obj) for obj in S.OBJECTIVES}


def _od(obj, share=True, avg=True, size=H):
    d = O.Diffusion2D({"final_conv.weight": torch.zeros(C, 1)}, image_size=size, frames=(C - 3) // 3, beta_schedule=S.BETA_SCHEDULE,
                      objective=obj, share_noise=share, use_average_share=avg)
    d.model = S.toy_model
    return d


def _E(x, t):
    return S.toy_model(x, torch.full((x.shape[0],), t, dtype=torch.long))


def _ratio(got, ref, n, A):
    assert got.shape == ref.shape, (got.shape, ref.shape)
    err = (got.double() - ref).abs()
    return float(torch.where(err == 0, torch.zeros_like(err), err / R.step2d_bound(n, A)).max())


def _noise(B, nb, t, size=H):
    zs, zb = S.make_noise(C, B, nb, t, size)
    return O.sample_noise_2d(zs, zb).reshape(B * nb, C, size, size)


def _step_ratios(got, obj, B, nb, x, t, share, avg, clip, z, mut=None):
    """{output: largest err / bound} of a p_mean_variance / p_sample result {"mean", "x_start", "state"} against the statement."""
    shape = (B, nb, C) + tuple(x.shape[2:])
    mean, x0, _, A = R.step2d_predict_f64(TAB[obj], shape, x, t, _E(x, t), objective=obj, share_noise=share, use_average_share=avg,
                                          clip=clip, _mut=mut)
    n = R.step2d_roundings(nb, obj, share_noise=share, clip=clip)
    st, As, ns = R.step2d_update_f64("ddpm", mean, A["mean"], n["mean"], z=z, t=t, logvar=TAB[obj]["posterior_log_variance_clipped"][t])
    ref = {"mean": (mean, n["mean"], A["mean"]), "x_start": (x0, n["x_start"], A["x_start"]), "state": (st, ns, As)}
    return {k: _ratio(v, *ref[k]) for k, v in got.items()}


def _predict_ratios(got, obj, B, nb, x, t, share, avg, clip, red, mut=None):
    shape = (B, nb, C) + tuple(x.shape[2:])
    _, x0, eps, A = R.step2d_predict_f64(TAB[obj], shape, x, t, _E(x, t), objective=obj, share_noise=share, use_average_share=avg,
                                         clip=clip, rederive=red, entry="model_predictions", _mut=mut)
    n = R.step2d_roundings(nb, obj, share_noise=share, clip=clip, rederive=red, entry="model_predictions")
    ref = {"x_start": (x0, n["x_start"], A["x_start"]), "pred_noise": (eps, n["pred_noise"], A["pred_noise"])}
    return {k: _ratio(v, *ref[k]) for k, v in got.items()}, x0


def _oracle_step(obj, B, nb, x, t, share, avg, clip, z):
    od = _od(obj, share, avg, x.shape[-1])
    shape = (B, nb, C) + tuple(x.shape[2:])
    state, x0 = O.p_sample_2d(od, shape, x.clone(), t, None if t == 0 else z, clip_denoised=clip)
    mean, _ = O.p_sample_2d(od, shape, x.clone(), t, None if t == 0 else torch.zeros_like(x), clip_denoised=clip)       # mean + sigma * 0
    return {"mean": mean, "x_start": x0, "state": state}


def _oracle_predict(obj, B, nb, x, t, share, avg, clip, red):
    shape = (B, nb, C) + tuple(x.shape[2:])
    eps, x0 = O.model_predictions_2d(_od(obj, share, avg, x.shape[-1]), shape, x.clone(), t, clip_x_start=clip, rederive_pred_noise=red,
                                     share_noise=share)
    return {"pred_noise": eps, "x_start": x0}


def _ddim_point(obj, B, nb, avg, eta, i, shared, guided=False, mut=None):
    """One DDIM pair: the oracle's fp32 (model_predictions_2d, ddim_coefs, the combine[, the shift]) against the statement."""
    od = _od(obj, True, avg)
    t, tn = O.ddim_time_pairs(1000, S.DDIM_S)[i]
    shape = (B, nb, C, H, H)
    x = S.make_state(C, B, nb, t, shared, H)
    z = _noise(B, nb, i)
    eps, x0 = O.model_predictions_2d(od, shape, x.clone(), t, clip_x_start=True, rederive_pred_noise=True)
    row = torch.stack([torch.as_tensor(v, dtype=torch.float32) for v in O.ddim_coefs(od, t, tn, eta)])
    got = x0 if tn < 0 else x0 * row[0] + row[1] * eps + row[2] * z
    _, r0, re, A = R.step2d_predict_f64(TAB[obj], shape, x, t, _E(x, t), objective=obj, share_noise=True, use_average_share=avg, clip=True,
                                        rederive=True, entry="model_predictions", _mut=mut)
    n = R.step2d_roundings(nb, obj, share_noise=True, clip=True, rederive=True, entry="model_predictions")
    st, As, ns = R.step2d_update_f64("ddim", r0, A["x_start"], n["x_start"], z=z, eps=re, A_eps=A["pred_noise"], n_eps=n["pred_noise"],
                                     row=row, last=tn < 0)
    if guided:
        g = torch.randn(x.shape, generator=torch.Generator().manual_seed(i + 3)) * 0.2
        w = (od.coeff_ratio * od.tab["betas"].flip(0)).double()[tn + 1:t + 1].sum().float()
        got = got - w * g
        st, As, ns = R.step2d_update_f64("guided", st, As, ns, w=w, g=g)
    return _ratio(got, st, ns, As)


# ------------------------------------------------------------------ the grid, the fp32 oracle
@pytest.mark.parametrize("obj", S.OBJECTIVES)
def test_step_oracle_within_bound(obj):
    """p_mean_variance / p_sample: share_noise x mean / sum x clip x t x (B, nb), half of the cases on a state the copies share.  At
    t = 500 with clip on the clamp acts on part of x_start under every objective (else the clamp-order mutations were invisible)."""
    n = 0
    for (share, avg, clip, t) in S.STEP_OPTIONS:
        for B, nb in S.BNB:
            shared = S.state_is_shared(share, avg, clip)
            x, z = S.make_state(C, B, nb, t, shared, H), _noise(B, nb, t)
            r = _step_ratios(_oracle_step(obj, B, nb, x, t, share, avg, clip, z), obj, B, nb, x, t, share, avg, clip, z)
            assert max(r.values()) <= 1.0, (obj, share, avg, clip, t, B, nb, r)
            n += 1
    assert n == 32 * 5


@pytest.mark.parametrize("obj", S.OBJECTIVES)
def test_predict_oracle_within_bound(obj):
    n = 0
    for (share, avg, clip, red, t) in S.PREDICT_OPTIONS:
        for B, nb in S.BNB:
            x = S.make_state(C, B, nb, t, S.state_is_shared(share, avg, clip, red), H)
            r, x0 = _predict_ratios(_oracle_predict(obj, B, nb, x, t, share, avg, clip, red), obj, B, nb, x, t, share, avg, clip, red)
            assert max(r.values()) <= 1.0, (obj, share, avg, clip, red, t, B, nb, r)
            if clip:
                frac = float((x0.abs() == 1.0).double().mean())
                if t == 500:
                    assert 0.1 < frac < 0.9, (obj, share, avg, B, nb, frac)
                if t == 999 and obj != "pred_noise":        # (pred_noise at t = 999: sqrt_recip is 1.8e3 and everything may be clamped)
                    assert 0.0 < frac < 1.0, (obj, frac)
            n += 1
    assert n == 64 * 5


@pytest.mark.parametrize("obj", S.OBJECTIVES)
def test_ddim_oracle_within_bound(obj):
    """The DDIM pairs (the last with time_next = -1), eta 0 and 0.5, mean / sum, every (B, nb); and the guided shift on the guided
    kernel's pairs."""
    n = 0
    for (avg, eta, i) in S.DDIM_OPTIONS:
        for B, nb in S.BNB:
            r = _ddim_point(obj, B, nb, avg, eta, i, S.state_is_shared(avg, eta > 0, i))
            assert r <= 1.0, (obj, avg, eta, i, B, nb, r)
            n += 1
    for i in S.GUIDED_PAIRS:
        for B, nb in S.GUIDED_BNB:
            r = _ddim_point(obj, B, nb, True, S.GUIDED_ETA, i, False, guided=True)
            assert r <= 1.0, (obj, "guided", i, B, nb, r)
            n += 1
    assert n == 16 * 5 + 6


def test_zero_noise_and_t0_are_the_mean():
    """What ``_oracle_step`` relies on: p_sample_2d with a zero draw, and at t = 0, hands back the posterior mean."""
    od = _od("pred_noise", False, True)
    x = S.make_state(C, 2, 3, 0, False, H)
    a, _ = O.p_sample_2d(od, (2, 3, C, H, H), x.clone(), 0, None)
    m, _, _, _ = R.step2d_predict_f64(TAB["pred_noise"], (2, 3, C, H, H), x, 0, _E(x, 0), objective="pred_noise", share_noise=False,
                                      use_average_share=True, clip=True)
    st, A, n = R.step2d_update_f64("ddpm", m, m.abs(), 5, t=0)
    assert torch.equal(st, m) and n == 5 and float((a.double() - m).abs().max()) < 1e-5


# ------------------------------------------------------------------ the reference's own execution
def test_golden_within_bound(gold_dir):
    g = np.load(os.path.join(gold_dir, "step2d_grid.npz"))
    arr = {k: torch.from_numpy(g[k]) for k in g.files}
    assert sorted(arr) == ["predict.pred_noise", "predict.x_start", "step.mean", "step.state", "step.x_start"]
    off = {"step": 0, "predict": 0}
    size = S.GOLDEN_SIZE
    recs = S.golden_records()
    assert len(recs) == 3 * (32 + 64) * 5
    for name, entry, obj, share, avg, clip, red, t, B, nb in recs:
        x = S.make_state(C, B, nb, t, False, size)
        numel = x.numel()
        kind = "step" if entry == "p_mean_variance" else "predict"
        take = lambda k: arr[f"{kind}.{k}"][off[kind]:off[kind] + numel].reshape(x.shape)
        if kind == "step":
            got = {"mean": take("mean"), "x_start": take("x_start"), "state": take("state")}
            r = _step_ratios(got, obj, B, nb, x, t, share, avg, clip, None if t == 0 else _noise(B, nb, t, size))
        else:
            r, _ = _predict_ratios({"pred_noise": take("pred_noise"), "x_start": take("x_start")}, obj, B, nb, x, t, share, avg, clip, red)
        off[kind] += numel
        assert max(r.values()) <= 1.0, (name, r)
    assert off["step"] == arr["step.mean"].numel() == arr["step.state"].numel() and off["predict"] == arr["predict.x_start"].numel()


# ------------------------------------------------------------------ the bound means something
# mutation: (entry, objective, share_noise, avg, clip, rederive, t, (B, nb)) points of the grid on which it must show, all on states
# the copies do NOT share; and, measured here, the smallest factor by which the fp32 oracle leaves the mutated statement's bound
MUTATIONS = {
    "all_images": [("step", "pred_noise", True, True, True, False, 500, (2, 3)), ("step", "pred_v", False, False, True, False, 500, (3, 2))],
    "mean_sum": [("step", "pred_noise", True, True, True, False, 500, (1, 2)), ("step", "pred_x0", False, False, False, False, 1, (2, 3)),
                 ("ddim", "pred_noise", True, False, True, True, 25, (1, 5))],
    "seam": [("step", "pred_noise", True, True, True, False, 500, (1, 2)), ("predict", "pred_noise", True, False, False, False, 999, (2, 3)),
             ("ddim", "pred_noise", True, True, True, True, 1, (3, 2))],
    "clamp_after": [("step", "pred_noise", False, True, True, False, 500, (1, 2)), ("step", "pred_x0", False, False, True, False, 500, (2, 3))],
    "mean_unshared": [("step", "pred_noise", False, True, True, False, 500, (1, 2)), ("step", "pred_v", False, False, False, False, 1, (1, 5))],
    "x_copy0": [("step", "pred_noise", False, True, True, False, 500, (1, 2)), ("step", "pred_noise", True, True, False, False, 0, (2, 3)),
                ("predict", "pred_v", True, True, True, False, 500, (3, 2)), ("ddim", "pred_x0", True, True, True, True, 25, (1, 2))],
    "rederive_unclamped": [("predict", "pred_noise", True, True, True, True, 500, (1, 2)), ("predict", "pred_x0", True, True, True, False, 500, (2, 3)),
                           ("ddim", "pred_v", True, True, True, True, 25, (1, 2))],
    "raw_eps": [("ddim", "pred_noise", True, True, True, True, 25, (1, 2)), ("predict", "pred_noise", True, False, True, True, 500, (2, 3))],
    "share_x0v": [("predict", "pred_x0", True, True, False, False, 500, (1, 2)), ("step", "pred_v", True, False, True, False, 500, (2, 3)),
                  ("ddim", "pred_x0", True, True, True, True, 0, (1, 5))],
}
FLOOR = 100.0


def _mut_point(kind, obj, share, avg, clip, red, t, bnb, mut):
    B, nb = bnb
    if kind == "ddim":
        return _ddim_point(obj, B, nb, avg, 0.5, t, False, mut=mut)
    x = S.make_state(C, B, nb, t, False, H)
    if kind == "step":
        z = _noise(B, nb, t)
        return max(_step_ratios(_oracle_step(obj, B, nb, x, t, share, avg, clip, z), obj, B, nb, x, t, share, avg, clip, z, mut).values())
    return max(_predict_ratios(_oracle_predict(obj, B, nb, x, t, share, avg, clip, red), obj, B, nb, x, t, share, avg, clip, red, mut)[0].values())


@pytest.mark.parametrize("mut", list(MUTATIONS))
def test_mutation_leaves_the_bound(mut):
    """(a) ``all_images`` the share taken over all B * nb images; (b) ``mean_sum`` mean where sum is asked and the reverse; (c) ``seam``
    the boundary channels shared too; (d) ``clamp_after`` share_noise False: the clamp after the share of x_start; (e)
    ``mean_unshared`` share_noise False: the posterior mean not shared again; (f) ``x_copy0`` every copy reads the x of copy 0; (g)
    ``rederive_unclamped`` the re-derived noise taken from the unclamped x_start; (h) ``raw_eps`` the raw shared output where the
    re-derived noise belongs; (i) ``share_x0v`` pred_x0 / pred_v: the output shared inside model_predictions.  Each puts the fp32
    oracle outside the mutated statement's bound on every point listed for it, by FLOOR = 100 x at least (what the 1-D mutations
    cleared); the factors reached are in MUTATION_FACTORS."""
    for kind, obj, share, avg, clip, red, t, bnb in MUTATIONS[mut]:
        if kind != "ddim":
            assert t in S.STEP_T and bnb in S.BNB
        good = _mut_point(kind, obj, share, avg, clip, red, t, bnb, None)
        bad = _mut_point(kind, obj, share, avg, clip, red, t, bnb, (mut,))
        print(f"{mut} {kind} {obj} share={share} avg={avg} clip={clip} red={red} t={t} {bnb}: good {good:.3f}, mutated {bad:.3e}")
        assert good <= 1.0 and bad > FLOOR, (mut, kind, obj, good, bad)


# For the record (asserted is FLOOR): the smallest err / bound each mutation reaches over its points, rounded down; the un-mutated
# statement stays at 0.34 or below on the same points.
MUTATION_FACTORS = {"all_images": 1.4e6, "mean_sum": 4.8e4, "seam": 4.0e5, "clamp_after": 1.8e6, "mean_unshared": 4.1e6, "x_copy0": 1.2e7,
                    "rederive_unclamped": 2.6e5, "raw_eps": 1.6e6, "share_x0v": 1.5e6}


def test_roundings_formula():
    """n_e at the ends of the grid, by hand."""
    n = R.step2d_roundings(2, "pred_noise", share_noise=True, clip=True)
    assert (n["pred_noise"], n["x_start"], n["mean"]) == (2, 5, 8)
    n = R.step2d_roundings(5, "pred_noise", share_noise=False, clip=True)
    assert (n["pred_noise"], n["x_start_pre"], n["x_start"], n["mean"]) == (0, 3, 8, 16)
    n = R.step2d_roundings(3, "pred_x0", share_noise=True, clip=False)
    assert (n["pred_noise"], n["x_start"], n["mean"]) == (3, 0, 3)
    n = R.step2d_roundings(3, "pred_v", share_noise=False, clip=True)
    assert (n["pred_noise"], n["x_start"], n["mean"]) == (6, 6, 12)
    n = R.step2d_roundings(3, "pred_noise", share_noise=True, clip=True, rederive=True, entry="model_predictions")
    assert (n["pred_noise"], n["x_start"], n["mean"]) == (9, 6, None)
    n = R.step2d_roundings(3, "pred_noise", share_noise=True, clip=False, rederive=True, entry="model_predictions")
    assert n["pred_noise"] == 3
    one = torch.ones(1, dtype=torch.float64)
    assert R.step2d_update_f64("ddpm", one, one, 8, z=one, t=5, logvar=torch.tensor(0.0))[2] == 12
    assert R.step2d_update_f64("ddim", one, one, 6, z=one, eps=one, A_eps=one, n_eps=9, row=torch.tensor([1.0, 1.0, 0.0]))[2] == 14
    assert R.step2d_update_f64("ddim", one, one, 6, last=True)[2] == 6
    assert R.step2d_update_f64("guided", one, one, 14, w=0.5, g=one)[2] == 16
    assert R.BOUND_SLACK == 4 and R.U24 == 2.0 ** -24
