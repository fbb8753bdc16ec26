"""CPU: the float64 composition of oracle/f64_reference.py (``compose_predict_f64``) is proven before it judges a kernel.

Over the whole grid of tests/compose_cases.py -- the one tests/test_gpu_compose_f64.py runs the library on -- the fp32 oracle
(``cindm_oracle.p_mean_variance``, ``_outside_aggregate``, ``gradient_4body``, ``gradient_3body``) lies within
(n_e + 4) * 2^-24 * A_e of ``compose_predict_f64`` element by element, on model outputs both sides share: a row-wise toy model
(a seeded matrix, one shift along time, tanh; evaluated in float64 and rounded, so its fp32 value does not depend on how rows are
batched) stands in for the U-Net, evaluated once on ``compose_rows`` and handed to the oracle as ``d.model`` /
``d.model_unconditioned``.  The reference's own execution (tests/golden/compose_grid.npz, oracle/make_golden_compose.py) is held to
the same bound, and six mutations of ``compose_predict_f64`` each leave it on at least one grid point.

What the oracle cannot express, and what stands in:
  * gradient(x, t, 3) at a batch other than 20 (the reference's literal slices): the three sums written out here (``_gradient3``).
  * pred_noise of the two outside modes (the reference computes it per pair and returns none): the oracle's per-pair
    ``p_mean_variance`` aggregated as ``_outside_aggregate`` aggregates (``_outside_eps32``).
  * outside modes with conditioned_steps > 0: the reference raises (the golden records its message), the oracle raises, the library
    refuses, ``compose_predict_f64`` raises ValueError with the library's text.
"""
import os

import numpy as np
import pytest
import torch

import cindm_oracle as O
import f64_reference as R
import compose_cases as C


# ------------------------------------------------------------------ the toy model
def _toy(F, seed):
    M = torch.randn((F, F), generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * 0.6

    def model(x, t):
        xd = x.double()
        y = xd + 0.5 * torch.roll(xd, 1, dims=1)
        return (1.5 * torch.tanh(y @ M + 0.3 * (t.double().view(-1, 1, 1) / 1000.0))).to(x.dtype)
    return model


TOY8, TOY4 = _toy(8, 8), _toy(4, 4)
TAB = {obj: O.make_schedule("cosine", 1000, obj) for obj in C.OBJECTIVES}


def _desc(d, objective="pred_noise", clip=True, uncond_coef=1.4):
    mode, nb, w, cs, k = d
    return R.ComposeCase(mode, nb, w, cs, C.WINDOW, k, objective, clip, uncond_coef)


def _oracle_d(desc):
    d = O.Diffusion1D({"final_conv.1.weight": torch.zeros(8, 1)}, image_size=C.WINDOW - desc.cond_steps, conditioned_steps=desc.cond_steps,
                      objective=desc.objective)
    d.model, d.model_unconditioned = TOY8, TOY4
    d.sd_uncond = True if desc.mode == "multibody" else None
    return d


def _kw(desc):
    return dict(compose_mode=desc.mode, n_composed=desc.n_windows - 1, compose_start_step=desc.compose_start_step,
                single_model_step=desc.window, compose_n_bodies=desc.n_bodies)


def _toy_outputs(desc, x, cond, t):
    """The toy models once on ``compose_rows`` -> (pair_eps [W, P, B, window, 8], single_eps | None), fp32."""
    pair_in, single_in = R.compose_rows(desc, x, cond)
    B = x.shape[0]
    if desc.mode == "plain":
        return TOY8(pair_in, torch.full((B,), t)).view(1, 1, B, desc.full_len, 8), None
    P = len(R.compose_pairs(desc.n_bodies))
    E = TOY8(pair_in, torch.full((pair_in.shape[0],), t)).view(desc.n_windows, P, B, desc.window, 8)
    U = None if single_in is None else TOY4(single_in, torch.full((single_in.shape[0],), t)).view(desc.n_bodies, B, desc.window, 4)
    return E, U


def _outside_eps32(d, desc, x, t):
    """pred_noise of the outside modes in fp32: per (window, pair) ``O.p_mean_variance``'s, aggregated as ``O._outside_aggregate`` does."""
    nb, W, cs, T = desc.n_bodies, desc.n_windows, desc.compose_start_step, desc.window
    agg = torch.zeros((W,) + tuple(x.shape[:2]) + (nb, nb, 4))
    mask = torch.zeros((W,) + tuple(x.shape))
    for kk in range(W):
        lo = kk * cs
        mask[kk, :, lo:lo + T] = 1.0
        for ii, jj in R.compose_pairs(nb):
            index = torch.cat([torch.arange(ii * 4, (ii + 1) * 4), torch.arange(jj * 4, (jj + 1) * 4)])
            e = O.p_mean_variance(d, x[:, lo:lo + T, index].contiguous(), None, t, desc.clip)[3]
            agg[kk, :, lo:lo + T, jj, ii] = e[..., :4]
            agg[kk, :, lo:lo + T, ii, jj] = e[..., 4:]
    if desc.mode == "mean":
        return (agg.sum(-3) / (nb - 1)).flatten(start_dim=3).sum(0) / mask.sum(0)
    return agg.sum(-3).flatten(start_dim=3).sum(0) / mask.mean(0)


def _gradient3(d, x, t):
    """gradient(x, t, 3) at any batch: pairs (0,1), (0,2), (1,2) one by one, n_i = the two pair predictions of body i - its single one."""
    B = x.shape[0]
    body = [x[:, :, 4 * i:4 * i + 4] for i in range(3)]
    tt = torch.full((B,), t)
    e01, e02, e12 = (d.model(torch.cat([body[i], body[j]], dim=2), tt) for i, j in ((0, 1), (0, 2), (1, 2)))
    u = [d.model_unconditioned(b.contiguous(), tt) for b in body]
    return torch.cat([e01[..., :4] + e02[..., :4] - u[0], e01[..., 4:] + e12[..., :4] - u[1], e02[..., 4:] + e12[..., 4:] - u[2]], dim=2)


def _oracle32(desc, x, cond, t, only_eps=False):
    """{"mean", "x_start", "pred_noise"} of the fp32 oracle (``only_eps``: gradient())."""
    d = _oracle_d(desc)
    if only_eps:
        if desc.n_bodies == 4:
            return {"pred_noise": O.gradient_4body(d, x, t)}
        return {"pred_noise": O.gradient_3body(d, x, t) if x.shape[0] == 20 else _gradient3(d, x, t)}
    if desc.mode in C.OUTSIDE:
        mean, _, x0 = O._outside_aggregate(d, x, cond, t, clip_denoised=desc.clip, **_kw(desc))
        return {"mean": mean, "x_start": x0, "pred_noise": _outside_eps32(d, desc, x, t)}
    kw = _kw(desc) if "inside" in desc.mode else {}
    mean, _, x0, eps = O.p_mean_variance(d, x, cond, t, desc.clip, **kw)
    return {"mean": mean, "x_start": x0, "pred_noise": eps}


def _ratios(got, desc, x, cond, t, E, U, mut=None):
    """-> ({output: largest |got - ref| / bound}, ref x_start) against ``compose_predict_f64`` (or a mutation of it)."""
    mean, x0, eps, A = R.compose_predict_f64(TAB[desc.objective], desc, x, cond, t, E, U, _mut=mut)
    ref, bound = {"mean": mean, "x_start": x0, "pred_noise": eps}, R.compose_bound(desc, A)
    out = {}
    for k, v in got.items():
        assert v.shape == ref[k].shape, (k, v.shape, ref[k].shape)
        err = (v.double() - ref[k]).abs()
        out[k] = float(torch.where(err == 0, torch.zeros_like(err), err / bound[k]).max())
    return out, x0


def _point(d, objective="pred_noise", clip=True, t=C.CROSS_T, B=C.CROSS_B, mut=None, only_eps=False, coef=1.4):
    desc = _desc(d, objective, clip, coef)
    x, cond = C.make_state(d, t, B)
    if only_eps:
        desc = desc.replace(clip=False)
    E, U = _toy_outputs(desc, x, cond, t)
    return _ratios(_oracle32(desc, x, cond, t, only_eps), desc, x, cond, t, E, U, mut)


def _clamped(x0):
    return float((x0.abs() == 1.0).double().mean())


# ------------------------------------------------------------------ the grid
@pytest.mark.parametrize("mode", C.WINDOWED)
def test_cross_oracle_within_bound(mode):
    """The full cross at pred_noise, clip on, t = 500, B = 3.  The clamp bites on part of x_start everywhere."""
    for d in [q for q in C.CROSS if q[0] == mode]:
        if mode in C.OUTSIDE and d[4] > 0:
            desc = _desc(d)
            x, cond = C.make_state(d, C.CROSS_T, C.CROSS_B)
            with pytest.raises(ValueError, match=C.REFUSAL_OUTSIDE_COND):
                R.compose_predict_f64(TAB["pred_noise"], desc, x, cond, C.CROSS_T, None)
            if d[1] > 2:      # the full-width cond does not concatenate with an 8-feature window (two bodies: 28 rows, which only a U-Net minds)
                with pytest.raises(RuntimeError):
                    O._outside_aggregate(_oracle_d(desc), x, cond, C.CROSS_T, clip_denoised=True, **_kw(desc))
            continue
        r, x0 = _point(d)
        assert max(r.values()) <= 1.0, (d, r)
        assert 0.02 < _clamped(x0) < 0.98, (d, _clamped(x0))


@pytest.mark.parametrize("name", list(C.DESCRIPTORS))
def test_descriptors_oracle_within_bound(name):
    """Objective x clip x t x B on the descriptors.  The clamped fraction is asserted where the schedule leaves room for both kinds:
    at t = 999 sqrt_recip_alphas_cumprod is above 1e4 and predict_start_from_noise of a 0.7-sigma state is clamped everywhere."""
    d = C.DESCRIPTORS[name]
    if d[0] in C.OUTSIDE and d[4] > 0:
        x, cond = C.make_state(d, 500, 3)
        with pytest.raises(ValueError, match=C.REFUSAL_OUTSIDE_COND):
            R.compose_predict_f64(TAB["pred_noise"], _desc(d), x, cond, 500, None)
        return
    for obj in C.OBJECTIVES:
        for clip in C.DESC_CLIP:
            for t in C.DESC_T:
                for B in C.DESC_B:
                    r, x0 = _point(d, obj, clip, t, B)
                    assert max(r.values()) <= 1.0, (name, obj, clip, t, B, r)
                    if clip and t == 500 and B == 3:
                        assert 0.02 < _clamped(x0) < 0.98, (name, obj, t, _clamped(x0))


def test_multibody_oracle_within_bound():
    d = ("multibody", 4, 1, 0, C.MB_COND)
    for obj in C.OBJECTIVES:
        for clip in C.DESC_CLIP:
            for t in C.MB_T:
                for B in C.MB_B:
                    r, _ = _point(d, obj, clip, t, B)
                    assert max(r.values()) <= 1.0, (obj, clip, t, B, r)


@pytest.mark.parametrize("nb", C.GRADIENT_NB)
def test_gradient_oracle_within_bound(nb):
    """gradient(x, t, nb): the 3-body branch through the oracle at batch 20 only (its literal slices), through ``_gradient3`` elsewhere;
    at batch 20 the two are the same numbers."""
    d = ("multibody", nb, 1, 0, 0)
    for B in C.GRADIENT_B:
        r, _ = _point(d, t=C.GRADIENT_T, B=B, only_eps=True, coef=1.4 if nb == 4 else 1.0)
        assert r["pred_noise"] <= 1.0, (nb, B, r)
    if nb == 3:
        x, _ = C.make_state(d, C.GRADIENT_T, 20)
        dd = _oracle_d(_desc(d))
        assert torch.equal(O.gradient_3body(dd, x, C.GRADIENT_T), _gradient3(dd, x, C.GRADIENT_T))


def test_zero_noise_step_is_the_mean():
    """``p_sample_compose_outside`` with zero noise hands back ``_outside_aggregate``'s mean: the step adds nothing to the composition."""
    d = C.DESCRIPTORS["mean-nb4-w3-cs16"]
    desc = _desc(d)
    x, _ = C.make_state(d, 500, 3)
    od = _oracle_d(desc)
    out, x0 = O.p_sample_compose_outside(od, x, None, 500, torch.zeros_like(x), **_kw(desc))
    mean, _, xs = O._outside_aggregate(od, x, None, 500, clip_denoised=True, **_kw(desc))
    assert torch.equal(out, mean) and torch.equal(x0, xs)


# ------------------------------------------------------------------ the reference's own execution
def test_golden_within_bound(gold_dir):
    g = np.load(os.path.join(gold_dir, "compose_grid.npz"))
    for name, d in C.GOLDEN.items():
        desc = _desc(d)
        if name + ".raises" in g.files:
            # the reference cannot run the descriptor; what the library does there (it refuses) is our definition
            assert d[0] in C.OUTSIDE and d[4] > 0 and str(g[name + ".raises"])
            with pytest.raises(ValueError, match=C.REFUSAL_OUTSIDE_COND):
                R.compose_predict_f64(TAB["pred_noise"], desc, torch.zeros(1, desc.state_len, 4 * desc.n_bodies),
                                      torch.zeros(1, desc.cond_steps, 4 * desc.n_bodies), C.GOLDEN_T, None)
            continue
        x = torch.from_numpy(g[name + ".x"])
        cond = torch.from_numpy(g[name + ".cond"]) if name + ".cond" in g.files else None
        E = torch.from_numpy(g[name + ".pair_eps"])
        assert x.shape[0] == C.GOLDEN_B and E.shape[:2] == (desc.n_windows, len(R.compose_pairs(desc.n_bodies)))
        got = {k: torch.from_numpy(g[f"{name}.{k}"]) for k in ("mean", "x_start", "pred_noise") if f"{name}.{k}" in g.files}
        assert {"mean", "x_start"} <= set(got)
        r, _ = _ratios(got, desc, x, cond, int(g[name + ".t"]), E, None)
        assert max(r.values()) <= 1.0, (name, r)
        # and the rows the reference's pair model saw are compose_rows', in its order
        assert torch.equal(torch.from_numpy(g[name + ".pair_in"]), R.compose_rows(desc, x, cond)[0])
    assert sum(1 for n in C.GOLDEN if n + ".raises" in g.files) == 1


# ------------------------------------------------------------------ the bound means something
MUTATIONS = {
    # mutation: grid points on which it must show (descriptor, objective, clip)
    "slot": [(("mean-inside", 2, 1, 4, 0), "pred_noise", True), (("mean", 3, 2, 24, 0), "pred_noise", True)],
    "pair_index": [(("sum-inside", 3, 3, 4, 0), "pred_noise", True), (("noise_sum", 3, 3, 16, 0), "pred_noise", True)],
    "cover": [(("mean-inside", 3, 3, 4, 0), "pred_noise", True), (("sum-inside", 4, 4, 1, 0), "pred_noise", True), (("mean", 2, 3, 16, 0), "pred_noise", True)],
    "nb": [(("mean-inside", 3, 2, 24, 0), "pred_noise", True), (("mean", 8, 1, 4, 0), "pred_noise", True)],
    "cond_offset": [(("mean-inside", 3, 3, 16, 4), "pred_noise", True), (("sum-inside", 2, 1, 4, 4), "pred_noise", True)],
    "clamp_after": [(("mean", 3, 2, 24, 0), "pred_noise", True), (("mean", 4, 3, 16, 0), "pred_x0", True)],
}


@pytest.mark.parametrize("mut", list(MUTATIONS))
def test_mutation_leaves_the_bound(mut):
    """A swapped slot, a pair index off by one, the divisor cover <-> W, nb - 1 <-> nb, the cond offset dropped from the window row,
    the clamp after the average in outside/mean: each puts the fp32 oracle OUTSIDE the bound of the mutated function, on every point
    listed for it (all of them points of the grid), by a wide margin."""
    for d, obj, clip in MUTATIONS[mut]:
        assert d in C.CROSS or d in C.DESCRIPTORS.values()
        good, _ = _point(d, obj, clip)
        bad, _ = _point(d, obj, clip, mut=(mut,))
        assert max(good.values()) <= 1.0 and max(bad.values()) > 100.0, (mut, d, good, bad)


def test_min_through_the_clamp_alone_is_no_bound():
    """Why ``A`` passes min(., 1) through the clamp only where the clamp surely acts: with min(., 1) on every element the fp32 oracle
    itself exceeds the bound where x_start's terms cancel inside [-1, 1], so that rule would fail correct code.  noise_sum under pred_x0
    at t = 999: x_start = ra x - rb ((ra x - out) / rb) with ra above 1e4 and the result below one -- 3377 x that bound on x_start,
    117 x on the mean; sum-inside with eight bodies and four windows at t = 500 (terms of tens): 1.14 x."""
    d = C.DESCRIPTORS["noise_sum-nb2-w1"]
    r, _ = _point(d, "pred_x0", True, 999, 3, mut=("min_clamp",))
    assert r["x_start"] > 100.0 and r["mean"] > 10.0, r
    r, _ = _point(d, "pred_x0", True, 999, 3)
    assert max(r.values()) <= 1.0, r
    r, _ = _point(("sum-inside", 8, 4, 1, 0), mut=("min_clamp",))
    assert r["x_start"] > 1.0, r


def test_roundings_formula():
    """n_e at the ends of the grid, by hand: plain pred_noise 0 / 3 / 6; mean-inside, 8 bodies, cover 4: 7 + 4 + 2 = 13 on the output."""
    n = R.compose_roundings("plain", 2, 1, "pred_noise")
    assert (n["pred_noise"], n["x_start"], n["mean"]) == (0, 3, 6)
    n = R.compose_roundings("mean-inside", 8, 4, "pred_noise")
    assert (n["pred_noise"], n["x_start"], n["mean"]) == (13, 16, 19)
    n = R.compose_roundings("sum-inside", 3, 2, "pred_x0")
    assert (n["x_start"], n["pred_noise"], n["mean"]) == (6, 9, 9)
    n = R.compose_roundings("noise_sum", 3, 2, "pred_v")
    assert (n["pred_noise"], n["x_start"], n["mean"]) == (12, 15, 18)
    n = R.compose_roundings("multibody", 4, 1, "pred_noise")
    assert (n["pred_noise"], n["x_start"], n["mean"]) == (5, 8, 11)
    assert R.BOUND_SLACK == 4 and R.U24 == 2.0 ** -24
