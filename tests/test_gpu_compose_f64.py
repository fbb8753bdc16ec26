"""GPU (MI355X): gather + aggregation + update of the composed predictions, held to the float64 composition of
oracle/f64_reference.py (``compose_predict_f64``) element by element, over the grid of tests/compose_cases.py.

Per case: the state (and condition) is seeded normal x 0.7; the LIBRARY evaluates its pair (and single-body) U-Net once on exactly the
rows, in the row order, of ``compose_rows`` -- E; the library's ``p_mean_variance`` (the two outside modes: the descriptor
``p_sample_compose_outside`` builds, through ``_predict``; multibody also ``gradient``) gives (mean, x_start, pred_noise); the float64
composition of E gives the reference and the magnitudes A; asserted, on all three outputs,

    |got - ref|  <=  (n_e + 4) * 2^-24 * A_e                                  (f64_reference.compose_bound)

The U-Net's own error is in E on both sides and cancels: a wrong row, slot, divisor or seam offset is an O(1) violation on the
elements it touches.  tests/test_compose_f64_host.py proves the reference first (the fp32 oracle and the reference project's own
execution stay within the same bound; six mutations leave it).  A descriptor the library refuses is an assertion on the refusal's text.

The steps (``p_sample`` / ``p_sample_compose_inside`` / ``_outside`` with an explicit noise) on the descriptors: x0 is
``p_mean_variance``'s x_start bit for bit; the new state is its mean bit for bit at t = 0 and within three fp32 roundings (and one
ulp of sigma for expf) of mean + exp(0.5 logvar) z in float64 at t > 0.

Measured on an MI355X (profiles/compose_f64.json, 605 cases): the largest ratio is 0.319 (plain, pred_x0: the re-derived pred_noise);
windowed modes <= 0.265, multibody and gradient() <= 0.239, under the two options <= 0.257.  What the grid found in the update before
it was fixed (the same module on the earlier kernel): noise_sum with three bodies and two windows under pred_x0 / pred_v summed raw
outputs instead of each pair's re-derived pred_noise -- x_start 2.2e6 x the bound, pred_noise 17 x under pred_v -- and the pred_noise
of outside mean under pred_x0 / pred_v was the average of raw outputs (1.5e6 x / 25 x); a model forward on 84 rows after one on 336
was refused with "workspace too small" (``test_forward_fewer_rows_after_more``).

With CINDM_COMPOSE_F64_JSON=<path> the module writes every case's largest err / bound with its output and element index
(profiles/compose_f64.json is such a run; the summary at its head)."""
import json
import os

import pytest
import torch

import cindm_amd
import f64_reference as R
import compose_cases as C
from cindm_oracle import make_schedule
from test_gpu_parity import build_unet

pytestmark = pytest.mark.gpu

# A (case, output) that cannot hold the bound needs its derivation written next to it.  None taken.
EXCEPTIONS = {}

_LOG = {}
_FRAC = {}
TAB = {obj: make_schedule("cosine", 1000, obj) for obj in C.OBJECTIVES}


@pytest.fixture(scope="module", autouse=True)
def _write_log():
    yield
    path = os.environ.get("CINDM_COMPOSE_F64_JSON")
    if path and _LOG:
        flat = sorted(((v["ratio"], k) for k, v in _LOG.items()), reverse=True)
        doc = {"metric": "largest |got - ref| / ((n_e + 4) * 2^-24 * A_e) over the elements of (mean, x_start, pred_noise); ref, A, n_e: "
                         "f64_reference.compose_predict_f64 / compose_roundings on the library's own U-Net outputs",
               "slack": R.BOUND_SLACK, "cases_run": len(_LOG), "largest": round(flat[0][0], 4),
               "ten_largest": [dict(case=k, **_LOG[k]) for _, k in flat[:10]],
               "clamped_fraction_min_max": [round(min(_FRAC.values()), 3), round(max(_FRAC.values()), 3)] if _FRAC else None,
               "cases": _LOG}
        with open(path, "w") as f:
            json.dump(doc, f, indent=0)
            f.write("\n")


@pytest.fixture(scope="module")
def unets(device):
    return build_unet(device)[0], build_unet(device, F=4)[0]


_DIFF = {}


def _diff(device, unets, objective, cond, multibody=False):
    """One GaussianDiffusion1D per (objective, conditioned_steps); the multibody ones (image_size 20 + 4 conditioned steps) hold the
    single-body model too."""
    key = (objective, cond, multibody)
    if key not in _DIFF:
        d = cindm_amd.GaussianDiffusion1D(unets[0], model_unconditioned=unets[1] if multibody else None, image_size=C.WINDOW - cond,
                                          conditioned_steps=cond, timesteps=1000, sampling_timesteps=1000, loss_type="l1", objective=objective)
        _DIFF[key] = d.to(device)
    return _DIFF[key]


def _tag(d, obj, clip, t, B, extra=""):
    mode, nb, w, cs, k = d
    return f"{mode}-nb{nb}-w{w}-cs{cs}-c{k}-{obj}-clip{int(clip)}-t{t}-B{B}{extra}"


def _kw(desc):
    return dict(compose_mode=desc.mode, n_composed=desc.n_windows - 1, compose_start_step=desc.compose_start_step,
                single_model_step=desc.window, compose_n_bodies=desc.n_bodies)


def _forward(m, rows, t, device):
    return m(rows.to(device), torch.full((rows.shape[0],), t, device=device)).cpu()


def _unet_outputs(unets, desc, x, cond, t, device):
    """The library's U-Nets, one forward each, on ``compose_rows`` -> (pair_eps [W, P, B, window, 8], single_eps | None)."""
    pair_in, single_in = R.compose_rows(desc, x, cond)
    B = x.shape[0]
    E = _forward(unets[0], pair_in, t, device)
    E = E.view(1, 1, B, desc.full_len, 8) if desc.mode == "plain" else E.view(desc.n_windows, len(R.compose_pairs(desc.n_bodies)), B, desc.window, 8)
    U = None if single_in is None else _forward(unets[1], single_in, t, device).view(desc.n_bodies, B, desc.window, 4)
    return E, U


def _predict(dev_d, desc, x, cond, t, device):
    """(mean, x_start, pred_noise) of the library."""
    xd, cd = x.to(device), None if cond is None else cond.to(device)
    if desc.mode in C.OUTSIDE:            # p_mean_variance has no outside form: the descriptor p_sample_compose_outside builds
        dd = dev_d._desc_for(xd.shape, desc.mode, desc.n_windows - 1, desc.compose_start_step, desc.window, desc.n_bodies,
                             clip=desc.clip, outside=True)
        return dev_d._predict(xd, cd, t, dd)
    kw = _kw(desc) if "inside" in desc.mode else {}
    mean, _, _, x0, eps = dev_d.p_mean_variance(xd, cd, t, clip_denoised=desc.clip, **kw)
    return mean, x0, eps


def _hold(tag, got, desc, x, cond, t, E, U):
    mean, x0, eps, A = R.compose_predict_f64(TAB[desc.objective], desc, x, cond, t, E.double(), None if U is None else U.double())
    ref, bound = {"mean": mean, "x_start": x0, "pred_noise": eps}, R.compose_bound(desc, A)
    worst = (-1.0, None, None)
    for k, v in got.items():
        v = v.cpu()
        assert v.shape == ref[k].shape and bool(torch.isfinite(v).all()), (tag, k)
        err = (v.double() - ref[k]).abs()
        ratio = torch.where(err == 0, torch.zeros_like(err), err / bound[k])
        i = int(ratio.argmax())
        if float(ratio.flatten()[i]) > worst[0]:
            worst = (float(ratio.flatten()[i]), k, [int(q) for q in torch.unravel_index(torch.tensor(i), ratio.shape)])
    print(f"{tag}: err/bound {worst[0]:.4f} at {worst[1]} {worst[2]}")
    _LOG[tag] = {"ratio": round(worst[0], 4), "output": worst[1], "index": worst[2]}
    assert worst[0] <= EXCEPTIONS.get((tag, worst[1]), 1.0), (tag, worst)
    return x0


def _case(device, unets, d, obj="pred_noise", clip=True, t=C.CROSS_T, B=C.CROSS_B, extra="", frac=False):
    mode, nb, w, cs, k = d
    desc = R.ComposeCase(mode, nb, w, cs, C.WINDOW, k, obj, clip)
    x, cond = C.make_state(d, t, B)
    dev_d = _diff(device, unets, obj, k, multibody=(mode == "multibody"))
    tag = _tag(d, obj, clip, t, B, extra)
    if mode in C.OUTSIDE and k > 0:
        with pytest.raises(cindm_amd._ffi.CindmError, match=C.REFUSAL_OUTSIDE_COND):
            _predict(dev_d, desc, x, cond, t, device)
        return
    E, U = _unet_outputs(unets, desc, x, cond, t, device)
    got = dict(zip(("mean", "x_start", "pred_noise"), _predict(dev_d, desc, x, cond, t, device)))
    x0 = _hold(tag, got, desc, x, cond, t, E, U)
    if frac and clip:
        _FRAC[tag] = float((x0.abs() == 1.0).double().mean())
        assert 0.02 < _FRAC[tag] < 0.98, (tag, _FRAC[tag])


def test_forward_repeats_bit_identically(device, unets):
    """E is evaluated apart from the step that is judged on it: the same rows give the same bits, for both models."""
    g = torch.Generator().manual_seed(5)
    for m, F in zip(unets, (8, 4)):
        rows = torch.randn((18, C.WINDOW, F), generator=g) * C.X_SCALE
        assert torch.equal(_forward(m, rows, C.CROSS_T, device), _forward(m, rows, C.CROSS_T, device))


def test_forward_fewer_rows_after_more(device, unets):
    """336 rows (eight bodies, four windows, three designs), then 84 (one window): the plan of the smaller batch needs the larger
    workspace, and the model's cached one is sized by the bytes a batch needs, not by its row count (this order used to be refused with
    "workspace too small")."""
    rows = torch.randn((336, C.WINDOW, 8), generator=torch.Generator().manual_seed(6)) * C.X_SCALE
    big = _forward(unets[0], rows, C.CROSS_T, device)
    small = _forward(unets[0], rows[:84], C.CROSS_T, device)
    assert float((small - big[:84]).abs().max() / big.abs().max()) < 2e-5


@pytest.mark.parametrize("mode,nb,cond", [(m, nb, k) for m in C.WINDOWED for nb in C.CROSS_NB for k in C.CROSS_COND],
                         ids=[f"{m}-nb{nb}-c{k}" for m in C.WINDOWED for nb in C.CROSS_NB for k in C.CROSS_COND])
def test_cross(device, unets, mode, nb, cond):
    """The full cross at pred_noise, clip on, t = 500, B = 3: one window, abutting windows, strides 16 and 4, stride 1; the clamp bites
    on part of x_start in every case.  The outside modes with conditioned steps are refused."""
    cases = [d for d in C.CROSS if (d[0], d[1], d[4]) == (mode, nb, cond)]
    assert len(cases) == len(C.CROSS_WCS)
    for d in cases:
        _case(device, unets, d, frac=True)


@pytest.mark.parametrize("obj", C.OBJECTIVES)
@pytest.mark.parametrize("name", list(C.DESCRIPTORS))
def test_descriptors(device, unets, name, obj):
    """Objective x clip x t in {0, 1, 500, 999} x B in {1, 3} on the descriptors.  The clamped fraction is asserted under pred_noise at
    t = 500: under pred_x0 x_start IS the model's output (mean |.| 0.29 for the synthetic weights: the clamp bites on under 1 %, whatever
    the state's scale), and at t = 999 predict_start_from_noise multiplies the state by more than 1e4 and everything is clamped."""
    for clip in C.DESC_CLIP:
        for t in C.DESC_T:
            for B in C.DESC_B:
                _case(device, unets, C.DESCRIPTORS[name], obj, clip, t, B, frac=(t == 500 and B == 3 and obj == "pred_noise"))


@pytest.mark.parametrize("obj", C.OBJECTIVES)
def test_multibody(device, unets, obj):
    """Four bodies through p_mean_variance with the single-body model set: six pairs and four single-body rows per design, 4 conditioned steps."""
    for clip in C.DESC_CLIP:
        for t in C.MB_T:
            for B in C.MB_B:
                _case(device, unets, ("multibody", 4, 1, 0, C.MB_COND), obj, clip, t, B)


@pytest.mark.parametrize("nb", C.GRADIENT_NB)
def test_gradient(device, unets, nb):
    """gradient(x, t, nb): three bodies (weight 1) at any batch give what the reference's branch gives at its batch of 20."""
    d = ("multibody", nb, 1, 0, 0)
    dev_d = _diff(device, unets, "pred_noise", 0, multibody=True)
    for B in C.GRADIENT_B:
        desc = R.ComposeCase("multibody", nb, 1, 0, C.WINDOW, 0, "pred_noise", False, 1.4 if nb == 4 else 1.0)
        x, _ = C.make_state(d, C.GRADIENT_T, B)
        E, U = _unet_outputs(unets, desc, x, None, C.GRADIENT_T, device)
        got = {"pred_noise": dev_d.gradient(x.to(device), C.GRADIENT_T, nb)}
        _hold(_tag(d, "pred_noise", False, C.GRADIENT_T, B, "-gradient"), got, desc, x, None, C.GRADIENT_T, E, U)


@pytest.mark.parametrize("opts", C.OPTIONS, ids=["-".join(f"{k}={v}" for k, v in o.items()) for o in C.OPTIONS])
def test_descriptors_under_options(device, unets, opts):
    """The descriptors once more with compose_gather_kernel launched where the first level kernel would read the state in place, and on
    the exchange-free kernels: the same bound."""
    before = {k: unets[0].get_option(k) for k in opts}
    for k, v in opts.items():
        unets[0].set_option(k, v)
    try:
        for k, v in opts.items():
            assert unets[0].get_option(k) == v
        for name, d in C.DESCRIPTORS.items():
            _case(device, unets, d, extra="-" + "-".join(f"{k}={v}" for k, v in opts.items()))
    finally:
        for k, v in before.items():
            unets[0].set_option(k, v)


@pytest.mark.parametrize("name", list(C.DESCRIPTORS))
def test_step_on_descriptors(device, unets, name):
    d = C.DESCRIPTORS[name]
    mode, nb, w, cs, k = d
    if mode in C.OUTSIDE and k > 0:
        return                      # refused: test_descriptors asserts the text
    desc = R.ComposeCase(mode, nb, w, cs, C.WINDOW, k)
    dev_d = _diff(device, unets, "pred_noise", k)
    for t in (0, 500, 999):
        x, cond = C.make_state(d, t, 3)
        z = torch.randn(x.shape, generator=torch.Generator().manual_seed(t + 17))
        xd, cd, zd = x.to(device), None if cond is None else cond.to(device), z.to(device)
        if mode == "plain":
            out, x0 = dev_d.p_sample(xd, cd, t, noise=zd)
        elif mode in C.OUTSIDE:
            out, x0 = dev_d.p_sample_compose_outside(xd, cd, t, noise=zd, **_kw(desc))
        else:
            out, x0 = dev_d.p_sample_compose_inside(xd, cd, t, noise=zd, **_kw(desc))
        mean, xs, _ = _predict(dev_d, desc, x, cond, t, device)
        assert torch.equal(x0, xs), (name, t)
        if t == 0:
            assert torch.equal(out, mean), name
            continue
        m64, z64 = mean.cpu().double(), z.double()
        sigma = torch.exp(0.5 * TAB["pred_noise"]["posterior_log_variance_clipped"][t].double())
        err = (out.cpu().double() - (m64 + sigma * z64)).abs()
        bound = 3 * R.U24 * (m64.abs() + (sigma * z64).abs()) + 2.0 ** -23 * sigma * z64.abs()
        assert bool((err <= bound).all()), (name, t, float((err / bound).max()))


def test_exceptions_stay_empty():
    assert EXCEPTIONS == {} and R.BOUND_SLACK == 4
