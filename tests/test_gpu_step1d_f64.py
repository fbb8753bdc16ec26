"""GPU (MI355X): the tail of every 1-D reverse step -- the design gradient, eta_t, the initial_state_overwrite, the relaxation, the DDPM
and the DDIM tail, the multistep term and the inpainting rows of ``compose_update_body`` in all its instantiations, and the fused copy
``plain_step_value`` -- held to the float64 statement of oracle/f64_reference.py (``design_grad_f64``, ``step1d_update_f64``) element by
element, over the grid of tests/step1d_cases.py.

Per case: the LIBRARY evaluates its U-Net once on ``R.compose_rows`` of the case's state -- E (``_unet_outputs`` of
tests/test_gpu_compose_f64.py); ``compose_predict_f64`` and the statement give the reference, A and n_e from that E; asserted

    |got - ref|  <=  (n_e + 4) * 2^-24 * A_e        on every element of the new state.

The U-Net's own error is in E on both sides and cancels.  tests/test_step1d_f64_host.py proves the statement first (the fp32 oracle
stays within the same bound over the same grid; thirteen mutations leave it by more than 100 x).  Every draw comes from a tape.

Entries: ``_run_guided_loop(x, None, desc, obj.descriptor(guidance), t, t, ...)`` for the guided DDPM step without recurrence and with
``-recurrence-1`` (one evaluation: the result is pred + sigma z of that iteration), ``_run_loop`` for the unguided tail with inpainting
rows, ``ddim_sample(..., init_img=x, step_range=(i, i + 1), noise=tape[, design_fn, solver="dpmpp-2m", history=h])`` for the DDIM
updates; the unguided pred_noise pairs run on the fused route (``plain_step_value`` inside the U-Net's last kernel) and with the option
``fuse_update`` off (``compose_update_kernel``), and ``last_step_info()`` says which one ran.

The relaxation needs two evaluations (``-recurrence-2``) and the state between them is not visible: those cases run on a model whose
output does not depend on its input (``step1d_cases.frozen_state_dict``: final_conv.1.weight = 0, a distinct bias per feature), so
that the float64 statement follows the iteration chain exactly -- ``test_frozen_model_ignores_its_input`` asserts the property -- and
on the objectives whose gradient is linear in the state (point and table L2square, quadratic, tc).  n_e accumulates over the two
iterations and A propagates through the second prediction (``compose_repredict_f64``); a wrong coefficient stays an O(1) violation.
The gather's indexing is NOT exercised by these cases (every row of E is the same): tests/test_gpu_compose_f64.py holds it.

Also asserted: the multistep history a segment call hands back is the step's x_start bit for bit (one-evaluation cases), and the last
pair and kappa = 0 leave a poisoned (NaN) history unread.

Measured on an MI355X (profiles/step1d_f64.json, 262 cases: the 244 of the grid and the 18 unguided DDIM pairs again with
``fuse_update`` off): the largest ratio is 0.2505 (guided DDPM, table L2square under standard-alpha, two windows, four bodies, t = 600);
guided DDIM <= 0.239, the relaxation cases <= 0.176, the unguided DDIM pairs <= 0.234, with the same ratio on the fused route and on compose_update_kernel for every pair.  The
fp32 oracle's largest over the same grid is the same 0.2505.  What the grid found before it was fixed: the unguided DDIM update under
pred_x0 / pred_v with the clamp on combined x_start with the pred_noise of the UNCLAMPED x_start, where ddim_sample's
model_predictions(clip_x_start = True) re-derives it from the clamped one -- 48 x the bound on the pair at t = 999, 2.3e5 x at t = 499
(on the 0.5 - 8 % of the elements the clamp holds; nothing on the last pair, which returns x_start).  compose_update_clamped_kernel,
an instantiation of compose_update_body of its own, now serves that combination; every other kernel kept its code.

With CINDM_STEP1D_F64_JSON=<path> the module writes every case's largest err / bound with its element index and the share of x_start
the clamp holds (profiles/step1d_f64.json is such a run)."""
import json
import os

import pytest
import torch

import cindm_amd
import f64_reference as R
import step1d_cases as S
from cindm_oracle import make_schedule
from test_gpu_compose_f64 import _unet_outputs
from test_gpu_parity import build_unet

pytestmark = pytest.mark.gpu

# A case that cannot hold the bound needs its derivation written next to it.  None taken.
EXCEPTIONS = {}

_LOG = {}
TAB = {obj: make_schedule("cosine", 1000, obj) for obj in S.OBJECTIVES}


@pytest.fixture(scope="module", autouse=True)
def _write_log():
    yield
    path = os.environ.get("CINDM_STEP1D_F64_JSON")
    if path and _LOG:
        flat = sorted(((v["ratio"], k) for k, v in _LOG.items()), reverse=True)
        doc = {"metric": "largest |got - ref| / ((n_e + 4) * 2^-24 * A_e) over the elements of the new state; ref, A, n_e: "
                         "f64_reference.compose_predict_f64 / design_grad_f64 / step1d_update_f64 on the library's own U-Net outputs",
               "slack": R.BOUND_SLACK, "cases_run": len(_LOG), "largest": round(flat[0][0], 4),
               "ten_largest": [dict(case=k, **_LOG[k]) for _, k in flat[:10]], "cases": _LOG}
        with open(path, "w") as f:
            json.dump(doc, f, indent=0)
            f.write("\n")


@pytest.fixture(scope="module")
def models(device):
    """{frozen: (model, state dict)}: the synthetic pair U-Net and the same one with the frozen output."""
    m, sd = build_unet(device)
    fsd = S.frozen_state_dict(sd)
    fm = cindm_amd.TemporalUnet1D(S.WINDOW, 8, False, attention=True)
    fm.load_state_dict(fsd, strict=True)
    return {False: (m, sd), True: (fm.to(device), fsd)}


_DIFF = {}


def _diff(device, m, objective, steps=1000, eta=0.0):
    key = (id(m), objective, steps, eta)
    if key not in _DIFF:
        _DIFF[key] = cindm_amd.GaussianDiffusion1D(m, image_size=S.WINDOW, conditioned_steps=0, timesteps=1000, sampling_timesteps=steps,
                                                   loss_type="l1", objective=objective, ddim_sampling_eta=eta).to(device)
    return _DIFF[key]


def _row(v, index, device):
    """A tape whose row ``index`` is ``v`` (the rows before it are never read by a single step)."""
    if v is None:
        return None
    tape = torch.zeros((index + 1,) + tuple(v.shape), device=device)
    tape[index] = v.to(device)
    return tape


def _dev(v, device):
    return None if v is None else v.to(device)


def _run(case, d, m, device, fused=True):
    """(new state, history | None, x_start of the library at the case's state | None) of the library on a case."""
    t, tn = S.case_times(case)
    x, obj = d["x"].to(device), d["obj"]
    tables = None if (obj is None or isinstance(obj, cindm_amd.PointObjective)) else obj
    shape = (case.B, case.L, case.F)
    if case.entry == "ddpm":
        dd = _diff(device, m, case.objective)
        desc = dd._desc_for(shape, "mean-inside", case.W - 1, S.CS, S.WINDOW, case.nb)
        tape = cindm_amd.NoiseTape(None, _row(d["z"], t, device), _row(d["rz"], t, device), _row(d["zc"], t, device))
        if obj is None:
            out = dd._run_loop(x.clone(), None, desc, t, t, noise_steps=tape.step, seed=0, sample_offset=0, inpaint_cond=_dev(d["cond"], device),
                               inpaint_noise_steps=tape.cond)
        else:
            out = dd._run_guided_loop(x.clone(), None, desc, obj.descriptor(case.guidance), t, t, noise=tape, seed=0, sample_offset=0,
                                      inpaint_cond=_dev(d["cond"], device), initial_state_overwrite=_dev(d["iso"], device), tables=tables)
        return out, None, None
    dd = _diff(device, m, case.objective, S.DDIM_S, case.eta)
    i = case.step
    tape = cindm_amd.NoiseTape(None, _row(d["z"], i, device), _row(d["rz"], i, device), _row(d["zc"], i, device))
    kw = {}
    if obj is not None:
        kw = dict(n_composed=0, compose_mode="mean-inside", compose_n_bodies=case.nb, design_fn=obj, design_guidance=case.guidance,
                  initial_state_overwrite=_dev(d["iso"], device))
    if case.ms:
        hist = None if i == 0 else (torch.full(shape, float("nan")) if tn < 0 else d["hist"])
        kw.update(solver="dpmpp-2m", history=_dev(hist, device))
    m.set_option("fuse_update", int(fused))
    try:
        out = dd.ddim_sample(shape, _dev(d["cond"], device), noise=tape, init_img=x.clone(), step_range=(i, i + 1), **kw)
        ran_fused = bool(dd.last_step_info()[1])
    finally:
        m.set_option("fuse_update", 1)
    can_fuse = obj is None and case.objective == "pred_noise" and not case.ms and not case.inpaint
    assert ran_fused == (fused and can_fuse), (case.name, fused, ran_fused)
    out, hist = out if case.ms else (out, None)
    x0 = None
    if case.rec <= 1:
        desc = dd._desc_for(shape, None) if obj is None else dd._desc_for(shape, "mean-inside", 0, S.CS, S.WINDOW, case.nb)
        x0 = dd._predict(x, None, t, desc)[1]
    return out, hist, x0


def _hold(case, models, device, fused=True, extra=""):
    m, _ = models[case.frozen]
    d = S.inputs(case)
    t, tn = S.case_times(case)
    E, _ = _unet_outputs((m, None), case.desc(), d["x"], None, t, device)
    row = None
    if case.entry == "ddim":
        dd = _diff(device, m, case.objective, S.DDIM_S, case.eta)
        kap = dd.multistep_kappa()[case.step] if case.ms else torch.zeros(())
        row = torch.cat([dd.ddim_schedule()[1][case.step], kap.reshape(1)])
    st = S.statement(case, d, E, TAB[case.objective], row=row)
    out, hist, x0 = _run(case, d, m, device, fused)
    r, where = S.ratio(out, st["state"])
    tag = case.name + extra
    print(f"{tag}: err/bound {r:.4f} at {where}, clamped {st['clamped']:.3f}")
    _LOG[tag] = {"ratio": round(r, 4), "index": where, "clamped": round(st["clamped"], 3)}
    if hist is not None and x0 is not None:
        assert torch.equal(hist, x0), tag          # the history handed back IS the step's x_start
    if hist is not None:
        assert bool(torch.isfinite(hist).all()), tag
    return [] if r <= EXCEPTIONS.get(tag, 1.0) else [(tag, round(r, 3), where)]


GROUPS = sorted({(c.entry, c.kind or "unguided", c.rec) for c in S.CASES})


def test_frozen_model_ignores_its_input(device, models):
    """Two forwards of the frozen model on different states are bit-equal, and equal to its bias; the other model's are not."""
    g = torch.Generator().manual_seed(8)
    a, b = (torch.randn((18, S.WINDOW, 8), generator=g) * S.X_SCALE for _ in range(2))
    tt = torch.full((18,), 600, device=device)
    fm, fsd = models[True]
    ea, eb = fm(a.to(device), tt).cpu(), fm(b.to(device), tt).cpu()
    assert torch.equal(ea, eb) and torch.equal(ea, fsd["final_conv.1.bias"].view(1, 1, 8).expand(18, S.WINDOW, 8))
    assert len(set(fsd["final_conv.1.bias"].tolist())) == 8
    m, _ = models[False]
    assert not torch.equal(m(a.to(device), tt), m(b.to(device), tt))


@pytest.mark.parametrize("entry,kind,rec", GROUPS, ids=[f"{e}-{k}-r{r}" for e, k, r in GROUPS])
def test_step(device, models, entry, kind, rec):
    """Every case of the grid; the unguided DDIM pairs on the fused route and on compose_update_kernel."""
    cases = [c for c in S.CASES if (c.entry, c.kind or "unguided", c.rec) == (entry, kind, rec)]
    assert cases
    over = []
    for c in cases:
        over += _hold(c, models, device)
        if c.entry == "ddim" and c.kind is None:
            over += _hold(c, models, device, fused=False, extra="-unfused")
    assert not over, over


def test_exceptions_stay_empty():
    assert EXCEPTIONS == {} and R.BOUND_SLACK == 4
