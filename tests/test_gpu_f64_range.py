"""GPU (MI355X): the edges of the split-fp16 range rule, held to the float64 row budget of tests/test_gpu_f64_budget.py.

The rule (``max_abs_in_fp16_window``, csrc/handle_core.inc) keeps a checkpoint on the split-fp16 kernels while every inspected tensor
has 2^-12 <= max|w| <= 2^15; tests/test_gpu_range.py checks it at scales well inside and well outside, against the fp32 oracle in the
whole-tensor norm at 2e-5.  Here the cases of tests/range_cases.py put tensors EXACTLY on an edge (the planes' hardest inputs: at
2^-12 a quarter of the hi plane and most of the lo plane are fp16 subnormals) and one fp32 number beyond it (the rule's comparison
and coverage), and every case asserts

  * ``range_fallback`` reads what the table states,
  * every served tap, row by row (1-D) or image by image: row_err(gpu, f64) <= M * max(e32(tap), 2^-23),
  * every output is finite,
  * the ``need`` set of taps was compared (2-D, ForceUnet: all of them; ForceUnet: activations and gradients).

``M``, ``row_err`` and ``e32`` are those of oracle/f64_reference.py; ``_hold`` does the comparison.  tests/test_f64_range_host.py runs
the same cases on the CPU first: the yardsticks are finite and above the 2e-7 floor except at the taps pinned in
``range_cases.BELOW_FLOOR``, and flushed subnormal planes sit above 10 x M x e32.

Measured on an MI355X (profiles/f64_range.json): fp16 subnormals survive pack, staging and MFMA -- lower edge 1.56 (1-D), 1.02
(2-D), 2.05 (ForceUnet, a gradient tap); upper edge 1.42 / 0.94 / 3.14; every option set that stages weight planes differently
<= 1.56.  The ws-tiny cases hold the budget with and without the rule on the folded tensors (the GroupNorm behind a folded-tiny
convolution hands on little more than its bias), so what they pin is ``range_fallback`` = 1.  The largest ratio of the module, 7.18
(force-ws-tiny, 3 images, the gradient at downs.3.2), is neither edge's: the odd image count's exact-fp32 3 x 3 convolutions at the
8 x 8 level (4.33 at unit scale, f64_reference.py), against a yardstick this nearly image-independent model shrinks to 3.6e-7; it
reads 7.59 with the folded-tensor check taken out.

With CINDM_F64_RANGE_JSON=<path> the module writes every case's largest ratio there (profiles/f64_range.json is such a run)."""
import os

import pytest
import torch

import cindm_amd
import cindm_oracle as O
import f64_reference as R
import range_cases as C
from test_gpu_f64_budget import NEED_1D, NOT_BLOCKS, _build1d, _dump_log, _hold, _tap_or_none
from test_gpu_f64_budget_force import _flat

pytestmark = pytest.mark.gpu

# An edge case that cannot hold M belongs on the fp32 side of the rule, not here.  None taken.
EXCEPTIONS = {}

_LOG = {}
_REF = {}


@pytest.fixture(scope="module", autouse=True)
def _write_log():
    yield
    path = os.environ.get("CINDM_F64_RANGE_JSON")
    if path and _LOG:
        _dump_log(path, _LOG, ("1d-lo-in", "1d-hi-in", "1d-all-ruled-lo", "2d-lo-in", "2d-hi-in", "2d-ws-tiny", "force-"),
                  metric="row_err(gpu, f64) / max(e32(tap), 2^-23); row_err = max|a - ref| / max|ref| per row (1-D) or image (2-D, ForceUnet)")


def _oid(o):
    return "-".join(f"{k}={v}" for k, v in o.items())


def _finite(*tensors):
    return all(bool(torch.isfinite(v).all()) for v in tensors)


# ------------------------------------------------------------------ 1-D
def _ref1d(case, B):
    """-> (sd, x, compared rows, float64 taps, row_err of the fp32 oracle), once per (case, rows)."""
    if (case, B) not in _REF:
        mk, _, _, amp, *seed = C.CASES_1D[case]
        sd, x, idx = mk(), C.input_1d(B, amp, *seed), C.rows_compared(B)
        tt = torch.full((len(idx),), C.T_1D, dtype=torch.long)
        t32, t64 = {}, {}
        t32["eps"], t64["eps"] = O.unet1d_forward(sd, x[idx], tt, taps=t32), R.unet1d_forward_f64(sd, x[idx], tt, taps=t64)
        names = [k for k in t64 if k not in NOT_BLOCKS]
        _REF[(case, B)] = (sd, x, idx, {k: t64[k] for k in names}, {k: R.row_err(t32[k], t64[k]) for k in names})
    return _REF[(case, B)]


def _model1d(device, sd, opts=None):
    m = cindm_amd.TemporalUnet1D(24, 8, False, attention=True)
    m.load_state_dict(sd, strict=True)
    m = m.to(device)
    for k, v in (opts or {}).items():
        m.set_option(k, v)
    return m


def _run1d(device, case, tag, m, B):
    _, x, idx, t64, r32 = _ref1d(case, B)
    xd, tt = x.to(device), torch.full((B,), C.T_1D, device=device)
    m.set_option("taps", 1)
    try:
        out = m(xd, tt)
        assert _finite(out), tag

        def fetch(k):
            v = out if k == "eps" else _tap_or_none(m, k, B)
            assert v is None or _finite(v), (tag, k)
            return None if v is None else v[idx].cpu()

        _hold(tag, fetch, t64, r32, need=NEED_1D, log=_LOG, exceptions=EXCEPTIONS, below_floor=C.BELOW_FLOOR.get(case, ()))
    finally:
        m.set_option("taps", 0)
    assert m.get_option("range_fallback") == C.CASES_1D[case][2], (tag, m.get_option("range_fallback"))
    assert cindm_amd._ffi.lib().cindm_unet1d_status(m._h, None) == 0


@pytest.mark.parametrize("case", list(C.CASES_1D))
def test_unet1d_cases(device, case):
    """Every row of range_cases.CASES_1D at each of its sizes: 9 | 17 the two dconv2 tile sizes, 321 the level pairs and the recycled
    workspace, 5 the size of tests/test_gpu_range.py."""
    m = _model1d(device, _ref1d(case, C.CASES_1D[case][1][0])[0])
    assert m.get_option("range_fallback") == C.CASES_1D[case][2], case            # decided at finalize, before any forward
    for B in C.CASES_1D[case][1]:
        _run1d(device, case, f"{case}-{B}", m, B)


@pytest.mark.parametrize("opts", C.OPTIONS_1D, ids=[_oid(o) for o in C.OPTIONS_1D])
def test_unet1d_lower_edge_under_options(device, opts):
    """The option sets that change which kernel stages weight planes, at the lower edge."""
    m = _model1d(device, _ref1d("1d-lo-in", 17)[0], opts)
    for k, v in opts.items():
        assert m.get_option(k) == v
    _run1d(device, "1d-lo-in", f"1d-lo-in-{_oid(opts)}-17", m, 17)


def test_build1d_is_the_unit_scale_model(device):
    """The cases move tensors of the model of tests/test_gpu_f64_budget.py (``_build1d``, weight seed 0): same keys, same values elsewhere."""
    m, sd = _build1d(device, 24, 8, 64, (1, 2, 4, 8), True, 0)
    lo = C.CASES_1D["1d-lo-in"][0]()
    edge = set(C.gauge_1d(sd)) | {"final_conv.1.weight"}
    assert set(lo) == set(sd) and m.get_option("range_fallback") == 0
    for k, v in sd.items():
        if k in edge:
            assert float(lo[k].abs().max()) == C.LO
        elif not (k.endswith(".bias") and k[:-5] + ".weight" in edge):
            assert torch.equal(lo[k], v), k


# ------------------------------------------------------------------ 2-D
def _ref2d(case):
    if case not in _REF:
        mk, size, _ = C.CASES_2D[case]
        sd, x = mk(), C.input_2d(size)
        tt = torch.full((x.shape[0],), C.T_2D, dtype=torch.long)
        t32, t64 = {}, {}
        t32["eps"], t64["eps"] = O.unet2d_forward(sd, x, tt, taps=t32), R.unet2d_forward_f64(sd, x, tt, taps=t64)
        _REF[case] = (sd, x, t64, {k: R.row_err(t32[k], t64[k]) for k in t64})
    return _REF[case]


def _run2d(device, case, tag, opts=None):
    sd, x, t64, r32 = _ref2d(case)
    m = cindm_amd.Unet(dim=64, dim_mults=(1, 2), channels=21, image_size=C.CASES_2D[case][1])
    m.load_state_dict(sd, strict=True)
    m = m.to(device)
    for k, v in (opts or {}).items():
        m.set_option(k, v)
    n = x.shape[0]
    out = m(x.to(device), C.T_2D)
    assert _finite(out), tag

    def fetch(k):
        v = out if k == "eps" else m.tap(k, n)
        assert _finite(v), (tag, k)
        return v.cpu()

    _hold(tag, fetch, t64, r32, need=set(t64), log=_LOG, exceptions=EXCEPTIONS, below_floor=C.BELOW_FLOOR.get(case, ()))
    assert len(_LOG[tag]["taps"]) == 22 and not _LOG[tag]["refused"]          # the 21 block outputs and eps
    assert m.get_option("range_fallback") == C.CASES_2D[case][2], (tag, m.get_option("range_fallback"))
    return m


@pytest.mark.parametrize("case", list(C.CASES_2D))
def test_unet2d_cases(device, case):
    """range_cases.CASES_2D.  2d-ws-tiny: the weight-standardised tensors fold to a maximum of 5e-7 .. 9e-7, outside the window; the
    rule looks at the folded tensors and the handle runs on the fp32 kernels (range_fallback 1)."""
    _run2d(device, case, case)


@pytest.mark.parametrize("opts", C.OPTIONS_2D, ids=[_oid(o) for o in C.OPTIONS_2D])
def test_unet2d_lower_edge_under_options(device, opts):
    m = _run2d(device, "2d-lo-in-32", f"2d-lo-in-32-{_oid(opts)}", opts)
    for k, v in opts.items():
        assert m.get_option(k) == v


# ------------------------------------------------------------------ ForceUnet: activations and gradients at every block boundary
def _refforce(case):
    if case not in _REF:
        sd, x = C.CASES_FORCE[case][0](), C.input_force()
        runs = [[_flat(f(sd, x[i:i + 1], C.LAMBDA_FORCE)) for i in range(x.shape[0])] for f in (R.force_unet_blocks, R.force_unet_f64)]      # each image alone
        f32, f64 = ({k: torch.cat([r[k] for r in run]) for k in run[0]} for run in runs)
        out = f64["out"]
        assert float((out[:, 0].abs() / out.abs().max()).min()) >= 1e-3, "the sign of |out0| is in question at this seed"
        _REF[case] = (sd, x, f64, {k: R.row_err(f32[k], f64[k]) for k in f64})
    return _REF[case]


_FORCE_MODEL = {}


@pytest.mark.parametrize("case,n", [(c, n) for c in C.CASES_FORCE for n in C.IMAGES_FORCE], ids=[f"{c}-n{n}" for c in C.CASES_FORCE for n in C.IMAGES_FORCE])
def test_forceunet_cases(device, case, n):
    """range_cases.CASES_FORCE at 2 images (paired at the 8 x 8 level) and 3 (the odd count's fp32 convolutions there).  The input-gradient
    pass reuses the weight planes: its taps are held to the same budget."""
    sd, x, t64, r32 = _refforce(case)
    if case not in _FORCE_MODEL:            # (one model alive at a time; the two image counts of a case follow each other)
        _FORCE_MODEL.clear()
        m = cindm_amd.ForceUnet(dim=64, dim_mults=(1, 2, 4, 8), channels=4)
        m.load_state_dict(sd, strict=True)
        _FORCE_MODEL[case] = m.to(device)
    m = _FORCE_MODEL[case]
    assert m.get_option("range_fallback") == C.CASES_FORCE[case][1], (case, m.get_option("range_fallback"))
    tag = f"{case}-n{n}"
    assert len(t64) == 42
    m.set_option("taps", 1)
    try:
        out, dx = m.input_grad(x[:n].to(device), lambda_force=C.LAMBDA_FORCE)
        assert _finite(out, dx), tag

        def fetch(k):
            v = out if k == "out" else dx if k == "dx" else m.tap(k[5:], n, grad=True) if k.startswith("grad:") else m.tap(k, n)
            assert _finite(v), (tag, k)
            return v.cpu()

        _hold(tag, fetch, t64, r32, rows=n, need=set(t64), log=_LOG, exceptions=EXCEPTIONS, out="out",
              below_floor=C.BELOW_FLOOR_FORCE + C.DEGENERATE.get(case, ()))
        assert len(_LOG[tag]["taps"]) == 42 and not _LOG[tag]["refused"]
    finally:
        m.set_option("taps", 0)
    assert m.get_option("range_fallback") == C.CASES_FORCE[case][1]


def test_exceptions_stay_empty():
    assert EXCEPTIONS == {} and R.M == 8
