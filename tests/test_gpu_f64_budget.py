"""GPU (MI355X): every U-Net block against the float64 reference of oracle/f64_reference.py, row by row.

The older forward tests compare eps with the fp32 oracle in the whole-tensor norm at 2e-5; the fp32 oracle itself is
about 1e-6 from exact, so they cannot say how accurate a kernel is, and a lost split-fp16 term in one deep layer passes
them (tests/test_f64_reference_host.py).  Here, for every compared row (1-D) or image (2-D) ``r`` and every tap ``T`` the
oracle produces and the handle serves, eps included:

    row_err(gpu, f64)[r]  <=  M * e32(T)

with ``row_err`` = max|a - ref| / max|ref| over the row, ``e32`` the fp32 oracle's own largest ``row_err`` over the compared
rows (computed here, from ``cindm_oracle``), and ``M`` the one constant of f64_reference.py.  The cases are the batch sizes,
time steps, option sets and constructor arguments at which another template instantiation or another plan runs.

All weights are the synthetic ones of ``build_unet`` / ``build_unet2d``, all inputs seeded (SEED_X below).  The float64
reference is evaluated once per (model, rows, t) and shared.  Above 65 rows it is evaluated on a subset of the rows (rows are
independent: test_f64_reference_host.py for the reference, test_unet_rows_are_independent for the library).

With CINDM_F64_BUDGET_JSON=<path> the module writes every case's largest row_err / e32 there when it finishes
(profiles/f64_budget.json is such a run)."""
import json
import os

import pytest
import torch

import cindm_amd
import cindm_oracle as O
import f64_reference as R
from test_gpu_parity_2d import build_unet2d
from test_gpu_paths import PATHS_1D

pytestmark = pytest.mark.gpu

SEED_X = 4100                   # 1-D input of a B-row case: seed SEED_X + B;  2-D: SEED_X2 + t (five images, the first n are used)
SEED_X2 = 5200
NOT_BLOCKS = ("temb", "mid")    # oracle taps that are no block output of their own (time embedding; alias of mid_block2)

# Section 5 of the issue: a (case, tap) whose kernel is honestly less accurate gets its own bound, with the derivation.  None taken.
EXCEPTIONS = {}

# taps every 1-D case must have compared (those of test_unet1d_paths_golden); a handle that serves fewer fails the case
NEED_1D = {"downs.0.1", "downs.0.3", "downs.1.0", "downs.2.1", "downs.3.2", "mid_block1", "mid_attn", "mid_block2", "ups.0.0",
           "ups.0.3", "ups.1.1", "ups.2.2", "ups.2.3"}

_REF = {}
_LOG = {}


def _dump_log(path, log, per_tap_cases, metric="row_err(gpu, f64) / e32(tap); row_err = max|a - ref| / max|ref| per row (1-D) or image (2-D)"):
    """Writes ``log`` (what ``_hold`` collected) as JSON; ``per_tap_cases``: the case-name prefixes listed tap by tap."""
    flat = [(v, case, tap, row) for case, c in log.items() for tap, (v, row) in c["taps"].items()]
    top = sorted(flat, key=lambda q: -q[0])[:10]
    doc = {"metric": metric,
           "M": R.M, "largest": round(top[0][0], 3),
           "ten_largest": [{"ratio": round(v, 3), "case": c, "tap": k, "row": r} for v, c, k, r in top],
           "cases": {case: {"largest": round(max((v for v, _ in c["taps"].values()), default=0.0), 3),
                            "tap": max(c["taps"], key=lambda k: c["taps"][k][0], default=None), "taps_compared": len(c["taps"]),
                            "not_served": c["refused"], "e32_min": float("%.3g" % c["e32"][0]), "e32_max": float("%.3g" % c["e32"][1])}
                     for case, c in log.items()},
           "per_tap": {case: {k: round(v, 3) for k, (v, _) in c["taps"].items()} for case, c in log.items()
                       if case.startswith(per_tap_cases)}}
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


@pytest.fixture(scope="module", autouse=True)
def _write_log():
    yield
    path = os.environ.get("CINDM_F64_BUDGET_JSON")
    if path and _LOG:
        _dump_log(path, _LOG, ("rows-320", "rows-321", "2d-64-n5", "2d-32"))


def _rows_compared(B):
    """All rows up to 65; above: the first 17, the last 17 and every 29th in between."""
    return list(range(B)) if B <= 65 else list(range(17)) + list(range(17, B - 17, 29)) + list(range(B - 17, B))


def _reference(key, fwd32, fwd64, sd, x, t):
    """-> ({tap: float64 reference}, {tap: row_err of the fp32 oracle}), ``eps`` among the taps; computed once per key."""
    if key not in _REF:
        tt = torch.full((x.shape[0],), t, dtype=torch.long)
        t32, t64 = {}, {}
        e32 = fwd32(sd, x, tt, taps=t32)
        e64 = fwd64(sd, x, tt, taps=t64)
        t32["eps"], t64["eps"] = e32, e64
        names = [k for k in t64 if k not in NOT_BLOCKS]
        _REF[key] = ({k: t64[k] for k in names}, {k: R.row_err(t32[k], t64[k]) for k in names})
    return _REF[key]


def _ref1d(mkey, sd, hz, F, B, t):
    x = torch.randn((B, hz, F), generator=torch.Generator().manual_seed(SEED_X + B))
    idx = _rows_compared(B)
    return (x, idx) + _reference((mkey, B, t), O.unet1d_forward, R.unet1d_forward_f64, sd, x[idx], t)


def _ref2d(size, sd, n, t):
    x = torch.randn((5, 21, size, size), generator=torch.Generator().manual_seed(SEED_X2 + t))
    return (x[:n],) + _reference(("2d", size, t), O.unet2d_forward, R.unet2d_forward_f64, sd, x, t)


ULP32 = 2.0 ** -23              # the yardstick is max(e32, one fp32 ulp): no different from e32 wherever the 2e-7 floor below is asserted


def _hold(case, fetch, t64, r32, rows=None, need=(), log=None, exceptions=None, out="eps", below_floor=()):
    """Every tap of ``t64`` that ``fetch`` serves, rows ``rows`` of the reference (default all), against M * max(e32, ULP32).
    ``log`` / ``exceptions``: another module's (tests/test_gpu_f64_budget_force.py); ``out``: the tap that is the model's output;
    ``below_floor``: taps one fp32 operation per element away from a tensor that is compared itself, whose e32 is under an ulp and
    which the floor assertion therefore leaves out."""
    sel = slice(None) if rows is None else slice(0, rows)
    book = _LOG if log is None else log
    log = book[case] = {"taps": {}, "refused": [], "e32": None}
    bad, e32s, floor = [], [], []
    for k, ref in t64.items():
        got = fetch(k)
        if got is None:
            log["refused"].append(k)
            continue
        assert got.shape == ref[sel].shape, (case, k, tuple(got.shape), tuple(ref[sel].shape))
        err = R.row_err(got, ref[sel])
        e32 = float(r32[k][sel].max())
        e32s.append(e32)
        if k not in below_floor:
            floor.append(e32)
        e32 = max(e32, ULP32)
        ratio, row = float(err.max() / e32), int(err.argmax())
        bound = (EXCEPTIONS if exceptions is None else exceptions).get((case, k), R.M)
        log["taps"][k] = (ratio, row)
        print(f"{case:40s} {k:16s} row_err {float(err.max()):.3e}  e32 {e32:.3e}  ratio {ratio:6.3f} (row {row})")
        if not bool(torch.isfinite(err).all()) or not ratio <= bound:
            bad.append((k, ratio, row))
    log["e32"] = (min(e32s), max(e32s))
    assert not bad, (case, bad)
    assert min(floor) > 2e-7, (case, "the reference's own error is too small to be a yardstick at this seed", min(floor))
    missing = set(need) - set(log["taps"])
    assert out in log["taps"] and not missing, (case, "taps not compared", missing)


def _tap_or_none(m, name, n):
    """The handle's own refusals -- no such block output on this plan, or one that lives inside a wider buffer -- mean
    'not served'; any other error is an error."""
    try:
        return m.tap(name, n)
    except cindm_amd.CindmError as e:
        if str(e).startswith("unknown tap") or "tap: strided tensor" in str(e):
            return None
        raise


def _run1d(case, m, mkey, sd, hz, F, B, t, device, need=NEED_1D, equal_without_taps=False):
    x, idx, t64, r32 = _ref1d(mkey, sd, hz, F, B, t)
    xd, tt = x.to(device), torch.full((B,), t, device=device)
    m.set_option("taps", 1)
    try:
        out = m(xd, tt)

        def fetch(k):
            v = out if k == "eps" else _tap_or_none(m, k, B)
            return None if v is None else v[idx].cpu()

        _hold(case, fetch, t64, r32, need=need)
    finally:
        m.set_option("taps", 0)
    if equal_without_taps:          # the sampling configuration (above 320 rows: on the recycled workspace) computes the same eps bit for bit
        assert torch.equal(m(xd, tt), out), case


def _build1d(device, hz, F, dim, mults, att, seed):
    sd = O.synth_state_dict(O.unet1d_param_shapes(hz, F, dim=dim, dim_mults=mults, attention=att), seed=seed)
    m = cindm_amd.TemporalUnet1D(hz, F, False, dim=dim, dim_mults=mults, attention=att)
    m.load_state_dict(sd, strict=True)
    return m.to(device), sd


@pytest.fixture(scope="module")
def unet8(device):
    return _build1d(device, 24, 8, 64, (1, 2, 4, 8), True, 0)


# ------------------------------------------------------------------ 1-D: rows across every selector
# 8 | 9, 16 | 17: the two dconv2 tile sizes (16 samples at L = 3, 8 at L = 6);  33: odd tile counts at both deep levels (no XCD
# re-mapping);  64: tile counts 4 and 8 (re-mapping on at both);  320 | 321: level pairs -> level0_down<2,2> / level1_down<1,2> and the
# recycled workspace;  496 | 497: dresample's 16- -> 32-column form
@pytest.mark.parametrize("B", [1, 8, 9, 16, 17, 33, 64, 65, 320, 321, 496, 497])
def test_rows_default_plan(device, unet8, B):
    m, sd = unet8
    _run1d(f"rows-{B}", m, "default", sd, 24, 8, B, 77, device, equal_without_taps=True)


@pytest.mark.parametrize("t", [0, 999])
def test_time_edges(device, unet8, t):
    m, sd = unet8
    _run1d(f"time-{t}", m, "default", sd, 24, 8, 17, t, device)


# ------------------------------------------------------------------ 1-D: every option set at sizes it has never run at
_PATH_MODEL = {}


@pytest.mark.parametrize("opts,B", [(o, B) for o in PATHS_1D for B in (17, 64, 321)],
                         ids=["-".join(f"{k}={v}" for k, v in o.items()) + f"-{B}" for o in PATHS_1D for B in (17, 64, 321)])
def test_paths(device, opts, B):
    key = json.dumps(opts)
    if key not in _PATH_MODEL:          # (one model alive at a time; the three sizes of an option set follow each other)
        _PATH_MODEL.clear()
        m, sd = _build1d(device, 24, 8, 64, (1, 2, 4, 8), True, 0)
        for k, v in opts.items():
            m.set_option(k, v)
        _PATH_MODEL[key] = (m, sd)
    m, sd = _PATH_MODEL[key]
    _run1d("path-" + "-".join(f"{k}={v}" for k, v in opts.items()) + f"-{B}", m, "default", sd, 24, 8, B, 77, device)
    assert cindm_amd._ffi.lib().cindm_unet1d_status(m._h, None) == 0


# ------------------------------------------------------------------ 1-D: other instantiations
_D = (64, (1, 2, 4, 8))
# (horizon, F, dim, dim_mults, attention, weight seed, refusal).  ``refusal`` None: the library serves the set and every served block is
# held to the budget.  Otherwise (where, message): the one error this set is known to end with -- anything else, and any error of a
# served set, fails the test.
_F_TEXT = "transition_dim must be a multiple of 4"
INSTANCES = (
    # test_unet_variants_golden
    [(24, 4, *_D, True, 1, None), (24, 16, *_D, True, 0, None), (24, 8, *_D, False, 0, None), (44, 8, *_D, True, 0, None),
     (8, 8, *_D, True, 0, None)]
    # test_unet_other_horizons_vs_oracle
    + [(16, 8, *_D, True, 0, None), (32, 8, *_D, True, 0, None), (32, 16, *_D, True, 0, None), (40, 8, *_D, True, 0, None),
       (12, 4, *_D, True, 1, None)]
    # test_unet_other_widths_and_depths
    + [(24, 8, 32, (1, 2, 4, 8), True, 4, None), (24, 8, 64, (1, 2, 4), True, 4, None), (24, 8, 64, (1, 4, 8), False, 4, None),
       (16, 8, 64, (1, 2), True, 4, None),
       (24, 6, 64, (1, 2, 4, 8), True, 4, ("construction", _F_TEXT)), (24, 3, 64, (1, 2, 4, 8), False, 4, ("construction", _F_TEXT)),
       # dim = 128 is no designed refusal: the handle is built and packed, and the first forward comes back with a launch error (a layer
       # shape no kernel is instantiated for).  Kept as the expected outcome, message asserted, so that a change of it is noticed; a
       # refusal with a stated reason at construction is the library's to add.
       (24, 8, 128, (1, 2, 4, 8), True, 4, ("forward", "kernel launch: invalid argument"))])


@pytest.mark.parametrize("hz,F,dim,mults,att,seed,refusal", INSTANCES,
                         ids=[f"h{a}-f{b}-d{c}-m{''.join(map(str, d))}-a{int(e)}" for a, b, c, d, e, _, _ in INSTANCES])
def test_other_instantiations(device, hz, F, dim, mults, att, seed, refusal):
    """Constructor arguments that select other kernels: what the library computes is held to the budget, at least eps, both
    blocks of the bottleneck and the first block of every level on the way down and up."""
    tag = f"inst-h{hz}-f{F}-d{dim}-m{''.join(map(str, mults))}-a{int(att)}"
    if refusal and refusal[0] == "construction":
        with pytest.raises(cindm_amd.CindmError, match=refusal[1]):
            _build1d(device, hz, F, dim, mults, att, seed)
        return
    m, sd = _build1d(device, hz, F, dim, mults, att, seed)
    if refusal:
        with pytest.raises(cindm_amd.CindmError, match=refusal[1]):
            m(torch.zeros((1, hz, F), device=device), 0)
        return
    need = {f"downs.{i}.0" for i in range(len(mults))} | {f"ups.{j}.0" for j in range(len(mults) - 1)} | {"mid_block1", "mid_block2"}
    for B in (9, 17):
        _run1d(f"{tag}-{B}", m, tag, sd, hz, F, B, 611, device, need=need)


# ------------------------------------------------------------------ 2-D
@pytest.fixture(scope="module")
def unet2d(device):
    return build_unet2d(device)


def _run2d(case, m, sd, size, n, t, device):
    x, t64, r32 = _ref2d(size, sd, n, t)
    out = m(x.to(device), t)
    _hold(case, lambda k: (out if k == "eps" else m.tap(k, n)).cpu(), t64, r32, rows=n)
    assert len(_LOG[case]["taps"]) == 22          # the 21 block outputs and eps: the 2-D handle serves them all


@pytest.mark.parametrize("t", [0, 500, 999])
@pytest.mark.parametrize("n", [1, 2, 3, 5])
def test_unet2d_images_and_times(device, unet2d, n, t):
    m, sd = unet2d
    _run2d(f"2d-64-n{n}-t{t}", m, sd, 64, n, t, device)


def test_unet2d_image_size_32(device):
    m, sd = build_unet2d(device, image_size=32, seed=3)
    _run2d("2d-32-n2-t500", m, sd, 32, 2, 500, device)


@pytest.mark.parametrize("opts", [{"mfma_f32": 1}, {"la_site": 0}, {"conv_ws": 0}, {"ws_alias": 0}, {"tail_h3": 0},
                                  {"ws_nosplit": 0}, {"ws_nosplit": 1}, {"la_wpi": 4, "la_nsplit": 4}],
                         ids=["mfma_f32", "la_site0", "conv_ws_0", "ws_alias_0", "tail_h3_0", "ws_kgroups", "ws_nosplit_all", "la_4_per_image"])
def test_unet2d_paths(device, opts):
    """The eight option sets of test_unet2d_paths_golden, three images."""
    m, sd = build_unet2d(device)
    for k, v in opts.items():
        m.set_option(k, v)
    _run2d("2d-path-" + "-".join(f"{k}={v}" for k, v in opts.items()), m, sd, 64, 3, 500, device)
