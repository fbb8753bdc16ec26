"""GPU (MI355X): the launch plan of TemporalUnet1D's forward -- which kernels `emit_forward` (csrc/unet1d_host.inc) emits, on which
grids, from which workspace -- against a recorded plan, tests/golden/unet1d_plan.json.

Per case the record holds `launches_per_forward`, `cindm_unet1d_workspace_bytes`, the `profile_detail` sequence of (kind, grid x,
grid y, stages, flops), with taps = 1 the tap names and shapes reachable after a forward, and `last_step_info()` after a 3-step
`p_sample_loop`, captured and eager (`ddpm_chain`): integers, names and host-computed doubles only, so the record does not depend on the box and
every comparison is equality.  It pins what a host-side change must not move: the level kernels and their pairs serving or not, the
`<1>` / `<2>` and `MINB = 2` instantiations (grids), the workspace recycling above 320 rows, and every option's alternative path.

Cases: synthetic weights, dim 64, timesteps 8 -- the smallest shapes at which each branch of the emitter can still go wrong:
horizon 24 with dim_mults (1, 2, 4, 8) (all four level kernels and both pairs; level 0 has L > 16), horizon 16 (L <= 16), dim_mults
(1, 2, 4) (ups_last serves, ups_tail cannot), attention off (no level kernel serves), F = 4 (the multibody second model's width);
rows 1, 3, 320 and 321 (321: the pairs switch off, two workgroups per CU, "ws_alias" = 1 starts recycling); and for the first
configuration every alternative option value, one at a time, at rows 3 and 321.

The record is written by tests/manual/make_golden_unet1d_plan.py (which runs `record_setting` below):
    python tests/manual/make_golden_unet1d_plan.py
A change that moves the plan ON PURPOSE regenerates the record with the new library, so that the move shows in review as the
record's diff; a host-only refactor regenerates nothing (its record comes from the commit before it)."""
import json
import os

import pytest
import torch

import cindm_amd
from cindm_amd import _ffi
from cindm_amd.synthetic import synthetic_init_

gpu = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "unet1d_plan.json")
T = 8
# id: (horizon, transition_dim, dim_mults, attention)
CONFIGS = {
    "hz24-F8": (24, 8, (1, 2, 4, 8), True),
    "hz16-F8": (16, 8, (1, 2, 4, 8), True),
    "hz24-F8-mults124": (24, 8, (1, 2, 4), True),
    "hz24-F8-noattn": (24, 8, (1, 2, 4, 8), False),
    "hz24-F4": (24, 4, (1, 2, 4, 8), True),
}
ROWS = (1, 3, 320, 321)
FIRST = "hz24-F8"
SETTINGS = [("level_pairs", 0), ("level1", 0), ("level1", 2), ("level0", 0), ("ups_last", 0), ("ups_tail", 0), ("attn_site", 0),
            ("local_gn", 0), ("dconv2", 0), ("dconv", 0), ("attn_head", 0), ("dresample", 0), ("dresample", 1), ("ws_alias", 0),
            ("ws_alias", 2), ("no_exchange", 1), ("mfma_f32", 1), ("taps", 1)]
SETTING_ROWS = (3, 321)
# (configuration, option or None, value, row counts)
CASES = [(c, None, 0, ROWS) for c in CONFIGS] + [(FIRST, k, v, SETTING_ROWS) for k, v in SETTINGS]
# every name cindm_unet1d_tap may know: the blocks of each level, the middle blocks and the head's pre-activation
TAP_NAMES = [f"{side}.{i}.{j}" for side in ("downs", "ups") for i in range(4) for j in range(4)] + \
            ["mid_block1", "mid_attn", "mid_block2", "final_conv.0.pre"]


def case_id(config, key, value):
    return config if key is None else f"{config}/{key}={value}"


_models = {}


def model(config, device):
    """One model and one diffusion object per configuration for the whole module (synthetic weights, seed 0)."""
    if config not in _models:
        hz, F, mults, att = CONFIGS[config]
        m = synthetic_init_(cindm_amd.TemporalUnet1D(hz, F, False, dim=64, dim_mults=mults, attention=att, timesteps=T)).to(device)
        d = cindm_amd.GaussianDiffusion1D(m, image_size=hz, conditioned_steps=0, timesteps=T).to(device)
        _models[config] = (m, d)
    return _models[config]


def ddpm_chain(d, rows, graph, seed=1):
    """Three DDPM steps of `rows` designs: `p_sample_loop`; for a one-body model (F = 4), which `p_sample_loop`'s composition
    descriptor refuses, the same library chain on the plain descriptor."""
    m = d.model
    shape = (rows, m.horizon, m.transition_dim)
    if m.transition_dim == 8:
        return d.p_sample_loop(shape, None, n_composed=0, seed=seed, use_graph=graph, t_stop=T - 3)
    img = d._init_state(shape, d.betas.device, None, seed, 0, T)
    return d._run_loop(img, None, d._desc_for(shape), T - 1, T - 3, noise_steps=None, seed=seed, sample_offset=0, inpaint_cond=None,
                       inpaint_noise_steps=None, use_graph=graph)


def _plan(m, d, rows, device):
    hz, F = m.horizon, m.transition_dim
    x = torch.zeros((rows, hz, F), device=device)
    m.sync_weights()
    rec = {"launches": int(m.launches_per_forward),
           "workspace_bytes": int(_ffi.lib().cindm_unet1d_workspace_bytes(m._h, rows)),
           "profile": [[kind, gx, gy, stages, flops] for kind, _, flops, gx, gy, stages in m.profile_detail(x, T - 1)],
           "step_info": {}}
    for name, graph in (("graph", True), ("eager", False)):
        ddpm_chain(d, rows, graph)
        n, fused = d.last_step_info()
        rec["step_info"][name] = [n, int(fused)]
    return rec


def _taps(m, rows, device):
    hz, F = m.horizon, m.transition_dim
    m(torch.zeros((rows, hz, F), device=device), T - 1)
    out = {}
    for name in TAP_NAMES:
        try:
            out[name] = list(m.tap(name, rows).shape)
        except _ffi.CindmError:
            pass
    return out


def record_setting(config, key, value, rows_list, device):
    """{str(rows): record} of one case; the model's options are back at what they were afterwards."""
    m, d = model(config, device)
    keep = {k: m._option(k) for k in ("taps",) + ((key,) if key else ())}
    out = {}
    try:
        if key:
            m.set_option(key, value)
        for rows in rows_list:
            out[str(rows)] = _plan(m, d, rows, device)
        m.set_option("taps", 1)
        for rows in rows_list:
            out[str(rows)]["taps"] = _taps(m, rows, device)
    finally:
        for k, v in keep.items():
            m.set_option(k, v)
    return out


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_golden_covers_every_case(golden):
    """The record has exactly this module's cases and row counts (no GPU: a case added here without its record fails at once)."""
    assert sorted(golden) == sorted(case_id(c, k, v) for c, k, v, _ in CASES)
    for c, k, v, rows in CASES:
        assert sorted(golden[case_id(c, k, v)]) == sorted(str(r) for r in rows), case_id(c, k, v)


@gpu
@pytest.mark.parametrize("config,key,value,rows", CASES, ids=[case_id(c, k, v) for c, k, v, _ in CASES])
def test_plan_equals_record(device, golden, config, key, value, rows):
    got = json.loads(json.dumps(record_setting(config, key, value, rows, device)))      # (through JSON: lists, string keys)
    want = golden[case_id(config, key, value)]
    for r in map(str, rows):
        for field in ("launches", "workspace_bytes", "step_info", "taps", "profile"):
            assert got[r][field] == want[r][field], (case_id(config, key, value), r, field)
