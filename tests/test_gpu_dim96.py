"""GPU (MI355X): TemporalUnet1D at dim = 96 -- the reference's `--Unet_dim 96` checkpoint, whose GroupNorm(8, C) groups are 12, 24,
48 and 96 channels wide: neither inside one 32-column tile nor made of whole tiles, so the convolution kernels keep the group
statistics per segment of gcd(gw, 32) channels (csrc/kernels.h, the G3 instantiations).

1. every served block against the float64 reference, row by row, at the bound M of oracle/f64_reference.py (the helpers, seeds and
   time step of tests/test_gpu_f64_budget.py);
2. the whole output tensor against the fp32 oracle, and independence of the rows;
3. sampling chains at horizon 44 against the oracle's loops;
4. a checkpoint file loaded through Trainer.load.

Shapes of 1.: horizon 44 gives levels of L = 44, 22, 11, 11 with 1, 2, 4, 4 samples per 48-row tile, horizon 24 gives L = 24, 12, 6, 3
with 2 ... 16; with the ragged last tiles of B = 9 / 17 / 65 these are the smallest at which the segment indexing, the three-partial
merge and the per-sample table can go wrong at all four group widths.

The fp32 oracle's own error (the yardstick's floor, > 2e-7 at every compared tap) was checked on the CPU for every case below with
weight seed 4: the smallest is 2.53e-7 (horizon 44, B = 9); B = 65: 3.33e-7, the compared rows of B = 321: 3.49e-7.

With CINDM_F64_BUDGET_DIM96_JSON=<path> the module writes every case's largest row_err / e32 there when it finishes
(profiles/f64_budget_dim96.json is such a run)."""
import os

import pytest
import torch

import cindm_amd
import cindm_oracle as O
from test_gpu_f64_budget import _LOG, SEED_X, _build1d, _dump_log, _run1d
from test_gpu_parity import TOL_CHAIN, TOL_FWD, TOL_STEP, rel

pytestmark = pytest.mark.gpu

T_BLOCKS = 611
SEED_W = 4
# (horizon, F, dim_mults, attention)
MODELS = {"h44": (44, 8, (1, 2, 4, 8), True), "h24": (24, 8, (1, 2, 4, 8), True), "h16m12": (16, 8, (1, 2), True),
          "h24f4": (24, 4, (1, 2, 4, 8), False)}
# (the first model last: the tests below the block cases go on with it)
BLOCK_CASES = [("h24", 9), ("h24", 17), ("h16m12", 9), ("h16m12", 17), ("h24f4", 9), ("h24f4", 17), ("h44", 9), ("h44", 17), ("h44", 65)]

_MODEL = {}


def _model(device, name, **opts):
    """One model alive at a time (the cases of a model follow each other)."""
    key = (name, tuple(sorted(opts.items())))
    if key not in _MODEL:
        _MODEL.clear()
        hz, F, mults, att = MODELS[name]
        m, sd = _build1d(device, hz, F, 96, mults, att, SEED_W)
        for k, v in opts.items():
            m.set_option(k, v)
        _MODEL[key] = (m, sd)
    return _MODEL[key]


def _need(mults):
    return {f"downs.{i}.0" for i in range(len(mults))} | {f"ups.{j}.0" for j in range(len(mults) - 1)} | {"mid_block1", "mid_block2"}


@pytest.fixture(scope="module", autouse=True)
def _write_log():
    yield
    _MODEL.clear()
    path = os.environ.get("CINDM_F64_BUDGET_DIM96_JSON")
    log = {k: v for k, v in _LOG.items() if k.startswith("dim96-")}
    if path and log:
        _dump_log(path, log, ("dim96-h44-17", "dim96-h44-mfma_f32-17"))


# ------------------------------------------------------------------ 1. blocks against float64
@pytest.mark.parametrize("name,B", BLOCK_CASES, ids=[f"{n}-{B}" for n, B in BLOCK_CASES])
def test_blocks_f64(device, name, B):
    hz, F, mults, _ = MODELS[name]
    m, sd = _model(device, name)
    _run1d(f"dim96-{name}-{B}", m, "dim96-" + name, sd, hz, F, B, T_BLOCKS, device, need=_need(mults))
    assert m.get_option("range_fallback") == 0


def test_blocks_f64_recycled_workspace(device):
    """Above 320 rows the sampling configuration runs on the recycled workspace: the same eps bit for bit with and without taps."""
    hz, F, mults, _ = MODELS["h44"]
    m, sd = _model(device, "h44")
    _run1d("dim96-h44-321", m, "dim96-h44", sd, hz, F, 321, T_BLOCKS, device, need=_need(mults), equal_without_taps=True)


# ------------------------------------------------------------------ 2. whole tensor
def test_forward_vs_oracle(device):
    hz, F, _, _ = MODELS["h44"]
    m, sd = _model(device, "h44")
    x = torch.randn((17, hz, F), generator=torch.Generator().manual_seed(SEED_X + 17))
    ref = O.unet1d_forward(sd, x, torch.full((17,), T_BLOCKS, dtype=torch.long))
    out = m(x.to(device), torch.full((17,), T_BLOCKS, device=device))
    assert rel(out, ref) < TOL_FWD
    assert m.launches_per_forward > 0


def test_rows_are_independent(device):
    """A sample's result does not depend on its batch mates, whichever tile and segment table it lands in."""
    hz, F, _, _ = MODELS["h44"]
    m, _ = _model(device, "h44")
    x = torch.randn((50, hz, F), generator=torch.Generator().manual_seed(5)).to(device)
    tt = torch.full((50,), 400, device=device)
    full = m(x, tt)
    part = m(x[37:40].contiguous(), tt[:3])
    assert torch.equal(full[37:40], part)
    assert torch.equal(full, m(x, tt))            # and launches are deterministic


# ------------------------------------------------------------------ 3. chains (horizon 44, F = 8, B = 5)
B_CHAIN = 5


def _diffusion(device, S=1000, eta=0.0):
    m, sd = _model(device, "h44")
    d = cindm_amd.GaussianDiffusion1D(m, image_size=44, conditioned_steps=0, timesteps=1000, sampling_timesteps=S, loss_type="l1",
                                      ddim_sampling_eta=eta).to(device)
    return d, O.Diffusion1D(sd, image_size=44, conditioned_steps=0), m


def _healthy(m):
    assert cindm_amd._ffi.lib().cindm_unet1d_status(m._h, None) == 0
    assert m.get_option("range_fallback") == 0


def test_chain_ddpm(device):
    """Plain DDPM chain, its last 8 steps, explicit noise."""
    d, od, m = _diffusion(device)
    tape = O.NoiseTape.make(1296, (B_CHAIN, 44, 8), 1000)
    ref = O.sample(od, B_CHAIN, tape, n_composed=0, compose_n_bodies=2, t_stop=992)
    out = d.sample(batch_size=B_CHAIN, cond=None, n_composed=0, compose_n_bodies=2, noise=cindm_amd.NoiseTape(tape.init, tape.step), t_stop=992)
    assert tuple(out.shape) == (B_CHAIN, 44, 8) and rel(out, ref) < TOL_CHAIN
    _healthy(m)


def test_chain_ddim(device):
    """Unguided DDIM, S = 10 (eta = 0.5: the step noise is used), against the oracle's ddim_sample; graph replay == stream launches."""
    from test_oracle_golden import ddim_tape
    d, od, m = _diffusion(device, S=10, eta=0.5)
    tp = ddim_tape(1297, (B_CHAIN, 44, 8), 10)
    ref = O.ddim_sample(od, (B_CHAIN, 44, 8), None, tp, sampling_timesteps=10, eta=0.5, n_composed=0, compose_n_bodies=2)
    out = d.sample(batch_size=B_CHAIN, cond=None, noise=cindm_amd.NoiseTape(tp["init"], tp["step"]), n_composed=0, compose_n_bodies=2)
    assert tuple(out.shape) == (B_CHAIN, 44, 8) and rel(out, ref) < TOL_CHAIN
    a = d.sample(batch_size=B_CHAIN, n_composed=0, seed=7)
    b = d.sample(batch_size=B_CHAIN, n_composed=0, seed=7, use_graph=False)
    assert torch.equal(a, b) and bool(torch.isfinite(a).all())
    _healthy(m)


def test_guided_step(device):
    """One reverse step (t = 999) guided by the built-in point objective under standard-recurrence-2, against the oracle
    differentiating the same objective with autograd."""
    d, od, m = _diffusion(device)
    obj = cindm_amd.PointObjective([0.25, -0.5], 2, coef=20.0, design_fn_mode="L2")
    tape = O.NoiseTape.make(1298, (B_CHAIN, 44, 8), 1000, recur=2)
    kw = dict(n_composed=0, compose_mode="mean-inside", design_fn=obj, design_guidance="standard-recurrence-2", t_stop=999)
    ref = O.sample(od, B_CHAIN, tape, **kw)
    out = d.sample(batch_size=B_CHAIN, noise=cindm_amd.NoiseTape(tape.init, tape.step, tape.recur), **kw)
    assert rel(out, ref) < TOL_STEP
    _healthy(m)


# ------------------------------------------------------------------ 4. checkpoint
def test_checkpoint_through_trainer_load(device, tmp_path):
    """{"step", "model": diffusion.state_dict()} written as a training run would, read by Trainer.load into a fresh dim-96 model: its
    forward is the directly loaded model's, bit for bit."""
    hz, F, mults, att = MODELS["h44"]
    direct, _ = _model(device, "h44")
    src = cindm_amd.GaussianDiffusion1D(direct, image_size=hz, conditioned_steps=0, timesteps=1000, sampling_timesteps=1000, loss_type="l1")
    torch.save({"step": 5000, "model": {k: v.detach().cpu() for k, v in src.state_dict().items()}, "version": "1.0"}, str(tmp_path / "model-5.pt"))
    fresh = cindm_amd.TemporalUnet1D(hz, F, False, dim=96, dim_mults=mults, attention=att)
    d = cindm_amd.GaussianDiffusion1D(fresh, image_size=hz, conditioned_steps=0, timesteps=1000, sampling_timesteps=1000, loss_type="l1")
    tr = cindm_amd.Trainer(d, None, results_folder=str(tmp_path), train_batch_size=1).load(5)
    assert tr.step == 5000
    d = d.to(device)
    x = torch.randn((7, hz, F), generator=torch.Generator().manual_seed(SEED_X + 7)).to(device)
    tt = torch.full((7,), 300, device=device)
    assert torch.equal(fresh(x, tt), direct(x, tt))


# ------------------------------------------------------------------ the fp32-MFMA plan (last: it builds its own model)
def test_blocks_f64_mfma_f32(device):
    """The exact fp32-MFMA kernels (what the range rule escalates to) serve the width too."""
    hz, F, mults, _ = MODELS["h44"]
    m, sd = _model(device, "h44", mfma_f32=1)
    _run1d("dim96-h44-mfma_f32-17", m, "dim96-h44", sd, hz, F, 17, T_BLOCKS, device, need=_need(mults))
    assert cindm_amd._ffi.lib().cindm_unet1d_status(m._h, None) == 0
