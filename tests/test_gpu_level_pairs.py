"""GPU (MI355X): the fused level pairs (option "level_pairs": level01_down_kernel = level0_down + level1_down, ups_tail_last_kernel =
ups_tail128 + ups_last, one launch each up to 320 rows) against the stand-alone launches of the same stages.  The fused kernels run the
stand-alone kernels' code on the same fp32 values (the hand-over tile stays in registers instead of going through memory), so every
comparison is bitwise: torch.equal between the option on and off.  The host half (the key's default and round trip) needs no GPU."""
import ctypes as C

import pytest
import torch

import cindm_amd
import cindm_oracle as O
from cindm_amd import _ffi

gpu = pytest.mark.gpu

TAPS = ["downs.0.0", "downs.0.1", "downs.0.2", "downs.0.3", "downs.1.0", "downs.1.1", "downs.1.2", "downs.1.3", "downs.2.1", "mid_block2",
        "ups.0.3", "ups.1.0", "ups.1.1", "ups.1.2", "ups.1.3", "ups.2.0", "ups.2.1", "ups.2.2", "ups.2.3", "final_conv.0.pre"]


def _unet(device, hz=24, F=8, seed=3):
    sd = O.synth_state_dict(O.unet1d_param_shapes(hz, F, attention=True), seed=seed)
    m = cindm_amd.TemporalUnet1D(hz, F, False, dim=64, dim_mults=(1, 2, 4, 8), attention=True)
    m.load_state_dict(sd, strict=True)
    return m.to(device)


def _diffusion(m, device, hz=24, **kw):
    return cindm_amd.GaussianDiffusion1D(m, image_size=hz, conditioned_steps=0, timesteps=1000,
                                         sampling_timesteps=kw.pop("sampling_timesteps", 1000), **kw).to(device)


def _on_off(m, fn):
    """fn() with the pairs fused and with the stand-alone launches; the option is back at its default afterwards."""
    out = {}
    try:
        for v in (1, 0):
            m.set_option("level_pairs", v)
            out[v] = fn()
    finally:
        m.set_option("level_pairs", 1)
    return out[1], out[0]


def test_level_pairs_option_round_trip(monkeypatch):
    """The key exists on the 1-D handle with default 1 and reads back what was written (the library's own entry points: no device)."""
    monkeypatch.delenv("CINDM_LEVEL_PAIRS", raising=False)
    m = cindm_amd.TemporalUnet1D(24, 8, False, attention=True)
    L, v = _ffi.lib(), C.c_int32()
    assert L.cindm_unet1d_get_option(m._h, b"level_pairs", C.byref(v)) == 0 and v.value == 1
    for val in (0, 1):
        assert L.cindm_unet1d_set_option(m._h, b"level_pairs", val) == 0
        assert L.cindm_unet1d_get_option(m._h, b"level_pairs", C.byref(v)) == 0 and v.value == val


@gpu
@pytest.mark.parametrize("hz,F", [(24, 8), (24, 4), (16, 8), (16, 4)], ids=["hz24-F8", "hz24-F4", "hz16-F8", "hz16-F4"])
def test_forward_bitwise(device, hz, F):
    """Horizon 24 (level0 stage with two position tiles) and 16 (one), transition_dim 8 and 4, batch 1 / 3 / 19, t = 0 / 417 / 999.
    The stand-alone level kernels serve both horizons (test_selection checks the launch counts), so the pairs are fused in all of them."""
    m = _unet(device, hz, F)
    g = torch.Generator().manual_seed(100 * hz + F)
    xs = {B: torch.randn((B, hz, F), generator=g).to(device) for B in (1, 3, 19)}

    def run():
        return [m(x, torch.full((B,), t, device=device)).clone() for B, x in xs.items() for t in (0, 417, 999)]
    on, off = _on_off(m, run)
    for a, b in zip(on, off):
        assert bool(torch.isfinite(a).all()) and torch.equal(a, b), (hz, F, tuple(a.shape))


@gpu
@pytest.mark.parametrize("hz", [24, 16])
def test_forward_taps_bitwise(device, hz):
    """taps = 1, batch 3: every tap equals the stand-alone path's -- including downs.0.3 and ups.1.3, the hand-over tensors that the fused
    launches write for the tap API only."""
    m = _unet(device, hz, 8)
    m.set_option("taps", 1)
    x = torch.randn((3, hz, 8), generator=torch.Generator().manual_seed(hz)).to(device)

    def run():
        y = m(x, torch.full((3,), 417, device=device)).clone()
        return [y] + [m.tap(k, 3).clone() for k in TAPS]
    on, off = _on_off(m, run)
    for k, a, b in zip(["eps"] + TAPS, on, off):
        assert bool(torch.isfinite(a).all()) and torch.equal(a, b), (hz, k)


@gpu
def test_sampling_bitwise(device):
    """DDPM loop of 19 designs over six steps -- graph replay, plain stream and an explicit noise tape --, four DDIM steps of a 250-step
    schedule, and a two-window mean-inside composition of three designs."""
    m = _unet(device)
    d = _diffusion(m, device)
    dd = _diffusion(m, device, sampling_timesteps=250, ddim_sampling_eta=0.5)
    t = O.NoiseTape.make(7, (19, 24, 8), 1000)
    tape = cindm_amd.NoiseTape(t.init, t.step, None, t.cond)
    z = torch.zeros((19, 24, 8), device=device)

    def run():
        return [d.sample(batch_size=19, n_composed=0, t_stop=994, seed=11),
                d.sample(batch_size=19, n_composed=0, t_stop=994, seed=11, use_graph=False),
                d.sample(batch_size=19, n_composed=0, t_stop=994, noise=tape),
                dd.ddim_sample((19, 24, 8), None, seed=5, step_range=(0, 4), init_img=z + 0.1),
                d.sample(batch_size=3, n_composed=1, compose_start_step=16, compose_mode="mean-inside", seed=13, t_stop=994)]
    on, off = _on_off(m, run)
    for i, (a, b) in enumerate(zip(on, off)):
        assert bool(torch.isfinite(a).all()) and torch.equal(a, b), i
    assert torch.equal(on[0], on[1])
    assert _ffi.lib().cindm_unet1d_status(m._h, None) == 0


@gpu
def test_selection(device):
    """Two launches fewer per step at 19 rows (both horizons), the same launches at 321 rows (above 320 rows level0 / level1 run two
    workgroups per CU and keep their own launches), and the same two fewer whatever the step driver adds around the forward."""
    for hz in (24, 16):
        m = _unet(device, hz, 8)
        d = _diffusion(m, device, hz)
        n = {}
        for B in (19, 321):
            on, off = _on_off(m, lambda: (d.sample(batch_size=B, n_composed=0, t_stop=998, seed=1), d.last_step_info()[0]))
            assert torch.equal(on[0], off[0]), (hz, B)
            n[B] = (on[1], off[1])
        assert n[19][0] == n[19][1] - 2, (hz, n)
        assert n[321][0] == n[321][1], (hz, n)
    m = _unet(device)
    d = _diffusion(m, device)
    try:
        for key in ("fuse_update", "pingpong"):
            m.set_option(key, 0)
            on, off = _on_off(m, lambda: (d.sample(batch_size=19, n_composed=0, t_stop=998, seed=1), d.last_step_info()[0]))
            assert torch.equal(on[0], off[0]) and on[1] == off[1] - 2, (key, on[1], off[1])
            m.set_option(key, 1)
    finally:
        m.set_option("fuse_update", 1); m.set_option("pingpong", 1)


@gpu
@pytest.mark.parametrize("opts", [{"level1": 2}, {"level1": 0}, {"ups_tail": 0}, {"ups_last": 0}, {"level0": 0}],
                         ids=["level1_2", "level1_0", "ups_tail_0", "ups_last_0", "level0_0"])
def test_fallbacks_reproduce_todays_output(device, opts):
    """A pair is fused only when both of its stand-alone kernels would have run: with one of them switched off (or level1 at two samples
    per workgroup) the option changes nothing for that pair, and the output is that setting's output without the option."""
    m = _unet(device)
    for k, v in opts.items():
        m.set_option(k, v)
    d = _diffusion(m, device)
    x = torch.randn((19, 24, 8), generator=torch.Generator().manual_seed(9)).to(device)

    def run():
        return (m(x, torch.full((19,), 417, device=device)).clone(), d.sample(batch_size=19, n_composed=0, t_stop=996, seed=4),
                d.last_step_info()[0])
    on, off = _on_off(m, run)
    assert torch.equal(on[0], off[0]) and torch.equal(on[1], off[1]), opts
    # level0 = 0 switches all four level kernels off: no pair; the other settings leave exactly one pair standing
    assert off[2] - on[2] == (0 if "level0" in opts else 1), (opts, on[2], off[2])
