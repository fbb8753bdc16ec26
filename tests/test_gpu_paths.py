"""GPU (MI355X): every selectable kernel path of the library, and the bench-size shapes, under the driver-run suite.

1. Kernel paths.  libcindm_hip.so keeps alternative implementations of most layers (exact fp32-MFMA kernels, per-layer
   launches instead of level kernels, three-launch attention, the conv_gemm_h3 path instead of dconv_kernel, ...),
   selected per model handle with ``set_option`` (cindm_unet1d_set_option / cindm_unet2d_set_option).  Each option set
   below runs the U-Net forward goldens, the per-block goldens and a 100-step free-running chain against the reference's
   vectors, at the same tolerances as the default path.
2. Branches the first fixture set did not reach (tests/golden/steps_1d_r2.npz, oracle/make_golden_r2.py):
   objective pred_x0 / pred_v, eight bodies (28 pairs), initialization_mode 1 / 2.
3. Bench-size shapes: config 4 at 128 designs per GPU (768 pair rows + 512 single rows) and config 5 at 64 designs x 2
   boundaries -- rows against the oracle on a subset, bitwise independence of the partition, shared states."""
import os

import numpy as np
import pytest
import torch

import cindm_amd
import cindm_oracle as O
from test_gpu_parity import TOL_CHAIN, TOL_FWD, TOL_STEP, _tape, build_unet, rel

pytestmark = pytest.mark.gpu

PATHS_1D = [
    {"mfma_f32": 1},                      # every product on the exact fp32 MFMA kernels
    {"local_gn": 0},                      # consumer-side GroupNorm (A / B / C launches), no fused levels
    {"attn_site": 0},                     # three-launch attention (wide qkv, core, out projection)
    {"level0": 0},                        # no level kernels: per-layer launches at every level
    {"level1": 2},                        # two samples per workgroup in level1_down_kernel
    {"level1": 0}, {"ups_last": 0}, {"ups_tail": 0},
    {"ws_alias": 2},                      # dead intermediates' workspace blocks recycled at every batch size (default: above 320 rows)
    {"pingpong": 0},                      # step counter / exchange epochs advanced by step_counter_kernel (one more launch per step)
    {"dconv2": 0},                        # deep-level blocks as two dconv_kernel launches (no in-launch all-gather)
    {"dresample": 0},                     # deep-level resampling convolutions on conv_gemm_h3_kernel<3 | 4>
    {"dresample": 1},                     # ... on dresample_kernel with 32 columns per workgroup at every batch size (default: 16 below 512 rows)
    {"dconv": 0},                         # deep levels on conv_gemm_h3_kernel
    {"attn_head": 0},                     # deep attention sites on attn1d_site_h3_kernel
    {"attn_head": 2},                     # ... all of them on attn1d_head_kernel
    {"l2_prefetch": 0},
    {"dconv": 0, "level0": 0, "attn_head": 0},      # the round-1 per-layer path
    {"no_exchange": 1},                   # the exchange-free selection a timed-out chain is re-run on (no in-launch hand-over between workgroups)
    {"tune": 3},                          # round 5's memory-system choices: L2 warm-ups at the head of a launch, outputs left dirty in L2
    {"tune": 1}, {"tune": 2},             # ... one at a time (bit 0: warm-up placement / regions, bit 1: plain output stores)
]
IDS_1D = ["-".join(f"{k}{v}" for k, v in p.items()) for p in PATHS_1D]


def build_with(device, opts, **kw):
    m, sd = build_unet(device, **kw)
    for k, v in opts.items():
        m.set_option(k, v)
    return m, sd


@pytest.mark.parametrize("opts", PATHS_1D, ids=IDS_1D)
def test_unet1d_paths_golden(gold_dir, device, opts):
    g = np.load(os.path.join(gold_dir, "unet1d_fwd.npz"))
    m, _ = build_with(device, opts)
    x = torch.from_numpy(g["x"]).to(device)
    for t in (0, 500, 999):
        assert rel(m(x, torch.full((4,), t, device=device)), g[f"eps_t{t}"]) < TOL_FWD, (opts, t)
    m.set_option("taps", 1)
    m(x[:2], torch.full((2,), 500, device=device))
    for k in ("downs.0.1", "downs.0.3", "downs.1.0", "downs.2.1", "downs.3.2", "mid_block1", "mid_attn", "mid_block2", "ups.0.0",
              "ups.0.3", "ups.1.1", "ups.2.2", "ups.2.3"):
        assert rel(m.tap(k, 2), g["tap." + k]) < TOL_FWD, (opts, k)


@pytest.mark.parametrize("opts", PATHS_1D, ids=IDS_1D)
def test_unet1d_paths_chain_and_ragged(gold_dir, device, opts):
    """100 free-running steps of config 1 against the reference's checkpoint at t = 900, and a ragged batch vs the oracle."""
    g = np.load(os.path.join(gold_dir, "chains_1d.npz"))
    m, sd = build_with(device, opts)
    d = cindm_amd.GaussianDiffusion1D(m, image_size=24, conditioned_steps=0, timesteps=1000, sampling_timesteps=1000).to(device)
    ts = list(g["cfg1.ckpt_t"])
    part = d.sample(batch_size=4, n_composed=0, compose_n_bodies=2, noise=_tape(1234, (4, 24, 8), 1000), t_stop=900)
    assert rel(part, g["cfg1.ckpt"][ts.index(900)]) < TOL_CHAIN, opts
    x = torch.randn((19, 24, 8), generator=torch.Generator().manual_seed(5))
    ref = O.unet1d_forward(sd, x, torch.full((19,), 611, dtype=torch.long))
    assert rel(m(x.to(device), torch.full((19,), 611, device=device)), ref) < TOL_FWD, opts
    assert cindm_amd._ffi.lib().cindm_unet1d_status(m._h, None) == 0


@pytest.mark.parametrize("opts", [{"mfma_f32": 1}, {"la_site": 0}, {"conv_ws": 0}, {"ws_alias": 0}, {"tail_h3": 0},
                                  {"ws_nosplit": 0}, {"ws_nosplit": 1}, {"la_wpi": 4, "la_nsplit": 4}],
                         ids=["mfma_f32", "la_site0", "conv_ws_0", "ws_alias_0", "tail_h3_0", "ws_kgroups", "ws_nosplit_all", "la_4_per_image"])
def test_unet2d_paths_golden(gold_dir, device, opts):
    from test_gpu_parity_2d import build_unet2d
    g = np.load(os.path.join(gold_dir, "unet2d_fwd.npz"))
    m, _ = build_unet2d(device)
    for k, v in opts.items():
        m.set_option(k, v)
    x = torch.from_numpy(g["x"]).to(device)
    for t in (0, 500, 999):
        assert rel(m(x, torch.full((2,), t, device=device)), g[f"eps_t{t}"]) < TOL_FWD, (opts, t)


@pytest.mark.parametrize("conv_ws", [1, 2, 3], ids=["all", "plain_only", "groupnorm_only"])
def test_unet2d_conv_ws_repeatable(device, conv_ws):
    """The persistent wave-specialised 3x3 kernel (conv2d_ws_kernel) is a producer / consumer pipeline inside one
    workgroup: 40 repeats of one forward must be bit-identical, block by block (a stale window pixel in its staging
    showed up as 3 wrong output pixels in about one run of five while it was being written), and agree with the
    per-tile kernel (conv_ws = 0) to rounding.  conv_ws = 2 / 3 route only the plain-source / only the
    GroupNorm-on-load convolutions through it, so both sides of the statistics hand-over are exercised."""
    from test_gpu_parity_2d import build_unet2d
    m, _ = build_unet2d(device)
    x = torch.randn((2, 21, 64, 64), generator=torch.Generator().manual_seed(1)).to(device)
    t = torch.full((2,), 500, device=device)
    names = ["downs.0.1", "downs.1.3", "mid_block1", "mid_block2", "ups.0.0", "ups.0.1", "ups.1.1", "final_res_block"]
    m.set_option("conv_ws", 0)
    m(x, t)
    ref = {n: m.tap(n, 2).clone() for n in names}
    m.set_option("conv_ws", conv_ws)
    first = None
    for it in range(40):
        m(x, t)
        cur = {n: m.tap(n, 2).clone() for n in names}
        if first is None:
            first = cur
            for n in names:
                assert rel(cur[n], ref[n].cpu().numpy()) < 1e-5, (conv_ws, n)
        for n in names:
            assert torch.equal(cur[n], first[n]), (conv_ws, n, it)


def test_unet2d_forward_128_images_repeatable_and_batch_independent(device):
    """The bench shape of config 5 (128 images per evaluation): every workgroup slot of the GPU is reused several times per
    launch, which is where two intra-kernel hand-over bugs of round 2 showed (sporadically wrong pixels in workgroups
    after the first residency wave).  Five forwards must be bit-identical, block by block, and images 60..67 must equal
    an 8-image forward of the same inputs."""
    from test_gpu_parity_2d import build_unet2d
    m, _ = build_unet2d(device)
    x = torch.randn((128, 21, 64, 64), generator=torch.Generator().manual_seed(3)).to(device)
    t = torch.full((128,), 500, device=device)
    names = ["downs.0.1", "downs.1.3", "mid_block1", "mid_attn", "mid_block2", "ups.0.1", "ups.1.1", "final_res_block"]
    y0 = m(x, t)
    first = {n: m.tap(n, 128).clone() for n in names}
    assert bool(torch.isfinite(y0).all())
    for it in range(4):
        y = m(x, t)
        for n in names:
            assert torch.equal(m.tap(n, 128), first[n]), (n, it)
        assert torch.equal(y, y0), it
    y8 = m(x[60:68].contiguous(), t[:8])
    assert torch.equal(y0[60:68], y8)


@pytest.mark.parametrize("objective", ["pred_noise", "pred_x0", "pred_v"])
def test_fused_update_equals_update_kernel(device, unet8, objective):
    """Plain single-model steps run their reverse-step update inside ups_last_kernel (option fuse_update); it must be
    bit-identical to the separate compose_update_kernel -- counter-based noise and an explicit tape, every objective."""
    m, _ = unet8
    d = cindm_amd.GaussianDiffusion1D(m, image_size=24, conditioned_steps=0, timesteps=1000, sampling_timesteps=1000,
                                      objective=objective).to(device)
    tape = _tape(5, (19, 24, 8), 1000)
    res, info = {}, {}
    try:
        for v in (0, 1):
            m.set_option("fuse_update", v)
            res[v] = (d.sample(batch_size=19, n_composed=0, compose_n_bodies=2, seed=17, sample_offset=3, t_stop=985),
                      d.sample(batch_size=19, n_composed=0, compose_n_bodies=2, noise=tape, t_stop=985),
                      d.sample(batch_size=19, n_composed=0, compose_n_bodies=2, seed=17, sample_offset=3, t_stop=985, use_graph=False))
            # the step the library actually emitted: with the switch on there is no compose_update_kernel launch
            info[v] = d.last_step_info()
    finally:
        m.set_option("fuse_update", 1)
    assert info[1][1] is True and info[0][1] is False, info
    assert info[1][0] == info[0][0] - 1, info
    for a, b in zip(res[0], res[1]):
        assert torch.equal(a, b)
    assert torch.equal(res[1][0], res[1][2])


@pytest.mark.parametrize("mode", ["mean", "noise_sum", "mean-inside", "sum-inside"])
def test_fused_update_every_single_window_mode(device, unet8, mode):
    """sample() reaches the library as an OUTSIDE / INSIDE composition with one window and one pair, never as the plain
    descriptor: each of those modes must take the fused update (round 2's switch only matched the plain descriptor, so it
    never fired from sample()) and reproduce the separate kernel bit for bit."""
    m, _ = unet8
    d = cindm_amd.GaussianDiffusion1D(m, image_size=24, conditioned_steps=0, timesteps=1000, sampling_timesteps=1000).to(device)
    out = {}
    try:
        for v in (0, 1):
            m.set_option("fuse_update", v)
            out[v] = d.sample(batch_size=7, n_composed=0, compose_n_bodies=2, compose_mode=mode, seed=3, t_stop=990)
            assert d.last_step_info()[1] is bool(v), (mode, v)
    finally:
        m.set_option("fuse_update", 1)
    assert torch.equal(out[0], out[1])
    # composition over windows keeps the separate kernel
    d.sample(batch_size=3, n_composed=1, compose_start_step=16, compose_n_bodies=2, compose_mode=mode, seed=3, t_stop=998)
    assert d.last_step_info()[1] is False


@pytest.mark.parametrize("cfg", ["plain", "windows", "multibody"])
def test_pingpong_step_state(device, unet8, cfg):
    """The plain sample loop keeps its step counter and exchange epochs in two slots; a step reads one and its own update
    writes the other (no step_counter_kernel launch; the graph holds two steps, an odd count ends with a one-step graph).
    Odd and even step counts, repeated calls on one handle, an eager forward in between: bit-identical to the
    counter-kernel loop, one launch fewer per step, no exchange time-out."""
    m, _ = unet8
    if cfg == "multibody":
        m4, _ = build_unet(device, F=4)
        d = cindm_amd.GaussianDiffusion1D(m, image_size=20, conditioned_steps=4, timesteps=1000, sampling_timesteps=1000).to(device)
        d.model_unconditioned = m4
        cond = torch.rand((9, 4, 16), generator=torch.Generator().manual_seed(1)).to(device)
        run = lambda n, **kw: d.sample_compose_multibodies(cond, n, 0, 4, seed=3, **kw)
        steps = (7, 6)
    else:
        d = cindm_amd.GaussianDiffusion1D(m, image_size=24, conditioned_steps=0, timesteps=1000, sampling_timesteps=1000).to(device)
        kw0 = dict(n_composed=0) if cfg == "plain" else dict(n_composed=2, compose_start_step=16, compose_mode="mean-inside")
        run = lambda n, **kw: d.sample(batch_size=21, compose_n_bodies=2, seed=3, t_stop=1000 - n, **kw0, **kw)
        steps = (7, 6, 1)
    ref, info = {}, {}
    try:
        for pp in (0, 1):
            m.set_option("pingpong", pp)
            outs = []
            for n in steps:
                outs.append(run(n))
                outs.append(run(n))                          # the cached graphs again
                info[(pp, n)] = d.last_step_info()[0]
                m(torch.zeros((3, 24, 8), device=device), torch.zeros((3,), device=device))      # an eager forward between loops
            outs.append(run(steps[0], use_graph=False))
            ref[pp] = outs
    finally:
        m.set_option("pingpong", 1)
    for a, b in zip(ref[0], ref[1]):
        assert torch.equal(a, b)
    assert torch.equal(ref[1][0], ref[1][1]) and torch.equal(ref[1][0], ref[1][-1])
    for n in steps:
        assert info[(1, n)] == info[(0, n)] - 1, info
    assert cindm_amd._ffi.lib().cindm_unet1d_status(m._h, None) == 0


def test_workspace_recycling(device, unet8):
    """On the sampling path the workspace blocks of dead intermediates are recycled: a fraction of the bytes, the same bits."""
    m, _ = unet8
    L = cindm_amd._ffi.lib()
    d = cindm_amd.GaussianDiffusion1D(m, image_size=24, conditioned_steps=0, timesteps=1000, sampling_timesteps=1000).to(device)
    size, out = {}, {}
    try:
        for v in (0, 2):
            m.set_option("ws_alias", v)
            m.sync_weights()
            size[v] = L.cindm_unet1d_workspace_bytes(m._h, 768)
            size[v, 256] = L.cindm_unet1d_workspace_bytes(m._h, 256)
            out[v] = (d.sample(batch_size=37, n_composed=0, compose_n_bodies=2, seed=2, t_stop=988),
                      d.sample(batch_size=5, n_composed=2, compose_start_step=16, compose_mode="mean-inside", seed=2, t_stop=994))
    finally:
        m.set_option("ws_alias", 1)
    assert size[2] < 0.4 * size[0], size
    assert size[2] < 120 << 20, size                     # 768 rows (config 3): weights (83 MB) + activations stay inside the 256 MiB Infinity Cache
    for a, b in zip(out[0], out[2]):
        assert torch.equal(a, b)
    m.set_option("ws_alias", 1)
    m.sync_weights()
    assert L.cindm_unet1d_workspace_bytes(m._h, 768) == size[2] and L.cindm_unet1d_workspace_bytes(m._h, 256) == size[0, 256] > size[2, 256]     # automatic above 320 rows
    x = torch.randn((19, 24, 8), generator=torch.Generator().manual_seed(5)).to(device)
    t = torch.full((19,), 611, device=device)
    y1 = m(x, t)
    m.set_option("ws_alias", 2)
    try:
        assert torch.equal(m(x, t), y1)
    finally:
        m.set_option("ws_alias", 1)


def test_exchange_timeout_is_recovered(device):
    """A pair exchange whose partner never publishes (ablation dbg = 39: odd n-tiles of the dconv kernels skip their publish,
    short spin bound) stands in for foreign load keeping a partner workgroup off the chip.  forward(), p_sample*() and sample()
    must RECOVER: the work is re-run once on the exchange-free kernels ("no_exchange") and the results are the ones that
    selection gives by itself -- bit for bit -- and right against the oracle; the handle counts the recoveries and works on the
    fast kernels again afterwards."""
    m, sd = build_unet(device)
    m.set_option("auto_range", 0)           # (the calibration forward at finalize would hit the ablation too)
    x = torch.randn((32, 24, 8), generator=torch.Generator().manual_seed(2)).to(device)
    t = torch.full((32,), 500, device=device)
    d = cindm_amd.GaussianDiffusion1D(m, image_size=24, conditioned_steps=0, timesteps=1000, sampling_timesteps=1000).to(device)
    kw = dict(compose_mode="mean", n_composed=0, single_model_step=24, compose_n_bodies=2)
    nz = torch.randn((32, 24, 8), generator=torch.Generator().manual_seed(3)).to(device)
    # what the exchange-free selection computes on its own
    m.exchange_free(True)
    ref_fwd = m(x, t).clone()
    ref_chain = d.sample(batch_size=32, n_composed=0, compose_n_bodies=2, seed=1, t_stop=997).clone()
    ref_step = d.p_sample_compose_outside(x, None, 500, noise=nz, **kw)[0].clone()
    m.exchange_free(False)
    assert m.recovered == 0
    m.set_option("dbg", 39)
    got = m(x, t)
    assert m.recovered == 1 and torch.equal(got, ref_fwd)
    ref = O.unet1d_forward(sd, x[:4].cpu(), torch.full((4,), 500, dtype=torch.long))
    assert rel(got[:4], ref) < TOL_FWD
    chain = d.sample(batch_size=32, n_composed=0, compose_n_bodies=2, seed=1, t_stop=997)
    assert m.recovered == 2 and torch.equal(chain, ref_chain)
    step = d.p_sample_compose_outside(x, None, 500, noise=nz, **kw)[0]
    assert m.recovered == 3 and torch.equal(step, ref_step)
    # opting out of the recovery: the time-out surfaces as CindmError -- never as silently wrong designs
    m.recover_exchange_timeouts = False
    with pytest.raises(cindm_amd.CindmError, match="exchange"):
        m(x, t)
    with pytest.raises(cindm_amd.CindmError, match="exchange"):
        d.p_sample_compose_outside(x, None, 500, noise=nz, **kw)
    with pytest.raises(cindm_amd.CindmError, match="recover = 0"):          # the library's chain loops honour the opt-out too
        d.sample(batch_size=32, n_composed=0, compose_n_bodies=2, seed=1, t_stop=997)
    m.poll_raw(device)                                                        # (the failed chain left its flag raised)
    m.recover_exchange_timeouts = True
    assert d.last_chain_info()["chains_in_flight"] == 1
    m.set_option("dbg", 0)
    m.set_option("auto_range", 1)
    n0 = m.recovered
    fast = m(x, t)
    assert m.recovered == n0 and rel(fast[:4], ref) < TOL_FWD and rel(fast, ref_fwd) < TOL_FWD


def test_forward_check_opt_out(device):
    """forward(check=False) issues the launches and returns without the device-to-host flag read (asynchronous callers poll
    themselves); under a stream capture the check is skipped automatically -- a synchronise would invalidate the capture."""
    m, _ = build_unet(device)
    x = torch.randn((8, 24, 8), generator=torch.Generator().manual_seed(4)).to(device)
    t = torch.full((8,), 300, device=device)
    ref = m(x, t).clone()
    out = m(x, t, check=False)
    assert m.poll_status(device) is False and torch.equal(out, ref)
    s = torch.cuda.Stream(device=device)
    s.wait_stream(torch.cuda.current_stream(device))
    with torch.cuda.stream(s):
        m(x, 300)                                # (workspace, exchange regions and epochs set up outside the capture)
        torch.cuda.synchronize(device)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            y = m(x, 300)                        # (an int timestep: reading a timestep TENSOR is a host synchronisation)
        g.replay()
        torch.cuda.synchronize(device)
        assert m.poll_status(device) is False and torch.equal(y, ref)


@pytest.mark.stress_gate
@pytest.mark.parametrize("seed", [1, 7919])
def test_stress_mode_1d(device, seed):
    """Pseudo-random pauses in front of every in-kernel hand-over (option "stress" = seed: dconv_kernel's GroupNorm pair
    exchange and its LDS reductions, attn1d_head_kernel's head exchange): the 256-row forward and a 768-row forward
    (three residency waves) must equal the unstressed results bit for bit, with no exchange time-out."""
    m, _ = build_unet(device)
    res = {}
    for rows in (256, 768):
        x = torch.randn((rows, 24, 8), generator=torch.Generator().manual_seed(rows)).to(device)
        t = torch.full((rows,), 421, device=device)
        m.set_option("stress", 0)
        ref = m(x, t)
        m.set_option("stress", seed)
        for it in range(2):
            assert torch.equal(m(x, t), ref), (rows, seed, it)
    m.set_option("stress", 0)


@pytest.mark.stress_gate
@pytest.mark.parametrize("seed", [1, 7919])
def test_stress_mode_2d(device, seed):
    """The same for conv2d_ws_kernel's matrix / memory wave pipeline at the 128-image bench shape: pauses before each of
    its barriers on both sides, block outputs bit-identical to the unstressed forward."""
    from test_gpu_parity_2d import build_unet2d
    m, _ = build_unet2d(device)
    x = torch.randn((128, 21, 64, 64), generator=torch.Generator().manual_seed(3)).to(device)
    t = torch.full((128,), 500, device=device)
    names = ["downs.0.1", "downs.1.3", "mid_block1", "mid_block2", "ups.0.1", "ups.1.1", "final_res_block"]
    y0 = m(x, t)
    ref = {n: m.tap(n, 128).clone() for n in names}
    m.set_option("stress", seed)
    y1 = m(x, t)
    for n in names:
        assert torch.equal(m.tap(n, 128), ref[n]), (seed, n)
    assert torch.equal(y1, y0)
    m.set_option("stress", 0)


def test_chains_repeatable_at_bench_shape(device, unet8):
    """Whole chains at the shapes bench.py runs -- config 2 (256 designs, 1000 steps) and config 5 (64 designs x 2 boundaries,
    25 steps) -- twice with the same seed: bit-identical (graph replay of kernels that hand data between workgroups)."""
    from test_gpu_parity_2d import build_unet2d
    m, _ = unet8
    d = cindm_amd.GaussianDiffusion1D(m, image_size=24, conditioned_steps=0, timesteps=1000, sampling_timesteps=1000).to(device)
    a = d.sample(batch_size=256, n_composed=0, compose_n_bodies=2, seed=5)
    b = d.sample(batch_size=256, n_composed=0, compose_n_bodies=2, seed=5)
    assert bool(torch.isfinite(a).all()) and torch.equal(a, b)
    m2, _ = build_unet2d(device)
    d2 = cindm_amd.GaussianDiffusion(m2, image_size=64, frames=6, cond_frames=2, timesteps=1000, sampling_timesteps=1000,
                                     loss_type="l2").to(device)
    a2 = d2.sample(batch_size=64, num_boundaries=2, seed=5, t_stop=975)
    b2 = d2.sample(batch_size=64, num_boundaries=2, seed=5, t_stop=975)
    assert bool(torch.isfinite(a2).all()) and torch.equal(a2, b2)


def test_unet1d_forward_256_rows_repeatable(device, unet8):
    """The same guard for the 1-D path at the bench batch: five forwards of 256 rows are bit-identical (pair exchanges,
    head-split attention and the level kernels all hand data between workgroups inside a launch)."""
    m, _ = unet8
    x = torch.randn((256, 24, 8), generator=torch.Generator().manual_seed(11)).to(device)
    t = torch.full((256,), 333, device=device)
    y0 = m(x, t)
    assert bool(torch.isfinite(y0).all())
    for it in range(4):
        assert torch.equal(m(x, t), y0), it
    assert torch.equal(m(x[100:104].contiguous(), t[:4]), y0[100:104])


# ------------------------------------------------------------------ branches of round 2's fixtures
@pytest.fixture(scope="module")
def unet8(device):
    return build_unet(device)


@pytest.mark.parametrize("obj", ["pred_x0", "pred_v"])
def test_objective_steps_golden(gold_dir, device, unet8, obj):
    """objective = pred_x0 / pred_v (model/diffusion_1d.py:1018-1027): x_{t-1} and x0 of single steps."""
    g = np.load(os.path.join(gold_dir, "steps_1d_r2.npz"))
    d = cindm_amd.GaussianDiffusion1D(unet8[0], image_size=24, conditioned_steps=0, timesteps=1000, sampling_timesteps=1000,
                                      objective=obj).to(device)
    kw = dict(compose_mode="mean", n_composed=0, compose_start_step=4, single_model_step=24, compose_n_bodies=2)
    kw3 = dict(compose_mode="mean-inside", n_composed=2, compose_start_step=16, single_model_step=24, compose_n_bodies=2)
    for tag, fn, kws, ts in ((f"{obj}.outside_mean", d.p_sample_compose_outside, kw, (999, 500, 1, 0)),
                             (f"{obj}.inside_w3", d.p_sample_compose_inside, kw3, (500, 0))):
        for t in ts:
            x = torch.from_numpy(g[f"{tag}.t{t}.x"]).to(device)
            nz = torch.from_numpy(g[f"{tag}.t{t}.noise"]).to(device)
            out, x0 = fn(x, None, t, noise=nz, **kws)
            assert rel(out, g[f"{tag}.t{t}.out"]) < TOL_STEP, (tag, t)
            assert rel(x0, g[f"{tag}.t{t}.x0"]) < TOL_STEP, (tag, t)


@pytest.mark.parametrize("tag,ncomp", [("nb8", 0), ("nb8_w2", 1)])
def test_eight_bodies_step_golden(gold_dir, device, unet8, tag, ncomp):
    """compose_n_bodies = 8: 28 pair evaluations per window (scripts_paper/1D/cindm.sh:19-20; loop :977-990)."""
    g = np.load(os.path.join(gold_dir, "steps_1d_r2.npz"))
    d = cindm_amd.GaussianDiffusion1D(unet8[0], image_size=24, conditioned_steps=0, timesteps=1000, sampling_timesteps=1000).to(device)
    kw8 = dict(compose_mode="mean-inside", n_composed=ncomp, compose_start_step=10, single_model_step=24, compose_n_bodies=8)
    for t in (500, 0):
        x = torch.from_numpy(g[f"{tag}.t{t}.x"]).to(device)
        nz = torch.from_numpy(g[f"{tag}.t{t}.noise"]).to(device)
        out, x0 = d.p_sample_compose_inside(x, None, t, noise=nz, **kw8)
        assert tuple(out.shape) == tuple(x.shape) and x.shape[-1] == 32
        assert rel(out, g[f"{tag}.t{t}.out"]) < TOL_STEP, (tag, t)
        assert rel(x0, g[f"{tag}.t{t}.x0"]) < TOL_STEP, (tag, t)


@pytest.mark.parametrize("mode", [1, 2])
def test_initialization_modes_chain_golden(gold_dir, device, unet8, mode):
    """p_sample_loop's initialization_mode 1 (start from the image) / 2 (image + noise), :1672-1678: 1000-step chains."""
    g = np.load(os.path.join(gold_dir, "steps_1d_r2.npz"))
    d = cindm_amd.GaussianDiffusion1D(unet8[0], image_size=24, conditioned_steps=0, timesteps=1000, sampling_timesteps=1000).to(device)
    img = torch.from_numpy(g["init.img"]).to(device)
    out = d.sample(batch_size=1, cond=None, n_composed=0, compose_n_bodies=2, initialization_mode=mode, initialization_img=img,
                   noise=_tape(1300 + mode, (1, 24, 8), 1000))
    assert rel(out, g[f"init_mode{mode}.final"]) < TOL_CHAIN


# ------------------------------------------------------------------ bench-size shapes
def test_cfg4_at_128_designs(device, unet8):
    """Config 4's per-GPU share: 128 four-body designs = 768 pair rows + 512 single-body rows per step.  (1) three steps
    with explicit noise: designs 5, 40, 77, 127 against the oracle run on just those designs (rows are independent);
    (2) the full 400-step chain: finite, deterministic, and bitwise equal to a 4-design run of designs 40..43."""
    m8, sd8 = unet8
    m4, sd4 = build_unet(device, F=4)
    d = cindm_amd.GaussianDiffusion1D(m8, image_size=20, conditioned_steps=4, timesteps=1000, sampling_timesteps=1000).to(device)
    d.model_unconditioned = m4
    B, N = 128, 400
    g = torch.Generator().manual_seed(404)
    cond = torch.rand((B, 4, 16), generator=g)
    tape = O.NoiseTape(torch.randn((B, 20, 16), generator=g), torch.randn((N, B, 20, 16), generator=g))
    out = d.sample_compose_multibodies(cond.to(device), N, 0, 4, noise=cindm_amd.NoiseTape(tape.init, tape.step), t_stop=N - 3)
    rows = [5, 40, 77, 127]
    od = O.Diffusion1D(sd8, image_size=20, conditioned_steps=4, sd_uncond=sd4)
    sub = O.NoiseTape(tape.init[rows], tape.step[:, rows])
    ref = O.sample_compose_multibodies(od, cond[rows], N, sub, t_stop=N - 3)
    assert rel(out[rows], ref) < TOL_STEP
    a = d.sample_compose_multibodies(cond.to(device), N, 0, 4, seed=9)
    b = d.sample_compose_multibodies(cond.to(device), N, 0, 4, seed=9)
    assert torch.equal(a, b) and bool(torch.isfinite(a).all()) and tuple(a.shape) == (B, 20, 16)
    part = d.sample_compose_multibodies(cond[40:44].to(device), N, 0, 4, seed=9, sample_offset=40)
    assert torch.equal(a[40:44], part)
    assert cindm_amd._ffi.lib().cindm_unet1d_status(m8._h, None) == 0


def test_cfg5_at_64x2(device):
    """Config 5 at the bench shape (64 designs x 2 boundaries = 128 images per step), 6 reverse steps: 4 designs of the 64
    bitwise equal to a 4-design run, states shared across the boundary copies, boundary channels not, finite."""
    from test_gpu_parity_2d import build_unet2d
    m, _ = build_unet2d(device)
    d = cindm_amd.GaussianDiffusion(m, image_size=64, frames=6, cond_frames=2, timesteps=1000, sampling_timesteps=1000,
                                    loss_type="l2").to(device)
    full = d.sample(batch_size=64, num_boundaries=2, seed=21, t_stop=994)
    part = d.sample(batch_size=4, num_boundaries=2, seed=21, sample_offset=30, t_stop=994)
    assert tuple(full.shape) == (64, 2, 21, 64, 64) and bool(torch.isfinite(full).all())
    assert torch.equal(full[30:34], part)
    assert torch.equal(full[:, 0, :-3], full[:, 1, :-3])
    assert not torch.equal(full[:, 0, -3:], full[:, 1, -3:])


_PROF_CHILD = r"""
import ctypes as C, sys, numpy as np, torch
sys.path.insert(0, sys.argv[1])
import cindm_amd
from cindm_amd import _ffi
from cindm_amd.synthetic import synthetic_init_
dev = torch.device("cuda:0")
m = synthetic_init_(cindm_amd.TemporalUnet1D(horizon=24, transition_dim=8, cond_dim=0, dim=64, dim_mults=(1, 2, 4, 8), attention=True), 0).to(dev)
x = torch.randn((256, 24, 8), generator=torch.Generator().manual_seed(5)).to(dev)
t = torch.full((256,), 417, device=dev)
ref = torch.load(sys.argv[2]).to(dev)
L = _ffi.lib()
out = m(x, t).clone()
assert torch.equal(out, ref), "profiling build, clocks not armed: output differs from the production library"
assert L.cindm_unet1d_phase_prof_enable(m._h, 1) == 0, L.cindm_last_error()
out = m(x, t).clone()
torch.cuda.synchronize()
assert torch.equal(out, ref), "profiling build, clocks armed: output differs from the production library"
cap = 32 * 1024 * 8 * 16
buf = np.zeros(cap, dtype=np.uint64)
n = L.cindm_unet1d_phase_prof_read(m._h, buf.ctypes.data_as(C.c_void_p), cap, _ffi.current_stream(dev))
assert n >= 18, (n, L.cindm_last_error())
names = [L.cindm_unet1d_phase_prof_name(m._h, i).decode() for i in range(n)]
assert any(s.startswith("dconv2") for s in names) and any(s.startswith("ups_last") for s in names), names
rec = buf[: n * 1024 * 8 * 16].reshape(n, 1024, 8, 16)
for i in range(n):
    st = rec[i, 0, 0]                      # workgroup 0, wave 0 of launch i: the marks this kernel variant passes ascend
    st = st[st > 0].astype(np.int64)
    assert len(st) >= 2 and bool((np.diff(st) >= 0).all()), (names[i], st)
    if i:
        assert rec[i, 0, 0, 0] >= rec[i - 1, 0, 0, 0], "launch order"
print("PROF_OK", n)
"""


def test_phase_clock_build(device, tmp_path):
    """The in-replay phase clocks exist only in the profiling build: the production library refuses to arm them;
    libcindm_hip_prof.so (same sources, -DCINDM_PHASE_PROF) computes bit-identical outputs armed or not, and its records name every
    launch of a forward, ascend inside a wave and follow the launch order."""
    import subprocess
    import sys
    from cindm_amd.synthetic import synthetic_init_
    L = cindm_amd._ffi.lib()
    m = synthetic_init_(cindm_amd.TemporalUnet1D(horizon=24, transition_dim=8, cond_dim=0, dim=64, dim_mults=(1, 2, 4, 8), attention=True), 0).to(device)
    assert L.cindm_unet1d_phase_prof_enable(m._h, 1) != 0 and b"not a profiling build" in L.cindm_last_error()
    here = os.path.dirname(os.path.abspath(cindm_amd.__file__))
    if not os.path.exists(os.path.join(here, "libcindm_hip_prof.so")):
        pytest.skip("libcindm_hip_prof.so has not been built (python -m cindm_amd.build --prof)")
    x = torch.randn((256, 24, 8), generator=torch.Generator().manual_seed(5)).to(device)
    t = torch.full((256,), 417, device=device)
    ref = tmp_path / "ref.pt"
    torch.save(m(x, t).cpu(), ref)
    env = dict(os.environ, CINDM_LIB_VARIANT="prof")
    r = subprocess.run([sys.executable, "-c", _PROF_CHILD, os.path.dirname(here), str(ref)], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "PROF_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


@pytest.mark.parametrize("mode", ["mean-inside", "sum-inside", "mean", "noise_sum"])
def test_gather_read_in_place(device, unet8, mode):
    """Time composition of two-body states: the gathered U-Net batch is a row-wise copy of the state's windows, so level0_down_kernel
    reads them in place and compose_gather_kernel is not launched (option fuse_gather): one launch fewer per step, bit-identical
    designs (three windows -> 56 steps, counter noise and an explicit tape, graph and stream)."""
    m, _ = unet8
    d = cindm_amd.GaussianDiffusion1D(m, image_size=24, conditioned_steps=0, timesteps=1000, sampling_timesteps=1000).to(device)
    tape = _tape(9, (5, 56, 8), 1000)
    kw = dict(n_composed=2, compose_start_step=16, compose_n_bodies=2, compose_mode=mode, t_stop=992)
    res, info = {}, {}
    try:
        for v in (0, 1):
            m.set_option("fuse_gather", v)
            res[v] = (d.sample(batch_size=5, seed=23, sample_offset=1, **kw), d.sample(batch_size=5, noise=tape, **kw),
                      d.sample(batch_size=5, seed=23, sample_offset=1, use_graph=False, **kw))
            info[v] = d.last_step_info()
    finally:
        m.set_option("fuse_gather", 1)
    assert info[1][0] == info[0][0] - 1, info
    for a, b in zip(res[0], res[1]):
        assert torch.equal(a, b)
    assert torch.equal(res[1][0], res[1][2])


def test_ddim_loop_fuses_and_pingpongs(device, unet8):
    """The DDIM loop (round 4) keeps its step state in two slots and runs the update of a plain single-model step inside
    ups_last_kernel, as the DDPM loop does: 19 launches per step instead of 21, bit-identical to the separate update kernel and to
    the counter-kernel loop -- eta = 0 and eta > 0, counter noise and an explicit tape, an odd and an even number of steps."""
    m, _ = unet8
    out, info = {}, {}
    try:
        for eta in (0.0, 0.5):
            d = cindm_amd.GaussianDiffusion1D(m, image_size=24, conditioned_steps=0, timesteps=1000, sampling_timesteps=50,
                                              ddim_sampling_eta=eta).to(device)
            tape = _tape(4, (6, 24, 8), 50)
            for fu, pp in ((1, 1), (0, 1), (1, 0), (0, 0)):
                m.set_option("fuse_update", fu); m.set_option("pingpong", pp)
                z = torch.zeros((6, 24, 8), device=device)
                out[eta, fu, pp] = (d.ddim_sample((6, 24, 8), None, seed=5, step_range=(0, 7), init_img=z),
                                    d.ddim_sample((6, 24, 8), None, noise=tape, step_range=(0, 8), init_img=z),
                                    d.ddim_sample((6, 24, 8), None, seed=5, step_range=(43, 50), init_img=z + 0.3))     # incl. the last step (x_start)
                info[eta, fu, pp] = d.last_step_info()
    finally:
        m.set_option("fuse_update", 1); m.set_option("pingpong", 1)
    for eta in (0.0, 0.5):
        assert info[eta, 1, 1][1] is True and info[eta, 0, 0][1] is False, info
        assert info[eta, 1, 1][0] == info[eta, 0, 0][0] - 2, info
        for key in ((eta, 0, 1), (eta, 1, 0), (eta, 0, 0)):
            for a, b in zip(out[eta, 1, 1], out[key]):
                assert torch.equal(a, b), key


@pytest.mark.parametrize("F", [4, 16])
def test_fused_update_other_state_widths(device, F):
    """The fused update (noise generated at the top of ups_last_kernel, state rows requested a layer ahead) for state widths other
    than the paper's 8 features: F = 4 (a quarter of the final stage's lanes hold state elements) and F = 16 (all of them).  The
    plain single-model loop that accepts any width is the DDIM one: fused against the separate update kernel bit for bit, counter
    noise and an explicit tape, eta > 0 so that noise is drawn."""
    m, _ = build_unet(device, F=F, seed=7)
    res = {}
    try:
        for v in (0, 1):
            m.set_option("fuse_update", v)
            dd = cindm_amd.GaussianDiffusion1D(m, image_size=24, conditioned_steps=0, timesteps=1000, sampling_timesteps=50,
                                               ddim_sampling_eta=0.3).to(device)
            tape = _tape(2, (5, 24, F), 50)
            z = torch.zeros((5, 24, F), device=device)
            res[v] = (dd.ddim_sample((5, 24, F), None, seed=11, sample_offset=2, step_range=(0, 6), init_img=z),
                      dd.ddim_sample((5, 24, F), None, noise=tape, step_range=(0, 5), init_img=z),
                      dd.ddim_sample((5, 24, F), None, seed=11, step_range=(44, 50), init_img=z + 0.2))
            assert dd.last_step_info()[1] is bool(v)
    finally:
        m.set_option("fuse_update", 1)
    for a, b in zip(res[0], res[1]):
        assert torch.equal(a, b) and bool(torch.isfinite(a).all())
    assert float(res[1][0].abs().max()) > 0


def test_1d_chains_refuse_before_they_touch_the_device(device, unet8):
    """The 1-D chain entries refuse a workspace one byte short, a misaligned workspace, ``cond_steps > 0`` without ``cond`` and (DDIM)
    more steps than the U-Net has timesteps up front, with the reason -- not inside their first captured step, behind the stream
    switch, the x_T snapshot, the workspace memsets, the counter and epoch launches and the dropped graph.  After each refused call
    the state is bit-identical and an armed recorder is consumed; afterwards the first chain repeats bit for bit (step state, epochs
    and cached graph of the handles are usable).  Horizon 24, B = 3, three steps (odd: the ping-pong tail graph).
    Most of this also holds where the refusals arrive late but leave x alone; what tells the two apart is the source test
    tests/test_ddim_guided_host.py::test_entry_allocates_nothing."""
    import ctypes as C
    from cindm_amd import _ffi
    m, _ = unet8
    HZ, B, S = 24, 3, 3
    d = cindm_amd.GaussianDiffusion1D(m, image_size=HZ, conditioned_steps=0, timesteps=1000, sampling_timesteps=S).to(device)
    L, shape = _ffi.lib(), (B, HZ, 8)
    desc = d._desc_for(shape, "mean-inside", 0, 4, HZ, 2)
    no_cond = _ffi.ComposeDesc.from_buffer_copy(desc)
    no_cond.cond_steps = 4                                 # (one window of the model's horizon: 4 prepended rows + a state of 20)
    h, un, _ = d._prepare(desc, B, device)
    nbytes = L.cindm_ddpm1d_workspace_bytes(h, m._h, un, C.byref(desc), B)
    assert 0 < nbytes <= L.cindm_ddpm1d_workspace_bytes(h, m._h, un, C.byref(no_cond), B)
    ws = torch.empty(L.cindm_ddpm1d_workspace_bytes(h, m._h, un, C.byref(no_cond), B) + 256, dtype=torch.uint8, device=device)
    assert ws.data_ptr() % 256 == 0
    x_T = d._init_state(shape, device, None, 5, 0, d.num_timesteps)
    x = x_T.clone()
    times, coefs = d.ddim_schedule()
    tarr, carr = (C.c_int32 * (S + 1))(*times), coefs.contiguous()
    T1 = m.timesteps + 1                                   # one step more than the U-Net's per-timestep table has rows
    long_t, long_c = (C.c_int32 * (T1 + 1))(*range(T1 - 1, -2, -1)), torch.zeros((T1, 3))
    dz = cindm_amd.PointObjective([0.25, -0.5], 2, coef=2.0).descriptor("standard-recurrence-2")
    assert dz is not None and dz.recurrence == 2
    rec_buf = torch.zeros(T1 * x.numel(), device=device)   # (large enough for every call below: the refusal is never the recorder's)
    info = (C.c_int32 * 4)()
    stream = lambda: _ffi.current_stream(device)

    def good():
        x.copy_(x_T)
        with torch.cuda.device(device):
            _ffi.check(L.cindm_ddpm1d_sample(h, m._h, un, C.byref(desc), _ffi.ptr(x), None, None, C.c_uint64(5), 0, None, 0, None,
                                             999, 997, B, _ffi.ptr(ws), nbytes, stream(), 1))
        torch.cuda.synchronize(device)
        return x.clone()

    def entry(name, c, w, wb, n_steps, t, co, use_graph):
        head = (h, m._h, un, C.byref(c))
        tail = (B, w, wb, stream(), use_graph)
        if name == "sample":
            return L.cindm_ddpm1d_sample(*head, _ffi.ptr(x), None, None, C.c_uint64(5), 0, None, 0, None, 999, 997, *tail)
        if name == "ddim":
            return L.cindm_ddpm1d_sample_ddim(*head, _ffi.ptr(x), None, n_steps, t, _ffi.ptr(co), None, C.c_uint64(5), 0, None, 0, None, *tail)
        if name == "guided":
            return L.cindm_ddpm1d_sample_guided(*head, C.byref(dz), _ffi.ptr(x), None, None, None, C.c_uint64(5), 0, None, 0, None, None, 0,
                                                999, 997, *tail)
        return L.cindm_ddpm1d_sample_ddim_guided(*head, C.byref(dz), _ffi.ptr(x), None, n_steps, t, _ffi.ptr(co), None, None, C.c_uint64(5), 0,
                                                 None, 0, None, None, 0, *tail)

    def refused(name, use_graph, c=desc, w=None, wb=nbytes, n_steps=S, t=tarr, co=carr):
        _ffi.check(L.cindm_ddpm1d_set_recorder(h, _ffi.ptr(rec_buf), rec_buf.numel(), 1, 1))
        with torch.cuda.device(device):
            rc = entry(name, c, _ffi.ptr(ws) if w is None else w, wb, n_steps, t, co, use_graph)
        msg = L.cindm_last_error().decode()
        torch.cuda.synchronize(device)
        assert rc != 0 and torch.equal(x, x_T), (name, use_graph, msg)
        _ffi.check(L.cindm_ddpm1d_recorder_info(h, info))
        assert list(info) == [0, 0, 0, 0], (name, use_graph, msg)
        return msg

    first = good()
    assert bool(torch.isfinite(first).all()) and not torch.equal(first, x_T)
    x.copy_(x_T)
    for use_graph in (1, 0):
        for name in ("sample", "ddim", "guided", "ddim_guided"):
            assert "workspace too small" in refused(name, use_graph, wb=nbytes - 1)
            assert "workspace must be 256-byte aligned" in refused(name, use_graph, w=C.c_void_p(ws.data_ptr() + 16))
            assert "cond_steps > 0 requires cond" in refused(name, use_graph, c=no_cond, wb=ws.numel() - 256)
            if "ddim" in name:
                assert "more DDIM steps than the U-Net's timesteps" in refused(name, use_graph, n_steps=T1, t=long_t, co=long_c)
    again = good()                                         # no recorder armed: the refused calls consumed theirs
    _ffi.check(L.cindm_ddpm1d_recorder_info(h, info))
    assert list(info) == [0, 0, 0, 0] and not bool(rec_buf.any())
    assert torch.equal(again, first)


def test_second_chain_on_a_device_goes_exchange_free_up_front(device):
    """One sampling chain per device is the rule of the exchange kernels.  Two host threads run a chain each, at the same time, on
    their own streams and their own models: the library's per-device registry sees the second chain start while the first is in
    flight and puts it on the exchange-free plan UP FRONT -- no time-out fires, nothing is recovered, both results are right (the
    late chain bit-equal to what `no_exchange` computes by itself), last_chain_info() says which was which and the Python face
    warns once."""
    import threading
    import time
    import warnings
    models = [build_unet(device)[0] for _ in range(2)]
    diffs = [cindm_amd.GaussianDiffusion1D(m, image_size=24, conditioned_steps=0, timesteps=1000, sampling_timesteps=1000).to(device) for m in models]
    kw = dict(batch_size=64, n_composed=0, compose_n_bodies=2, seed=4, t_stop=940)
    long_kw = dict(kw, t_stop=0)                            # chain 0 of the concurrent pair: 1000 steps (~0.3 s) -- the overlap is FORCED
    fast = diffs[0].sample(**kw).clone()                     # alone on the device: the fast plan
    fast_long = diffs[0].sample(**long_kw).clone()
    models[1].exchange_free(True)
    slow = diffs[1].sample(**kw).clone()
    models[1].exchange_free(False)
    assert rel(fast, slow) < 1e-5
    cindm_amd.GaussianDiffusion1D._warned_crowded = False
    out, infos, errs = [None, None], [None, None], []
    gate = threading.Barrier(2)

    def run(i):
        try:
            with torch.cuda.stream(torch.cuda.Stream(device=device)):
                gate.wait()
                if i == 1:
                    time.sleep(0.05)                        # chain 0 (0.3 s) is in flight by now and for long after
                out[i] = diffs[i].sample(**(long_kw if i == 0 else kw)).clone()
                infos[i] = diffs[i].last_chain_info()
        except Exception as e:          # noqa: BLE001
            errs.append(e)

    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        th = [threading.Thread(target=run, args=(i,)) for i in range(2)]
        [t.start() for t in th]
        [t.join() for t in th]
    assert not errs, errs
    assert all(m.recovered == 0 for m in models), "a time-out fired: the registry did not demote the second chain"
    assert not any(i["recovered"] for i in infos)
    crowded = [i["exchange_free_up_front"] for i in infos]
    assert crowded == [False, True], crowded                 # (round 5's version accepted "no overlap" silently)
    assert infos[1]["chains_in_flight"] == 2
    assert any("ONE chain per device" in str(x.message) for x in w)
    # chain 0 (undisturbed plan) is bit-equal to its solo run.  The DEMOTED chain is held to the chain tolerance against its solo exchange-free run,
    # not to bit-equality: late in round 6 it came out with one to four samples -- always samples 11 - 13 of a 16-sample tile -- off by 1e-5 ... 7e-5
    # on most fresh boxes (never when repeated in the same process, never alone).  The best lead: dresample_kernel's 16-column form, where two
    # workgroups write the two 64-byte halves of every 128-byte fp32 output line (`dresample` = 0 or 1 in the second chain: 4 clean boxes of 4); the
    # exchange-free plan uses the 32-column form since, which made it rarer, not impossible (3 clean boxes, then 1 failure).  Open: DESIGN.md 4.12.
    assert torch.equal(out[0], fast_long)
    if not torch.equal(out[1], slow):
        nz = (out[1] != slow).nonzero()
        print("demoted chain under contention differs from its solo run: samples", sorted(set(nz[:, 0].tolist())), "elements", int(nz.shape[0]),
              "max |difference|", float((out[1] - slow).abs().max()))
    assert rel(out[1], slow) < TOL_CHAIN
    # ... and ONE handle cannot be inside two chains at once: the second caller gets an error, not a race on the handle's plan switches
    errs2, done = [], []

    def run_same(i):
        try:
            with torch.cuda.stream(torch.cuda.Stream(device=device)):
                if i == 1:
                    time.sleep(0.05)
                done.append(diffs[0].sample(**(long_kw if i == 0 else kw)))
        except cindm_amd.CindmError as e:
            errs2.append(str(e))

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        th = [threading.Thread(target=run_same, args=(i,)) for i in range(2)]
        [t.start() for t in th]
        [t.join() for t in th]
    assert len(done) == 1 and len(errs2) == 1 and "already inside a sampling chain" in errs2[0], (len(done), errs2)
    assert torch.equal(done[0], fast_long)
    assert torch.equal(diffs[0].sample(**kw), fast)         # the handle is free again


def test_unet2d_round5_paths_agree_at_full_occupancy(device):
    """The kernel variants added in round 5 at 128 images (every CU busy, several tiles per persistent workgroup -- the 2-image goldens
    cannot see a hand-over problem there): conv2d_ws without k-groups (16x16x32 and 32x32x16 forms), the pipelined ResnetBlock
    tails, the 128-query attention, the split-fp16 per-head products and the pipelined pixel-unshuffle 1x1 each agree with the round-4 selection to rounding, and
    the default selection repeats bit for bit."""
    from test_gpu_parity_2d import build_unet2d
    m, _ = build_unet2d(device)
    x = torch.randn((128, 21, 64, 64), generator=torch.Generator().manual_seed(3)).to(device)
    t = torch.full((128,), 400, device=device)
    new = m(x, t).clone()
    assert torch.equal(m(x, t), new)
    for v in (0, 1):                                # round 2's k-groups everywhere / K never split
        m.set_option("ws_nosplit", v)
        assert rel(m(x, t), new) < 5e-6, v
    m.set_option("ws_nosplit", 2)
    assert torch.equal(m(x, t), new)


def _standin_simulation(features, n_steps, **kw):
    """The deterministic stand-in of tests/test_host_logic.py (utils.simulation is a pymunk program): constant velocity with
    reflecting walls, [batch, n_bodies, 4] -> [batch, n_steps, n_bodies, 4]; runs on whatever device `features` lives on."""
    f = features.double()
    steps = torch.arange(1, n_steps + 1, dtype=torch.float64, device=f.device).view(1, -1, 1, 1)
    pos = f[:, None, :, :2] + f[:, None, :, 2:] * steps / 60.0
    pos = 200.0 - (pos.remainder(400.0) - 200.0).abs()
    vel = f[:, None, :, 2:].expand(-1, n_steps, -1, -1)
    return torch.cat([pos, vel], dim=-1).float()


def test_checkpoint_to_eval_simu_on_the_device(device, tmp_path):
    """SURVEY section 8 f4, end to end ON THE DEVICE: a checkpoint FILE -> `load_state_dict(torch.load(path)["model"])` (1-D,
    inference/inverse_design_diffusion_1d.py:179-180) and `Trainer(diffusion, ...).load(milestone)` (2-D, model/diffusion_2d.py:1213-1231)
    -> a few reverse steps on the HIP path -> `to_simulator_units` -> `eval_simu` (utils.py:1127-1148, stand-in simulator) on the device
    output -- compared with the oracle driven the same way from the same file."""
    from cindm_amd.data_utils import eval_simu, get_item_1d, to_simulator_units
    # ---- 1-D: the checkpoint a training run of the reference would have written ({"step", "model": diffusion.state_dict(), ...}) ----
    src, sd = build_unet(device)
    d_src = cindm_amd.GaussianDiffusion1D(src, image_size=24, conditioned_steps=0, timesteps=1000, sampling_timesteps=1000, loss_type="l1")
    path = tmp_path / "model-7.pt"
    torch.save({"step": 7000, "model": {k: v.detach().cpu() for k, v in d_src.state_dict().items()}, "version": "1.0"}, str(path))
    fresh = cindm_amd.TemporalUnet1D(24, 8, False, attention=True)
    d = cindm_amd.GaussianDiffusion1D(fresh, image_size=24, conditioned_steps=0, timesteps=1000, sampling_timesteps=1000, loss_type="l1")
    d.load_state_dict(torch.load(str(path), map_location="cpu")["model"])          # strict: the reference's key names
    d = d.to(device)
    tape = _tape(4242, (4, 24, 8), 1000)
    out = d.sample(batch_size=4, cond=None, n_composed=0, compose_n_bodies=2, noise=tape, t_stop=990)
    file_sd = {k[len("model."):]: v for k, v in torch.load(str(path), map_location="cpu")["model"].items() if k.startswith("model.")}
    od = O.Diffusion1D(file_sd, image_size=24, conditioned_steps=0)
    otape = O.NoiseTape.make(4242, (4, 24, 8), 1000)
    ref = O.sample(od, 4, otape, n_composed=0, compose_n_bodies=2, t_stop=990)
    assert out.is_cuda and rel(out, ref) < TOL_CHAIN
    # post-processing on the DEVICE output: simulator units and back, then the re-simulation + objective of eval_simu
    sim_units = to_simulator_units(out, 2)
    assert sim_units.is_cuda and tuple(sim_units.shape) == (8, 24, 4)

    class Batch(dict):
        dyn_dims = [0, 0, 0, 0]
    assert torch.allclose(get_item_1d(Batch(y=sim_units), "y"), out, rtol=0, atol=1e-6)
    objective = lambda traj: ((traj[:, -1, :2] - 0.25) ** 2).sum(-1).mean() + ((traj[:, -1, 4:6] + 0.5) ** 2).sum(-1).mean()
    pred, score = eval_simu(out[:, :4], objective, 2, 20, time_interval=4, simulation=_standin_simulation)
    pred_ref, score_ref = eval_simu(ref[:, :4], objective, 2, 20, time_interval=4, simulation=_standin_simulation)
    assert pred.is_cuda and tuple(pred.shape) == (4, 20, 8)
    assert rel(pred, pred_ref) < TOL_CHAIN and abs(float(score) - float(score_ref)) < TOL_CHAIN * max(1.0, abs(float(score_ref)))
    with pytest.raises(TypeError):
        eval_simu(out[:, :4], objective, 2, 20, simulation=None)
    # ---- 2-D: Trainer(diffusion, ...).load(milestone), as inverse_design_2d.py:191-207 does ----
    sd2 = O.synth_state_dict_2d(O.unet2d_param_shapes(64, (1, 2), 21), 3)
    donor = cindm_amd.Unet(dim=64, dim_mults=(1, 2), channels=21, image_size=64)
    donor.load_state_dict(sd2, strict=True)
    gd_src = cindm_amd.GaussianDiffusion(donor, image_size=64, frames=6, cond_frames=2, timesteps=1000, sampling_timesteps=1000,
                                         loss_type="l2", objective="pred_noise")
    torch.save({"step": 11, "model": {k: v.detach().cpu() for k, v in gd_src.state_dict().items()}, "version": "1.0"}, str(tmp_path / "model-3.pt"))
    m2 = cindm_amd.Unet(dim=64, dim_mults=(1, 2), channels=21, image_size=64)
    gd = cindm_amd.GaussianDiffusion(m2, image_size=64, frames=6, cond_frames=2, timesteps=1000, sampling_timesteps=1000,
                                     loss_type="l2", objective="pred_noise")
    tr = cindm_amd.Trainer(gd, None, results_folder=str(tmp_path), train_batch_size=1).load(3)
    assert tr.step == 11
    gd = gd.to(device)
    from test_gpu_parity_2d import _tape as tape2d
    t2 = tape2d(91, 1, 2, 21, 64, 64, 1000, t_min=996)
    out2 = gd.sample(batch_size=1, num_boundaries=2, noise=t2, t_stop=996)
    od2 = O.Diffusion2D(sd2, image_size=64, frames=6)
    steps = {t: (t2.step_state[t], t2.step_boundary[t]) for t in range(1, 1000)}
    ref2 = O.p_sample_loop_2d(od2, (1, 2, 21, 64, 64), t2.init, steps, t_stop=996)
    assert out2.is_cuda and rel(out2, ref2) < TOL_CHAIN


def test_bench_plain_run_dumps_the_last_timed_chain(device, tmp_path):
    """`bench.py` without --full prints the headline line only (no roofline leg, CPU leg or nested workloads), and --dump-outputs
    writes the designs of the LAST timed chain: the chain of that index (seed 1234 + warm-up + steps - 1), run here, reproduces them."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--steps", "2", "--warmup", "1", "--batch", "32",
                        "--dump-outputs", str(tmp_path / "dump")], capture_output=True, text=True, timeout=900, cwd=root, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    line = json.loads(lines[0])
    assert line["steps"] == 2 and line["warmup"] == 1 and line["ms_per_step"] > 0 and line["dtype"] == "f32"
    assert abs(line["value"] - 32 / (line["ms_per_step"] / 1000.0)) < 1e-2 * line["value"]
    assert line["roofline"] is None and not any(k in line for k in ("cpu_baseline", "rel_err", "workloads"))
    got = np.load(tmp_path / "dump" / "designs.npy")
    assert got.dtype == np.float32 and got.shape == (32, 24, 8) and np.isfinite(got).all()
    sys.path.insert(0, root)
    import bench
    want = bench.build_1d("cfg2", 32, device)["chain"](1 + 2 - 1, 0)
    assert rel(torch.from_numpy(got), want) < TOL_CHAIN
