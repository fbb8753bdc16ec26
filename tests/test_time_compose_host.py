"""The parallel time composition's host side (no GPU): a CPU restatement of composing_time_sample's loop on
cindm_oracle.model_predictions / ddim_coefs pinned against the reference's own run (tests/golden/time_compose_parallel.npz,
tests/manual/make_golden_time_compose.py), the refusals, the assembly of the returned pair, and the new entry's binding."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import cindm_amd
import cindm_oracle as O
from cindm_amd import _ffi
from cindm_amd.diffusion1d import time_compose_assemble, time_compose_segments

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "cindm_ddpm1d_sample_timecompose"

# tag: (horizon, Lc, R, K, S, eta) -- tests/manual/make_golden_time_compose.py; B = 5, F = 8 throughout
CASES = {"default": (24, 4, 20, 3, 6, 0.0), "stochastic": (24, 4, 20, 3, 6, 0.5), "whole_state": (8, 4, 4, 4, 6, 0.0),
         "two_segment": (24, 4, 20, 2, 4, 0.0)}
B, F = 5, 8


def load_case(gold_dir, tag):
    g = np.load(os.path.join(gold_dir, "time_compose_parallel.npz"))
    return {k: torch.from_numpy(g[f"{tag}.{k}"]) for k in ("cond", "init", "step", "img", "img_infered", "states")}


def _diffusion(hz=24, Lc=4, R=20, **kw):
    m = cindm_amd.TemporalUnet1D(hz, 8, False, attention=True)
    return cindm_amd.GaussianDiffusion1D(m, image_size=R, conditioned_steps=Lc, timesteps=1000, loss_type="l1", **kw)


def restated_loop(od, cond, init, step, S, eta, clip=True, x_starts=None):
    """:1823-1846: per step the hand-over from the current state, one prediction on all K * B rows, the DDIM update.
    Returns the state after every step [S, K, B, R, F]; ``x_starts``: a list that receives every step's x_start."""
    K, Bn = init.shape[0], init.shape[1]
    x = init.reshape((K * Bn,) + tuple(init.shape[2:])).clone()
    c = torch.zeros((K * Bn,) + tuple(cond.shape[1:]))
    c[:Bn] = cond
    states = []
    for i, (time, time_next) in enumerate(O.ddim_time_pairs(od.num_timesteps, S)):
        c[Bn:] = x[:(K - 1) * Bn, -od.conditioned_steps:]
        pred_noise, x_start = O.model_predictions(od, x, c, time, clip_x_start=clip)
        san, cc, sigma = O.ddim_coefs(od, time, time_next, eta)
        x = x_start if time_next < 0 else x_start * san + cc * pred_noise + sigma * step[i].reshape(x.shape)
        states.append(x.reshape(init.shape).clone())
        if x_starts is not None:
            x_starts.append(x_start.reshape(init.shape).clone())
    return torch.stack(states)


@pytest.mark.parametrize("tag", sorted(CASES))
def test_restatement_reproduces_reference_golden(gold_dir, tag):
    hz, Lc, R, K, S, eta = CASES[tag]
    g = load_case(gold_dir, tag)
    assert tuple(g["cond"].shape) == (B, Lc, F) and tuple(g["init"].shape) == (K, B, R, F)
    assert tuple(g["step"].shape) == tuple(g["states"].shape) == (S, K, B, R, F)
    od = O.Diffusion1D(O.synth_state_dict(O.unet1d_param_shapes(hz, F), seed=0), image_size=R, conditioned_steps=Lc)
    states = restated_loop(od, g["cond"], g["init"], g["step"], S, eta)
    for i in range(S):
        scale = float(g["states"][i].abs().max())
        assert float((states[i] - g["states"][i]).abs().max()) <= 2e-6 * scale, (tag, i)
    # the states between steps are not clamped (what the clamp of the last step cannot hide), the returned ones are
    assert float(g["states"][:-1].abs().max()) > 1.0 and float(g["states"][-1].abs().max()) <= 1.0
    assert float((g["img"].abs() == 1).float().mean()) < 0.5 and float((g["img_infered"].abs() == 1).float().mean()) < 0.5


@pytest.mark.parametrize("tag", sorted(CASES))
def test_tail_assembly_matches_fixture(gold_dir, tag):
    hz, Lc, R, K, S, eta = CASES[tag]
    g = load_case(gold_dir, tag)
    img, inf = time_compose_assemble(g["states"][-1].reshape(K * B, R, F), K)
    n = min(20, R)
    assert tuple(inf.shape) == tuple(g["img_infered"].shape) == (B, (K - 1) * n, F)
    assert torch.equal(img, g["img"]) and torch.equal(inf, g["img_infered"])
    for k in range(1, K):                     # segment order along the row axis
        assert torch.equal(inf[:, (k - 1) * n:k * n], g["states"][-1, k, :, -n:])


def test_tail_assembly_keeps_twenty_rows():
    x = torch.arange(3 * 2 * 24 * 4, dtype=torch.float32).reshape(6, 24, 4)
    img, inf = time_compose_assemble(x, 3)
    assert tuple(img.shape) == (2, 24, 4) and tuple(inf.shape) == (2, 40, 4)
    assert torch.equal(inf[:, :20], x[2:4, 4:]) and torch.equal(inf[:, 20:], x[4:6, 4:])


def test_segment_count_and_refusals():
    assert time_compose_segments(4, 20, 2) == 3 and time_compose_segments(4, 4, 1) == 2
    with pytest.raises(NotImplementedError, match="conditioned_steps == 0"):
        time_compose_segments(0, 24, 2)
    with pytest.raises(ValueError, match="n_composed"):
        time_compose_segments(4, 20, 0)
    with pytest.raises(ValueError, match="image_size 2 < conditioned_steps 4"):
        time_compose_segments(4, 2, 2)


def test_method_refuses_before_any_device_work():
    """Every refusal comes from the CPU-resident object, ahead of the CindmError of the missing device."""
    d0 = _diffusion(Lc=0, R=24, sampling_timesteps=4)
    with pytest.raises(NotImplementedError, match="conditioned_steps == 0"):
        d0.composing_time_sample((2, 24, 8), torch.zeros(2, 0, 8))
    d = _diffusion(sampling_timesteps=4)
    cond = torch.zeros(2, 4, 8)
    with pytest.raises(ValueError, match="n_composed"):
        d.composing_time_sample((2, 20, 8), cond, n_composed=0)
    with pytest.raises(ValueError, match="image_size"):
        _diffusion(hz=6, Lc=4, R=2, sampling_timesteps=4).composing_time_sample((2, 2, 8), cond)
    with pytest.raises(ValueError, match="conditioned_steps = 4"):
        d.composing_time_sample((2, 20, 8), torch.zeros(2, 3, 8))
    with pytest.raises(ValueError, match="features"):
        d.composing_time_sample((2, 20, 4), torch.zeros(2, 4, 4))
    for shape in ((3, 20, 8), (2, 24, 8), (2, 20, 4), (2, 20)):
        with pytest.raises(ValueError, match="shape must be"):
            d.composing_time_sample(shape, cond)
    good = cindm_amd.NoiseTape(torch.zeros(3, 2, 20, 8), torch.zeros(4, 3, 2, 20, 8))
    for tape in (cindm_amd.NoiseTape(torch.zeros(2, 2, 20, 8), good.step), cindm_amd.NoiseTape(good.init, torch.zeros(3, 4, 2, 20, 8)),
                 cindm_amd.NoiseTape(good.init, None)):
        with pytest.raises(ValueError, match="noise: init must be"):
            d.composing_time_sample((2, 20, 8), cond, noise=tape)
    with pytest.raises(ValueError, match="trajectory"):
        d.composing_time_sample((2, 20, 8), cond, return_trajectory_every=1, trajectory=("eps",))
    # and with everything in order, the CPU module is what is left to refuse
    with pytest.raises(cindm_amd.CindmError, match="no CPU execution path"):
        d.composing_time_sample((2, 20, 8), cond, noise=good)
    with pytest.raises(cindm_amd.CindmError, match="no CPU execution path"):
        d.composing_time_sample((2, 20, 8), cond, seed=0, return_trajectory_every=2, trajectory=("x", "x0"))


def test_sample_still_ignores_is_composing_time():
    """As the reference's sample(): the keyword selects nothing; the method is called directly."""
    import inspect
    src = inspect.getsource(cindm_amd.GaussianDiffusion1D.sample)
    assert "is_composing_time" in inspect.signature(cindm_amd.GaussianDiffusion1D.sample).parameters
    assert "composing_time_sample" not in src


def test_entry_is_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "cindm_hip.h")).read()
    m = re.search(r"int\s+" + NAME + r"\(([^;]*)\);", header)
    assert m
    params = [p.strip() for p in m.group(1).replace("\n", " ").split(",")]
    assert params == ["cindm_ddpm1d* h", "cindm_unet1d* pair", "cindm_unet1d* uncond", "const cindm_compose_desc* c", "float* x",
                      "const float* cond", "float* cond_buf", "int32_t n_seg", "int32_t n_steps", "const int32_t* times",
                      "const float* coefs", "const uint64_t* seeds", "const float* init_tape", "const float* noise_steps",
                      "int64_t sample_offset", "int64_t B", "void* ws", "size_t ws_bytes", "void* stream", "int32_t use_graph"]
    vp, i32, i64, sz = C.c_void_p, C.c_int32, C.c_int64, C.c_size_t
    want = [vp, vp, vp, C.POINTER(_ffi.ComposeDesc), vp, vp, vp, i32, i32, vp, vp, vp, vp, vp, i64, i64, vp, sz, vp, i32]
    assert _ffi.SIGNATURES[NAME] == (C.c_int, want)
    lib = _ffi.lib()
    assert lib.cindm_abi_version() == _ffi.ABI_VERSION      # an added entry: the version stays
    fn = getattr(lib, NAME)
    assert fn.restype is C.c_int and list(fn.argtypes) == want
    # argument checks come before any device work
    assert fn(None, None, None, None, None, None, None, 1, 4, None, None, None, None, None, 0, 5, None, 0, None, 0) != 0
    assert b"n_seg must be >= 2" in lib.cindm_last_error()
    assert fn(None, None, None, None, None, None, None, 3, 4, None, None, None, None, None, 0, 30000, None, 0, None, 0) != 0
    assert b"65535" in lib.cindm_last_error()
    assert fn(None, None, None, None, None, None, None, 3, 4, None, None, None, None, None, 0, 5, None, 0, None, 0) != 0
    assert b"null argument" in lib.cindm_last_error()


def test_entry_allocates_nothing_and_refuses_first():
    """The entry's file holds no allocation, and every refusal of the entry stands before its first launch, copy or synchronise."""
    src = open(os.path.join(ROOT, "cindm_amd", "csrc", "timecompose_host.inc")).read()
    assert not re.search(r"\bhip(Malloc|Free)\w*\s*\(", src)
    body = src[src.index('extern "C" int ' + NAME):]
    # (its first statement takes everything armed, and it serves none of it but the recorder: test_host_logic.py states the rule)
    from test_host_logic import chain_entries
    assert chain_entries()[NAME]["serves"] == set()
    work = ("hipLaunchKernelGGL", "hipMemcpy", "hipStreamSynchronize", "chain_stream(", "ddim_tables1(", "run_chain_with_recovery(")
    first_work = min(body.index(k) for k in work)
    assert max(body.rindex(k) for k in ("REQUIRE(", "_refuse(", "refuse_all_but(", "rec_begin(")) < first_work
    assert "run_chain_with_recovery" in body and "loop_steps(" in body and "rec_done(" in body
