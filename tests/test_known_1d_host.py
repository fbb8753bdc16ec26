"""Replacement conditioning of the 1-D chains (``known=`` / ``known_mask=``; cindm_ddpm1d_set_known1d), host side
(no GPU): the C entry is declared, bound and exported; ``GaussianDiffusion1D.known_replace`` IS the definition
    x[m] = sqrt_alphas_cumprod[l] k + sqrt_one_minus_alphas_cumprod[l] z   (l >= 0),     x[m] = k   (l < 0)
(compared bit for bit: the helper and the expression are the same three fp32 operations); the refusals are ValueErrors raised
before any device work (the diffusion here lives on the CPU: a call that passed them ends in CindmError); the two methods that
do not hold a region; the tape's positional construction; the shard slicing."""
import ctypes as C
import os
import re

import pytest
import torch

import cindm_amd
from cindm_amd import _ffi, dist as cdist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "cindm_ddpm1d_set_known1d"
B, L, F = 3, 24, 8


@pytest.fixture(scope="module")
def diff():
    m = cindm_amd.TemporalUnet1D(L, F, False, attention=True)
    return cindm_amd.GaussianDiffusion1D(m, image_size=L, conditioned_steps=0, timesteps=1000, sampling_timesteps=1000, loss_type="l1")


@pytest.fixture(scope="module")
def diff_ddim():
    m = cindm_amd.TemporalUnet1D(L, F, False, attention=True)
    return cindm_amd.GaussianDiffusion1D(m, image_size=L, conditioned_steps=0, timesteps=1000, sampling_timesteps=4, loss_type="l1")


def test_entry_is_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "cindm_hip.h")).read()
    assert re.search(r"int\s+" + NAME + r"\(cindm_ddpm1d\* h, const float\* known, int32_t known_per_design,", header)
    assert re.search(r"#define\s+CINDM_ABI_VERSION\s+4\b", header)
    assert NAME in _ffi.SIGNATURES and len(_ffi.SIGNATURES[NAME][1]) == 14
    lib = _ffi.lib()
    assert lib.cindm_abi_version() == _ffi.ABI_VERSION == 4
    fn = getattr(lib, NAME)
    assert fn.restype is C.c_int and len(fn.argtypes) == 14
    buf = (C.c_float * 16)()
    assert fn(None, buf, 0, buf, 0, None, None, 0, None, 0, 1, 1, 4, 4) != 0
    assert b"null handle" in lib.cindm_last_error()
    assert fn(None, None, 0, None, 0, None, None, 0, None, 0, 1, 0, 0, 0) != 0          # disarming needs a handle too
    assert lib.cindm_last_error()


def test_every_chain_entry_takes_the_region():
    """Every chain entry takes the armed region with everything else that is armed (test_host_logic.py states that rule); four 1-D
    entries check it before their first work and run it, the rollout, the Langevin chain, the time composition and the 2-D entries
    refuse it with the reason."""
    from test_host_logic import chain_entries
    entries = chain_entries()
    one = {k: v for k, v in entries.items() if v["file"] == "ddpm1d_host.inc"}
    two = {k: v for k, v in entries.items() if v["file"] == "ddpm2d_host.inc"}
    assert len(one) == 6 and len(two) == 4
    begin = re.compile(r"known1_begin\(took, ch, x, [^;]*\) != 0\) return -1;\n    if \(chain_stream\(")
    assert sorted(k for k, v in entries.items() if begin.search(v["body"])) == sorted(k for k, v in one.items() if "kServesKnown1" in v["serves"])
    assert sum("kServesKnown1" in v["serves"] for v in one.values()) == 4
    # the others hand refuse_all_but their reason: two 1-D entries of that file, the time composition and the four 2-D entries
    reason = lambda v: re.search(r"took\.refuse_all_but\([^,)]*, (\"|kKnown1Not2D\))", v["body"]) is not None
    assert sum(reason(v) for v in one.values()) == 2 and sum(reason(v) for v in two.values()) == 4
    assert all(reason(v) != ("kServesKnown1" in v["serves"]) for v in entries.values())


def _case(seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((B, L, F), generator=g)
    k = torch.rand((B, L, F), generator=g) * 2 - 1
    m = torch.rand((B, L, F), generator=g) > 0.5
    z = torch.randn((B, L, F), generator=g)
    return x, k, m, z


@pytest.mark.parametrize("level", [999, 517, 0])
def test_helper_is_the_definition_on_a_level(diff, level):
    x, k, m, z = _case(level)
    got = diff.known_replace(x, k, m, level, z)
    q = diff.sqrt_alphas_cumprod[level] * k + diff.sqrt_one_minus_alphas_cumprod[level] * z
    assert torch.equal(got, torch.where(m, q, x))
    assert torch.equal(got[~m], x[~m]) and not torch.equal(got[m], x[m]) and got is not x
    # values and mask shared by all designs broadcast
    got = diff.known_replace(x, k[0], m[0], level, z)
    q = diff.sqrt_alphas_cumprod[level] * k[:1].expand(B, L, F) + diff.sqrt_one_minus_alphas_cumprod[level] * z
    assert torch.equal(got, torch.where(m[:1].expand(B, L, F), q, x))


def test_helper_returns_the_clean_values_below_level_zero(diff):
    x, k, m, z = _case(5)
    got = diff.known_replace(x, k, m, -1, z)
    assert torch.equal(got, torch.where(m, k, x)) and torch.equal(got[m], k[m])
    assert torch.equal(diff.known_replace(x, k, m, -1), got)          # (no draw is made)


def test_helper_returns_x_itself_for_an_empty_mask(diff):
    x, k, m, z = _case(6)
    assert diff.known_replace(x, k, torch.zeros_like(m), 300, z) is x
    assert diff.known_replace(x, k, torch.zeros((L, F), dtype=torch.bool), -1) is x


def _ok(fn):
    """The good call: through the checks, then no device."""
    with pytest.raises(cindm_amd.CindmError) as e:
        fn()
    assert "CPU" in str(e.value)


@pytest.mark.parametrize("which", ["ddpm", "ddim"])
def test_refusals_are_value_errors_before_any_device_work(diff, diff_ddim, which):
    d = diff if which == "ddpm" else diff_ddim
    x, k, m, z = _case(7)
    m[:, :4] = False                                                      # rows 0 .. 3 stay free for cond / overwrite below
    run = lambda **kw: d.sample(batch_size=B, n_composed=0, **kw)
    _ok(lambda: run(known=k, known_mask=m))
    _ok(lambda: run(known=k[0], known_mask=m[0]))                          # shared by all designs
    _ok(lambda: run(known=k, known_mask=m[0, :, :1]))                      # a mask that broadcasts
    with pytest.raises(ValueError, match="known_mask without known"):
        run(known_mask=m)
    with pytest.raises(ValueError, match="needs known_mask"):
        run(known=k)
    with pytest.raises(ValueError, match="known must be"):
        run(known=k[:, :-1], known_mask=m)
    with pytest.raises(ValueError, match="known must be"):
        run(known=k[:2], known_mask=m)
    with pytest.raises(ValueError, match="broadcast"):
        run(known=k, known_mask=m[:, :-1])
    with pytest.raises(ValueError, match="broadcast"):
        run(known=k, known_mask=m[None])
    with pytest.raises(ValueError, match="bool"):
        run(known=k, known_mask=m.float())
    bad = k.clone()
    bad[1, 10, 3] = float("nan")
    mm = m.clone()
    mm[1, 10, 3] = True
    with pytest.raises(ValueError, match="non-finite"):
        run(known=bad, known_mask=mm)
    mm[1, 10, 3] = False
    _ok(lambda: run(known=bad, known_mask=mm))                             # (off the region the values are not read)
    # rule 5: rows claimed by cond inpainting or by initial_state_overwrite
    cond = torch.zeros((B, 4, F))
    _ok(lambda: run(known=k, known_mask=m, cond=cond))
    m3 = m.clone()
    m3[0, 3, 0] = True
    with pytest.raises(ValueError, match="cond"):
        run(known=k, known_mask=m3, cond=cond)
    obj = cindm_amd.PointObjective([0.1, 0.2], 2, coef=1.0)
    guided = dict(design_fn=obj, design_guidance="standard-recurrence-2", compose_mode="mean-inside")
    with pytest.raises(ValueError, match="initial_state_overwrite"):
        run(known=k, known_mask=m3, initial_state_overwrite=torch.zeros((B, 4, F)), **guided)
    # a built-in objective together with a region is allowed
    _ok(lambda: run(known=k, known_mask=m, **guided))
    wp = cindm_amd.WaypointObjective(torch.zeros((L, F // 4, 2)), torch.zeros((L, F // 4)))
    _ok(lambda: run(known=k, known_mask=m, **dict(guided, design_fn=wp)))
    # a tape needs the region's rows
    rows = 1000 if which == "ddpm" else 4
    tape = lambda **kw: cindm_amd.NoiseTape(z, torch.zeros((rows, B, L, F)), torch.zeros((rows, 2, B, L, F)), **kw)
    with pytest.raises(ValueError, match="known_init"):
        run(known=k, known_mask=m, noise=tape())
    with pytest.raises(ValueError, match="known_step"):
        run(known=k, known_mask=m, noise=tape(known_init=z, known_step=torch.zeros((rows - 1, B, L, F))))
    _ok(lambda: run(known=k, known_mask=m, noise=tape(known_init=z, known_step=torch.zeros((rows, B, L, F)))))
    with pytest.raises(ValueError, match="known_recur"):
        run(known=k, known_mask=m, noise=tape(known_init=z, known_step=torch.zeros((rows, B, L, F))), **guided)
    _ok(lambda: run(known=k, known_mask=m, noise=tape(known_init=z, known_step=torch.zeros((rows, B, L, F)),
                                                       known_recur=torch.zeros((rows, 2, B, L, F))), **guided))


def test_the_rollout_and_the_multibody_sampler_do_not_take_a_region(diff):
    x, k, m, z = _case(8)
    with pytest.raises(TypeError, match="known"):
        diff.autoregress_time_compose_sample(B, torch.zeros((B, 4, F)), 1, known=k, known_mask=m)
    with pytest.raises(TypeError, match="known"):
        diff.sample_compose_multibodies(torch.zeros((B, 4, 16)), 401, 0, 4, known=k, known_mask=m)


def test_noise_tape_positional_construction_is_unchanged():
    a, b, c, d_, e = (torch.zeros(1) + i for i in range(5))
    t = cindm_amd.NoiseTape(a, b, c, d_, e)
    assert (t.init, t.step, t.recur, t.cond, t.ula) == (a, b, c, d_, e)
    assert t.known_init is None and t.known_step is None and t.known_recur is None
    t = cindm_amd.NoiseTape(a, b)
    assert t.recur is None and t.cond is None and t.ula is None and t.known_init is None
    with pytest.raises(TypeError):
        cindm_amd.NoiseTape(a, b, c, d_, e, a)                            # the known rows are keyword-only
    t = cindm_amd.NoiseTape(a, b, known_init=c, known_step=d_, known_recur=e).to("cpu")
    assert torch.equal(t.known_init, c) and torch.equal(t.known_step, d_) and torch.equal(t.known_recur, e) and t.recur is None


def test_shard_slicing():
    x, k, m, z = _case(9)
    kw = cdist.shard_known1d(dict(known=k, known_mask=m, seed=1), B, 1, 3)
    assert torch.equal(kw["known"], k[1:3]) and torch.equal(kw["known_mask"], m[1:3]) and kw["seed"] == 1
    kw = cdist.shard_known1d(dict(known=k[0], known_mask=m[0]), B, 1, 3)              # shared tables pass through
    assert kw["known"] is not None and torch.equal(kw["known"], k[0]) and torch.equal(kw["known_mask"], m[0])
    kw = cdist.shard_known1d(dict(known=k, known_mask=m[:1]), B, 0, 1)                # a mask that broadcasts over the designs
    assert torch.equal(kw["known"], k[:1]) and torch.equal(kw["known_mask"], m[:1])
    kw = cdist.shard_known1d(dict(known=k, known_mask=m[0, :, :1]), B, 2, 3)
    assert torch.equal(kw["known"], k[2:3]) and torch.equal(kw["known_mask"], m[0, :, :1])
    assert cdist.shard_known1d(dict(seed=3), B, 0, 1) == dict(seed=3)
    with pytest.raises(ValueError, match="designs"):
        cdist.shard_known1d(dict(known=k, known_mask=m), B + 1, 0, 1)
