"""Replacement conditioning of the 2-D chains (``known=`` / ``known_mask=`` / ``cond=``; cindm_ddpm1d_set_known2d), host side
(no GPU): the C entry is declared, bound and exported; ``GaussianDiffusion.known_replace`` IS the definition
    x[m] = sqrt_alphas_cumprod[t] k + sqrt_one_minus_alphas_cumprod[t] z   (t >= 0),     x[m] = k   (t < 0)
(compared bit for bit: the helper and the expression are the same three fp32 operations); the refusals are ValueErrors raised
before any device work (the diffusion here lives on the CPU: a call that passed them would end in CindmError); the shard slicing."""
import ctypes as C
import os
import re

import pytest
import torch

import cindm_amd
import cindm_oracle as O
from cindm_amd import _ffi, dist as cdist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "cindm_ddpm1d_set_known2d"
SHAPE = (2, 2, 21, 8, 8)          # the helper is shape-agnostic: small images keep the CPU test quick


@pytest.fixture(scope="module")
def unet():
    m = cindm_amd.Unet(dim=64, dim_mults=(1, 2), channels=21)
    m.load_state_dict(O.synth_state_dict_2d(O.unet2d_param_shapes(64, (1, 2), 21), 0), strict=True)
    return m


def _diffusion(unet, **kw):
    kw.setdefault("cond_frames", 2)
    return cindm_amd.GaussianDiffusion(unet, image_size=64, frames=6, timesteps=1000, **kw)


def test_entry_is_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "cindm_hip.h")).read()
    assert re.search(r"int\s+" + NAME + r"\(cindm_ddpm1d\* h, const float\* known, const uint8_t\* mask,", header)
    assert re.search(r"#define\s+CINDM_ABI_VERSION\s+4\b", header)
    assert NAME in _ffi.SIGNATURES and len(_ffi.SIGNATURES[NAME][1]) == 12
    L = _ffi.lib()
    assert L.cindm_abi_version() == _ffi.ABI_VERSION == 4
    fn = getattr(L, NAME)
    assert fn.restype is C.c_int and len(fn.argtypes) == 12
    buf = (C.c_float * 16)()
    assert fn(None, buf, buf, None, None, None, None, 0, 0, 1, 4, 4) != 0
    assert b"null handle" in L.cindm_last_error()
    assert fn(None, None, None, None, None, None, None, 0, 0, 0, 0, 0) != 0          # disarming needs a handle too
    assert L.cindm_last_error()


def test_every_chain_entry_takes_the_region():
    """Every chain entry takes the armed region with everything else that is armed (test_host_logic.py states that rule); the four 2-D
    entries check it before their first work, the 1-D entries do not serve it: refuse_all_but refuses it for them."""
    from test_host_logic import chain_entries
    csrc = os.path.join(ROOT, "cindm_amd", "csrc")
    two = open(os.path.join(csrc, "ddpm2d_host.inc")).read()
    entries = chain_entries()
    begin = re.compile(r"known2_begin\(took, ch, x, z\) != 0\) return -1;\n    if \(chain_stream\(")
    began = sorted(k for k, v in entries.items() if begin.search(v["body"]))
    assert began == sorted(k for k, v in entries.items() if v["file"] == "ddpm2d_host.inc") and len(began) == 4
    assert sum("kServesKnown2" not in v["serves"] for v in entries.values()) == 7
    assert all(("kServesKnown2" in v["serves"]) == (k in began) for k, v in entries.items())
    assert two.count("known2_node(ch, x, 0)") == 2 and two.count("known2_node(ch, x, 1)") == 1


def _case(seed, shape=SHAPE):
    B, nb, Cc, H, W = shape
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=g)
    k = torch.rand(shape, generator=g) * 2 - 1
    k[:, :, :-3] = k[:, :1, :-3]
    m = torch.rand((B, 1, Cc, H, W), generator=g) > 0.5
    m = m.expand(shape).clone()
    m[:, :, -3:] = torch.rand((B, nb, 3, H, W), generator=g) > 0.5          # the boundary channels may differ per image
    zs, zb = torch.randn((B, 1, Cc - 3, H, W), generator=g), torch.randn((B, nb, 3, H, W), generator=g)
    return x, k, m, zs, zb


@pytest.mark.parametrize("t", [999, 517, 0, -1])
def test_helper_is_the_definition(unet, t):
    """Rule 1 (t = t0 = 999 with the init draw), a step with t_next >= 0 (517, 0) and the last one (t_next = -1)."""
    d = _diffusion(unet)
    B, nb, Cc, H, W = SHAPE
    x, k, m, zs, zb = _case(3 + max(t, 0))
    assert bool(m.any()) and not bool(m.all())
    got = d.known_replace(SHAPE, x.reshape(B * nb, Cc, H, W), k, m, t, (zs, zb))
    assert got.shape == (B * nb, Cc, H, W)
    got = got.reshape(SHAPE)
    z = torch.cat([zs.expand(-1, nb, -1, -1, -1), zb], dim=2)          # the state draw: once per design
    want = k if t < 0 else d.sqrt_alphas_cumprod[t] * k + d.sqrt_one_minus_alphas_cumprod[t] * z
    assert torch.equal(got[m], want[m]) and torch.equal(got[~m], x[~m])
    if t >= 0:
        assert not torch.equal(got[m], k[m])
    # the state channels of the region stay shared over the boundary copies; its boundary channels do not
    sm = m[:, 0, :-3]
    assert torch.equal(got[:, 0, :-3][sm], got[:, 1, :-3][sm])
    if t >= 0:
        both = m[:, 0, -3:] & m[:, 1, -3:]
        assert not torch.equal(got[:, 0, -3:][both], got[:, 1, -3:][both])
    # a full tensor z is taken as it is; a mask that broadcasts is broadcast
    assert torch.equal(d.known_replace(SHAPE, x, k, m, t, z), got)
    row = torch.zeros((1, 1, Cc, 1, 1), dtype=torch.bool)
    row[:, :, :6] = True
    g2 = d.known_replace(SHAPE, x, k, row, t, z)
    assert torch.equal(g2[:, :, :6], want[:, :, :6]) and torch.equal(g2[:, :, 6:], x[:, :, 6:])


def test_helper_draws_state_channels_once_per_design(unet):
    """z = None: the helper draws like sample_noise -- with everything known at a level with noise, the state channels of the two
    boundary copies of a design are the same numbers, their boundary channels are not."""
    d = _diffusion(unet)
    x, k, m, _, _ = _case(11)
    torch.manual_seed(5)
    got = d.known_replace(SHAPE, x, k, torch.ones((), dtype=torch.bool), 700)
    assert torch.equal(got[:, 0, :-3], got[:, 1, :-3]) and not torch.equal(got[:, 0, -3:], got[:, 1, -3:])
    assert not torch.equal(got[0, 0, :-3], got[1, 0, :-3])
    kz = (got - d.sqrt_alphas_cumprod[700] * k) / d.sqrt_one_minus_alphas_cumprod[700]          # the draw: unit variance
    assert 0.9 < float(kz.std()) < 1.1


def test_region_from_cond_and_known(unet):
    d = _diffusion(unet)                      # cond_frames = 2: six channels
    B, nb, Cc, H, W = shape = (2, 2, 21, 64, 64)
    g = torch.Generator().manual_seed(1)
    cond = torch.rand((B, 6, H, W), generator=g)
    k, m = d._known_region(shape, None, None, cond)
    assert tuple(k.shape) == shape and m.dtype == torch.bool
    assert bool(m[:, :, :6].all()) and not bool(m[:, :, 6:].any())
    assert torch.equal(k[:, 0, :6], cond) and torch.equal(k[:, 1, :6], cond)
    known = torch.rand(shape, generator=g)
    km = torch.zeros(shape, dtype=torch.bool)
    km[0, 1, -3:] = True                      # one boundary image
    k, m = d._known_region(shape, known, km, cond)
    assert bool(m[:, :, :6].all()) and bool(m[0, 1, -3:].all()) and int(m.sum()) == B * nb * 6 * H * W + 3 * H * W
    assert torch.equal(k[0, 1, -3:], known[0, 1, -3:]) and torch.equal(k[:, 1, :6], cond)
    assert d._known_region(shape, None, None, None) is None


def _tape(shape, rows, **known):
    B, nb, Cc, H, W = shape
    z = lambda *s: torch.zeros(s)
    return cindm_amd.NoiseTape2D((z(B, 1, Cc - 3, H, W), z(B, nb, 3, H, W)), z(rows, B, 1, Cc - 3, H, W), z(rows, B, nb, 3, H, W), **known)


def test_refusals_are_value_errors_before_any_device_work(unet):
    """The diffusion is on the CPU: a call that passes the host checks ends in CindmError (no CPU execution path), so a ValueError
    here was raised before the device was looked at."""
    B, nb, Cc, H, W = shape = (1, 2, 21, 64, 64)
    g = torch.Generator().manual_seed(2)
    known = torch.rand(shape, generator=g)
    known[:, :, :-3] = known[:, :1, :-3]
    ok = torch.zeros(shape, dtype=torch.bool)
    ok[:, :, 18:] = True
    cond = torch.rand((B, 6, H, W), generator=g)
    for d, call in ((_diffusion(unet), lambda d, **kw: d.p_sample_loop(shape, **kw)),
                    (_diffusion(unet, sampling_timesteps=50), lambda d, **kw: d.ddim_sample(shape, **kw)),
                    (_diffusion(unet, sampling_timesteps=50), lambda d, **kw: d.sample(batch_size=B, num_boundaries=nb, **kw))):
        with pytest.raises(cindm_amd.CindmError) as e:                      # the good call: through the checks, then no device
            call(d, known=known, known_mask=ok, cond=cond)
        assert not isinstance(e.value, ValueError)
        # shapes that do not broadcast
        with pytest.raises(ValueError, match="broadcast"):
            call(d, known=known, known_mask=torch.zeros((1, 3, Cc, H, W), dtype=torch.bool))
        with pytest.raises(ValueError, match="broadcast"):
            call(d, known=known, known_mask=torch.zeros((Cc + 1, H, W), dtype=torch.bool))
        with pytest.raises(ValueError, match="shape of the state"):
            call(d, known=known[:, :1], known_mask=ok)
        with pytest.raises(ValueError, match="cond must be"):
            call(d, cond=cond[:, :3])
        with pytest.raises(ValueError):
            call(d, known=known)                                            # values without a mask
        with pytest.raises(ValueError):
            call(d, known_mask=ok)                                          # a mask without values
        with pytest.raises(ValueError, match="bool"):
            call(d, known=known, known_mask=ok.float())
        # state channels that differ over the boundary copies: the mask, then the values
        bad = ok.clone()
        bad[0, 1, 7, 3, 3] = True
        with pytest.raises(ValueError, match="identical over the boundary copies"):
            call(d, known=known, known_mask=bad)
        both = ok.clone()
        both[:, :, 7] = True
        call_ok = pytest.raises(cindm_amd.CindmError)
        with call_ok:
            call(d, known=known, known_mask=both)
        kv = known.clone()
        kv[0, 1, 7, 3, 3] += 0.5
        with pytest.raises(ValueError, match="identical over the boundary copies"):
            call(d, known=kv, known_mask=both)
        kv = known.clone()
        kv[0, 1, 2, 3, 3] += 0.5                                           # ... outside the mask the values are not read
        with pytest.raises(cindm_amd.CindmError) as e:
            call(d, known=kv, known_mask=both)
        assert not isinstance(e.value, ValueError)
        # cond= on channels known= names too
        over = ok.clone()
        over[:, :, 5] = True
        with pytest.raises(ValueError, match="same channels"):
            call(d, known=known, known_mask=over, cond=cond)
        # tape rows: missing, or of the wrong shape
        rows = 1000 if not d.is_ddim_sampling else 50
        with pytest.raises(ValueError, match="known_init"):
            call(d, cond=cond, noise=_tape(shape, rows))
        z = lambda *s: torch.zeros(s)
        good = dict(known_init=(z(B, 1, Cc - 3, H, W), z(B, nb, 3, H, W)), known_state=z(rows, B, 1, Cc - 3, H, W),
                    known_boundary=z(rows, B, nb, 3, H, W))
        with pytest.raises(cindm_amd.CindmError) as e:
            call(d, cond=cond, noise=_tape(shape, rows, **good))
        assert not isinstance(e.value, ValueError)
        for key, wrong in (("known_init", (z(B, nb, Cc - 3, H, W), z(B, nb, 3, H, W))), ("known_state", z(rows, B, nb, Cc - 3, H, W)),
                           ("known_boundary", z(rows, B, 1, 3, H, W)), ("known_state", z(rows - 1, B, 1, Cc - 3, H, W)),
                           ("known_boundary", z(B, nb, 3, H, W))):
            with pytest.raises(ValueError, match="known_init"):
                call(d, cond=cond, noise=_tape(shape, rows, **dict(good, **{key: wrong})))


class _Recorder:
    def __init__(self):
        self.calls = []

    def sample(self, **kw):
        self.calls.append(kw)
        return torch.zeros((kw["batch_size"], kw["num_boundaries"], 21, 4, 4))


def test_shard_slicing():
    B, nb, Cc, H, W = shape = (7, 2, 21, 4, 4)
    g = torch.Generator().manual_seed(4)
    known, cond = torch.rand(shape, generator=g), torch.rand((B, 6, H, W), generator=g)
    per_design = torch.rand(shape, generator=g) > 0.5
    shared = torch.rand((1, nb, Cc, H, W), generator=g) > 0.5
    seen = []
    for rank in range(3):
        lo, hi = cdist.shard_bounds(B, rank, 3)
        kw = cdist.shard_known2d(dict(known=known, known_mask=per_design, cond=cond, t_stop=995), B, lo, hi)
        assert torch.equal(kw["known"], known[lo:hi]) and torch.equal(kw["cond"], cond[lo:hi])
        assert torch.equal(kw["known_mask"], per_design[lo:hi]) and kw["t_stop"] == 995
        kw = cdist.shard_known2d(dict(known=known, known_mask=shared), B, lo, hi)
        assert kw["known_mask"] is shared and "cond" not in kw
        seen += list(range(lo, hi))
    assert seen == list(range(B))
    assert cdist.shard_known2d(dict(fused=False), B, 0, 3) == dict(fused=False)
    with pytest.raises(ValueError, match="designs"):
        cdist.shard_known2d(dict(cond=cond[:3]), B, 0, 3)
    # through sample2d_sharded (no process group: one rank that holds every design)
    fake = _Recorder()
    out = cdist.sample2d_sharded(fake, B, seed=5, num_boundaries=nb, known=known, known_mask=per_design, cond=cond)
    assert tuple(out.shape) == (B, nb, 21, 4, 4)
    kw, = fake.calls
    assert (kw["batch_size"], kw["sample_offset"], kw["seed"]) == (B, 0, 5)
    assert torch.equal(kw["known"], known) and torch.equal(kw["known_mask"], per_design) and torch.equal(kw["cond"], cond)
