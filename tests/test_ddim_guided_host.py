"""Guided DDIM with the built-in point objective as one library chain, host side (no GPU): the C entry is declared, exported and
bound, and ``GaussianDiffusion1D.ddim_sample`` routes to it exactly when ``design_fn`` is a ``PointObjective`` whose descriptor
exists for the guidance, the guidance carries ``-recurrence-N`` (N >= 1) and ``last_n_step <= L``.  Every other combination keeps
the Python loop (or its refusal).

The routing tests replace the library call by a recording stub and everything that would touch a device by a stand-in: what is
tested is which entry ``ddim_sample`` reaches and with which schedule."""
import contextlib
import ctypes as C
import os
import re

import pytest
import torch

import cindm_amd
from cindm_amd import _ffi
from test_ddim_guided_2d_host import WORK, _chunks, _with_helpers
from test_host_logic import chain_entries

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "cindm_ddpm1d_sample_ddim_guided"
HZ, F, B, S = 24, 8, 2, 10


def test_symbol_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "cindm_hip.h")).read()
    assert re.search(r"\bint\s+" + NAME + r"\s*\(", hdr)
    assert NAME in _ffi.SIGNATURES
    L = _ffi.lib()
    fn = getattr(L, NAME)
    assert fn.restype is C.c_int and len(fn.argtypes) == 24
    assert L.cindm_abi_version() == _ffi.ABI_VERSION
    # argument checks come before any device work: a null handle is refused with the reason
    assert fn(*([None] * 7 + [1, None, None, None, None, 0, 0, None, 0, None, None, 0, 1, None, 0, None, 0])) != 0
    assert b"null argument" in L.cindm_last_error()


ENTRIES = ("cindm_ddpm1d_sample", "cindm_ddpm1d_sample_ddim", "cindm_ddpm1d_sample_autoregress", "cindm_ddpm1d_sample_ula",
           "cindm_ddpm1d_sample_guided", NAME)


def test_entry_allocates_nothing():
    """The x_T snapshot, the DDIM tables and the second state buffer are slices of the caller's workspace, laid out once per call
    by Chain1D; every refusal of an entry stands before its first launch, copy or synchronise.  Stated over each of the six 1-D
    entries and, transitively, the helpers of its file (ddpm1d_host.inc) that it names."""
    csrc = os.path.join(ROOT, "cindm_amd", "csrc")
    chunks = _chunks(open(os.path.join(csrc, "ddpm1d_host.inc")).read())
    driver = _chunks(open(os.path.join(csrc, "chain_host.inc")).read())
    for entry in ENTRIES:
        used = _with_helpers(chunks, entry)
        everything = "\n".join(used.values())
        assert not re.search(r"\bhip(Malloc|Free)\w*\s*\(", everything), entry
        # the entry: its last refusal (a REQUIRE of its own or a refusal function) stands before its first work
        body = used[entry]
        assert "chain_stream(" in body
        first_work = min(body.index(k) for k in WORK if k in body)
        assert max(body.rindex(k) for k in ("REQUIRE(", "_refuse(") if k in body) < first_work, entry
        # (that the call consumes what was armed however it ends: test_host_logic.py::test_every_chain_entry_takes_everything_armed)
        assert "chain1_refuse(" in body and "step1_refuse(" in used["chain1_refuse"]
        assert ("guided_refuse(" in body) == entry.endswith("guided") == ("kServesTables" in chain_entries()[entry]["serves"])
        # the chain runs under run_chain_with_recovery through replay_steps
        assert "run_chain_with_recovery" in used and "replay_steps" in used, entry
        assert "body()" in used["run_chain_with_recovery"]
    # the refusal functions themselves, the recorder's check and the design tables' issue no work
    for k in ("step1_refuse", "chain1_refuse", "guided_refuse"):
        assert not any(w in chunks[k] for w in WORK), k
    for k in ("rec_begin", "design_begin", "design_refuse", "refuse_all_but"):
        assert not any(w in driver[k] for w in WORK), k
    # one layout per call: Chain1D's constructor computes it, the size query is the only other caller
    callers = sorted(k for k, v in chunks.items() if k != "step_layout" and "step_layout(" in v)
    assert callers == ["Chain1D", "cindm_ddpm1d_workspace_bytes"]
    assert "".join(chunks.values()).count("step_layout(") == 3


# ------------------------------------------------------------------ routing
class _OnDevice(torch.Tensor):
    """A CPU tensor that claims to live on the device: the host logic is what is tested."""
    device = property(lambda self: torch.device("cuda", 0))


def _floats(p, n):
    return torch.tensor([C.cast(p, C.POINTER(C.c_float))[i] for i in range(n)])


class _FakeLib:
    """Records the arguments of the new entry; what they point to is copied while the call is alive (``peek``: argument
    index -> number of floats)."""

    def __init__(self):
        self.calls, self.schedules, self.peek, self.peeked = [], [], {}, {}

    def cindm_ddpm1d_sample_ddim_guided(self, *a):
        self.calls.append(a)
        n_steps = a[7]
        self.schedules.append((n_steps, list(a[8]), _floats(a[9], 3 * n_steps).reshape(n_steps, 3)))
        self.peeked = {i: _floats(a[i], n) for i, n in self.peek.items()}
        return 0

    def __getattr__(self, name):
        raise AssertionError(f"the routing test reached another library entry: {name}")


@pytest.fixture
def rig(monkeypatch):
    m = cindm_amd.TemporalUnet1D(HZ, F, False, attention=True)
    d = cindm_amd.GaussianDiffusion1D(m, image_size=HZ, conditioned_steps=0, timesteps=1000, sampling_timesteps=S,
                                      loss_type="l1", ddim_sampling_eta=0.3)
    d._buffers["betas"] = d._buffers["betas"].as_subclass(_OnDevice)
    assert d.betas.device.type == "cuda"
    lib = _FakeLib()
    monkeypatch.setattr(_ffi, "lib", lambda: lib)
    monkeypatch.setattr(_ffi, "current_stream", lambda device: None)
    monkeypatch.setattr(torch.cuda, "device", lambda dev: contextlib.nullcontext())
    monkeypatch.setattr(d, "_init_state", lambda shape, *a, **k: torch.zeros(shape))
    monkeypatch.setattr(d, "_f32", lambda t, device=None: None if t is None else t.detach().float().contiguous())

    def fake_chain(img, desc, call, result=None):
        call(C.c_void_p(1), None, torch.zeros(256, dtype=torch.uint8))
        return img
    monkeypatch.setattr(d, "_chain", fake_chain)
    monkeypatch.setattr(d, "_timed_out", lambda desc, device: False)
    python_route = []

    def fake_guided_step(x, cond, t, desc, design_fn, design_guidance, iso, noise, recur_noise, ddim_return=False, check=True):
        python_route.append((t, design_guidance))
        return torch.zeros_like(x), torch.zeros_like(x)
    monkeypatch.setattr(d, "_guided_step", fake_guided_step)
    return d, lib, python_route


def _objective(n=2, cls=cindm_amd.PointObjective):
    return cls([0.25, -0.5], n, coef=5.0)


def test_point_objective_with_recurrence_reaches_the_library_chain(rig):
    d, lib, python_route = rig
    out = d.ddim_sample((B, HZ, F), None, n_composed=0, compose_mode="mean-inside", design_fn=_objective(),
                        design_guidance="standard-recurrence-2", seed=3, sample_offset=5)
    assert tuple(out.shape) == (B, HZ, F) and len(lib.calls) == 1 and not python_route
    call = lib.calls[0]
    times, coefs = d.ddim_schedule()
    n_steps, t_seen, c_seen = lib.schedules[0]
    assert n_steps == S and t_seen == times and len(times) == S + 1 and torch.equal(c_seen, coefs)
    dz = call[4]._obj
    assert (dz.mode, dz.alpha, dz.recurrence, dz.last_n_step) == (1, 0, 2, 2) and dz.coef == 5.0
    desc = call[3]._obj
    assert desc.mode == _ffi.COMPOSE_MEAN_INSIDE and desc.window == HZ and desc.n_windows == 1 and desc.clip_denoised == 1
    assert call[12].value == 3 and call[13] == 5 and call[19] == B and call[23] == 1
    assert call[10] is None and call[11] is None and call[14] is None and call[17] is None     # no tape, no inpainting, no overwrite


def test_step_range_slices_schedule_and_tapes(rig):
    d, lib, _ = rig
    g = torch.Generator().manual_seed(1)
    tape = cindm_amd.NoiseTape(torch.zeros((B, HZ, F)), torch.randn((S, B, HZ, F), generator=g),
                               torch.randn((S, 1, B, HZ, F), generator=g), torch.randn((S, B, 4, F), generator=g))
    tape.to = lambda device: tape
    cond = torch.rand((B, 4, F), generator=g)
    iso = torch.rand((B, 3, F), generator=g)
    n = B * HZ * F
    lib.peek = {10: n, 11: n, 16: B * 4 * F}
    d.ddim_sample((B, HZ, F), cond, n_composed=0, compose_mode="mean-inside", design_fn=_objective(),
                  design_guidance="standard-alpha-recurrence-1", initial_state_overwrite=iso, noise=tape,
                  init_img=torch.zeros((B, HZ, F)), step_range=(3, 7), use_graph=False)
    call = lib.calls[0]
    times, coefs = d.ddim_schedule()
    n_steps, t_seen, c_seen = lib.schedules[0]
    assert n_steps == 4 and t_seen == times[3:8] and torch.equal(c_seen, coefs[3:7])
    assert torch.equal(lib.peeked[10], tape.step[3].reshape(-1))              # tapes start at the segment's first step
    assert torch.equal(lib.peeked[11], tape.recur[3, 0].reshape(-1))
    assert torch.equal(lib.peeked[16], tape.cond[3].reshape(-1))
    assert call[15] == 4 and call[18] == 3 and call[23] == 0                  # inpaint rows, overwrite rows, use_graph
    assert call[4]._obj.alpha == 1 and call[4]._obj.recurrence == 1


@pytest.mark.parametrize("case", ["lambda", "universal", "last_n_step", "recurrence-0"])
def test_other_combinations_keep_the_python_loop(rig, monkeypatch, case):
    d, lib, python_route = rig
    obj = _objective()
    fn, guid = obj, "standard-recurrence-2"
    if case == "lambda":
        fn = lambda x: obj(x)
    elif case == "universal":
        guid = "universal-forward-recurrence-2"
    elif case == "last_n_step":
        fn = _objective(HZ + 1)
    else:
        guid = "standard-recurrence-0"
    tape = cindm_amd.NoiseTape(torch.zeros((B, HZ, F)), torch.zeros((S, B, HZ, F)), torch.zeros((S, 2, B, HZ, F)))
    tape.to = lambda device: tape
    orig_to = torch.Tensor.to

    def to(self, *a, **k):               # the Python loop moves its coefficient table to the "device"
        return self if (a and isinstance(a[0], torch.device) and a[0].type == "cuda") else orig_to(self, *a, **k)
    monkeypatch.setattr(torch.Tensor, "to", to)
    out = d.ddim_sample((B, HZ, F), None, n_composed=0, compose_mode="mean-inside", design_fn=fn, design_guidance=guid,
                        noise=tape)
    assert tuple(out.shape) == (B, HZ, F)
    assert not lib.calls and [t for t, _ in python_route] == d.ddim_schedule()[0][:-1]
    assert all(g == guid for _, g in python_route)


def test_guidance_without_recurrence_is_still_refused(rig):
    d, lib, python_route = rig
    with pytest.raises(NotImplementedError, match="recurrence"):
        d.ddim_sample((B, HZ, F), None, n_composed=0, design_fn=_objective(), design_guidance="standard", seed=0)
    assert not lib.calls and not python_route


def test_unguided_loop_is_untouched(rig, monkeypatch):
    d, lib, python_route = rig
    seen = []
    lib.cindm_ddpm1d_sample_ddim = lambda *a: seen.append(a) or 0
    d.ddim_sample((B, HZ, F), None, n_composed=0, seed=0)
    assert len(seen) == 1 and not lib.calls and not python_route


def test_sample_reaches_it_through_ddim_sample(rig):
    d, lib, _ = rig
    d.sample(batch_size=B, n_composed=0, compose_mode="mean-inside", design_fn=_objective(),
             design_guidance="standard-recurrence-3", seed=1, t_stop=5)
    assert len(lib.calls) == 1 and lib.calls[0][4]._obj.recurrence == 3
