"""Guided 2-D DDIM with the airfoil objective as one library chain, host side (no GPU): the per-step guidance weights, the
dispatch of ``GaussianDiffusion.ddim_sample`` (a ``ForceObjective`` under "standard-alpha" passes the refusals and reaches the
device check; everything else is refused as before) and the C entry being declared, bound and exported."""
import ctypes as C
import os
import re

import pytest
import torch

import cindm_amd
import cindm_oracle as O
from cindm_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "cindm_ddpm2d_sample_ddim_force"


@pytest.fixture(scope="module")
def unet():
    m = cindm_amd.Unet(dim=64, dim_mults=(1, 2), channels=21)
    m.load_state_dict(O.synth_state_dict_2d(O.unet2d_param_shapes(64, (1, 2), 21), 0), strict=True)
    return m


def _diffusion(unet, **kw):
    return cindm_amd.GaussianDiffusion(unet, image_size=64, frames=6, timesteps=1000, **kw)


def _objective(B=1, nb=2):
    m = cindm_amd.ForceUnet(dim=64, dim_mults=(1, 2, 4, 8), channels=4)          # (a handle and CPU parameters: no device needed)
    return cindm_amd.ForceObjective(m, B, nb, 6, p_min=-37.7, p_max=57.6)


@pytest.mark.parametrize("S", [5, 50, 250, 1000])
def test_guidance_weights(unet, S):
    d = _diffusion(unet, sampling_timesteps=S, coeff_ratio=0.05)
    w = d.ddim_guidance_weights()
    times, _ = d.ddim_schedule()
    eta = d.coeff_ratio * d.betas.flip(0)                      # the [T] table p_sample indexes for "standard-alpha"
    assert eta.dtype == torch.float32
    assert w.dtype == torch.float32 and tuple(w.shape) == (S,) and bool(torch.isfinite(w).all())
    if S == 1000:
        assert torch.equal(w, eta[times[:-1]])                 # strides of one step: the DDPM chain's own weight, bit for bit
    for i, (t, tn) in enumerate(zip(times[:-1], times[1:])):
        assert w[i] == eta.double()[tn + 1:t + 1].sum().float(), (i, t, tn)
    # the DDIM steps tile 0 .. T-1: the chain applies the DDPM chain's total guidance
    assert abs(float(w.double().sum()) - float(eta.double().sum())) <= 1e-6 * float(eta.double().sum())


def test_force_objective_passes_the_refusals_and_reaches_the_device_check(unet):
    d = _diffusion(unet, sampling_timesteps=50)
    fn = _objective()
    with pytest.raises(cindm_amd.CindmError) as e:
        d.sample(batch_size=1, num_boundaries=2, design_fn=fn, design_guidance="standard-alpha")
    assert not isinstance(e.value, NotImplementedError)
    with pytest.raises(cindm_amd.CindmError):
        d.ddim_sample((1, 2, 21, 64, 64), design_fn=fn, design_guidance="standard-alpha", fused=False)


def test_everything_else_is_still_refused(unet):
    d = _diffusion(unet, sampling_timesteps=50)
    fn = _objective()
    with pytest.raises(NotImplementedError, match="design_fn"):
        d.sample(batch_size=1, num_boundaries=2, design_fn=lambda x: torch.zeros_like(x), design_guidance="standard-alpha")
    with pytest.raises(NotImplementedError, match="design_fn"):
        d.sample(batch_size=1, num_boundaries=2, design_fn=fn, design_guidance="standard")
    with pytest.raises(NotImplementedError, match="design_fn"):
        d.sample(batch_size=1, num_boundaries=2, design_fn=fn, design_guidance="universal-forward")
    with pytest.raises(NotImplementedError, match="return_all_timesteps"):
        d.sample(batch_size=1, num_boundaries=2, design_fn=fn, design_guidance="standard-alpha", return_all_timesteps=True)
    with pytest.raises(NotImplementedError, match="share_noise"):
        _diffusion(unet, sampling_timesteps=50, share_noise=False).sample(batch_size=1, num_boundaries=2, design_fn=fn,
                                                                          design_guidance="standard-alpha")


def test_symbol_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "cindm_hip.h")).read()
    assert re.search(r"\bint\s+" + NAME + r"\s*\(", hdr)
    assert NAME in _ffi.SIGNATURES
    L = _ffi.lib()
    fn = getattr(L, NAME)
    assert fn.restype is C.c_int and len(fn.argtypes) == 31
    assert L.cindm_abi_version() == _ffi.ABI_VERSION
    # argument checks come before any device work: null handles are refused with the reason
    assert fn(*([None] * 4 + [1, 2, 1, 1] + [None] * 4 + [0, None, None, 0, 0, 6, 0.0, 1.0, 1.0, 1.0, 4, 1, None, None, 0, None, 0, None, 1])) != 0
    assert b"null argument" in L.cindm_last_error()


def _chunks(src):
    """name -> text of every top-level function and struct of a host file, comments stripped (a chunk runs from a line that
    starts in column 0 to the next line that starts with '}'; one-line declarations that end with ';' are not chunks)."""
    out, lines, i = {}, [re.sub(r"//.*", "", ln).rstrip() for ln in src.split("\n")], 0
    while i < len(lines):
        ln = lines[i]
        if not ln or ln[0].isspace() or ln[0] in "}#" or ln.endswith(";"):
            i += 1
            continue
        j = i
        while not (lines[j].startswith("}") or (j == i and ln.endswith("}"))):
            j += 1
        text = "\n".join(lines[i:j + 1])
        head = re.sub(r"^template\s*<[^>]*>\s*", "", text)
        m = re.match(r"struct\s+(\w+)", head) or re.search(r"(\w+)\s*\(", head)
        out[m.group(1)] = text
        i = j + 1
    return out


def _with_helpers(chunks, name):
    """The entry `name` and every function / struct of the same file that it names, transitively."""
    seen, todo = {}, [name]
    while todo:
        n = todo.pop()
        if n in seen:
            continue
        seen[n] = chunks[n]
        todo += [k for k in chunks if k not in seen and re.search(r"\b" + k + r"\b", chunks[n])]
    return seen


WORK = ("chain_stream(", "upload_ddim_tables(", "hipLaunchKernelGGL", "hipMemcpyAsync", "hipMemsetAsync")


def test_entry_allocates_nothing_and_checks_before_it_launches():
    """The x_T snapshot is a slice of the caller's diffusion workspace and the tables live in the caller's buffer; every refusal
    of the entry's own stands before its first launch or copy.  Stated over the entry and the static helpers of its file
    (ddpm2d_host.inc) that it calls; the guided DDPM entry refuses before its first work in the same way."""
    for entry in (NAME, "cindm_ddpm2d_sample_force"):
        _check_entry(entry)


def _check_entry(entry):
    chunks = _chunks(open(os.path.join(ROOT, "cindm_amd", "csrc", "ddpm2d_host.inc")).read())
    used = _with_helpers(chunks, entry)
    everything = "\n".join(used.values())
    assert not re.search(r"\bhip(Malloc|Free)\w*\s*\(", everything)
    # the entry: its last refusal (a REQUIRE of its own or a refusal function) stands before its first work; the refusal functions
    # themselves, and the recorder's check, issue none
    body = used[entry]
    first_work = min(body.index(k) for k in WORK if k in body)
    assert "chain_stream(" in body and "run_chain2(" in body
    assert max(body.rindex(k) for k in ("REQUIRE(", "_refuse(") if k in body) < first_work < body.index("run_chain2(")
    assert "chain2_refuse(" in body and "force_refuse(" in body
    for k in ("step2_refuse", "chain2_refuse", "force_refuse", "rec_begin2"):
        assert not any(w in used[k] for w in WORK), k
    # the chain runs under force_chain_with_recovery through replay_once
    tail = used["run_chain2"]
    assert "force_chain_with_recovery(" in tail and "replay_once(" in tail
    assert "chain()" in used["force_chain_with_recovery"]
    # the one call of the objective, on the chain's x
    assert everything.count("cindm_airfoil_design_grad(") == 1
    if entry == NAME:
        # the guided DDIM step: the shift is part of the update, not a second pass
        assert "ddim_step2" in used and "ddpm_step2" not in used
        assert "ddim2d_guided_update_kernel" in used["run_ddim_step2"]
        assert "guided_shift2d_kernel" not in everything
    else:
        assert "ddpm_step2" in used and "guided_shift2d_kernel" in used["ddpm_step2"]
