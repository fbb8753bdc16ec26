"""GPU (MI355X): the arithmetic between "the U-Net's output" and "the next state" of the 2-D sampling path -- update2d_kernel,
ddim2d_update_kernel, ddim2d_guided_update_kernel -- held to the float64 statement of oracle/f64_reference.py
(``step2d_predict_f64``, ``step2d_update_f64``) element by element, over the grid of tests/step2d_cases.py.

Per case: the state is seeded normal x 0.7 (its state channels shared over the boundary copies of a design in half of the cases); the
LIBRARY's U-Net gives E = model(x, t); the library entry under test runs on the same x; the float64 statement on E gives the
reference, the magnitudes A and the rounding counts n_e; asserted, on every element of every returned tensor,

    |got - ref|  <=  (n_e + 4) * 2^-24 * A_e                                  (f64_reference.step2d_bound)

The U-Net's own error is in E on both sides and cancels (``test_entry_sees_the_same_E``: the entry's forward is the model's, bit for
bit): a wrong copy, divisor, seam, clamp order or noise is an O(1) violation on the elements it touches, however few and however small
against the tensor's largest.  tests/test_step2d_f64_host.py proves the statement first (the fp32 oracle and the reference project's
own execution stay within the same bound; nine mutations leave it by more than 100 x).

update2d_kernel is reached through the raw C entries (``cindm_ddpm2d_step``: x_out, x0, mean, explicit noise; ``cindm_ddpm2d_predict``:
eps_out, x0) on output buffers filled with a sentinel, so the padding lanes c >= C are asserted to be written, and to hold 0, as well.
The DDIM kernels are reached through ``ddim_sample(init_img=, step_range=(i, i + 1), noise=tape)``; the guided one with
g = ForceObjective(x), the library's own entry on the step's input.

Shapes: 32 x 32 images; C = 21 (CP = 24: channel group 4 straddles the state / boundary seam, group 5 is one channel and three pads)
and C = 15 (CP = 16: the seam on a group boundary, one pad), each on the full grid; one 64 x 64 case per kernel; (B, nb) in
{(1, 1), (1, 2), (2, 3), (3, 2), (1, 5)}.  The U-Net serves 32 and 64 pixels only, so B * H * W *
CP / 4 threads are always a whole number of 256-thread blocks: the kernels' ``i < total`` guard cannot be reached from a served shape,
and no case is contorted to reach it.

The chain route reads t from device memory: a one-step ``p_sample_loop`` equals the step entry, and the whole chain of a 4-timestep
diffusion equals four step calls, bit for bit.

Measured on an MI355X (profiles/step2d_f64.json, 3390 cases): the largest ratio is 0.403 (the predict entry under pred_x0: the
re-derived pred_noise); the step entry <= 0.365, ddim2d_update_kernel <= 0.349, ddim2d_guided_update_kernel <= 0.339.  The grid found
no defect in the three kernels.  That it would: with ``update2d_kernel``'s share_noise-False branch reading copy 0's x for every copy
the three ``test_step_entry`` cases fail; with ``c0 < Cs`` in place of ``c < Cs`` where the shared prediction is picked (channels 18
and 19 of 21) ``test_step_entry`` and both ``test_predict_entry`` cases under pred_noise fail; with ``ddim2d_update_kernel`` dividing
the shared sum by nb when the sum is asked ``test_ddim_update[pred_noise]`` fails (scratch builds, not kept).

With CINDM_STEP2D_F64_JSON=<path> the module writes every case's largest err / bound with its output and element index, one line per
(entry, objective, C, size, B, nb) (profiles/step2d_f64.json is such a run; the summary at its head)."""
import json
import os

import pytest
import torch

import cindm_amd
import cindm_oracle as O
import f64_reference as R
import step2d_cases as S
from cindm_amd import _ffi
from cindm_amd.diffusion2d import _boundary_cl, _state_cl
from cindm_amd.unet2d import to_device_layout

pytestmark = pytest.mark.gpu

# A (case, output) that cannot hold the bound needs its derivation written next to it.  None taken.
EXCEPTIONS = {}

SENTINEL = 7.0              # what the raw entries' output buffers hold before the call: a lane the kernel does not write keeps it
_LOG = {}
TAB = {obj: O.make_schedule(S.BETA_SCHEDULE, 1000, obj) for obj in S.OBJECTIVES}
MULTS = {32: (1, 1), 64: (1, 2)}        # the served configurations of test_gpu_parity_2d.py::test_unet2d_other_configurations


@pytest.fixture(scope="module", autouse=True)
def _write_log():
    yield
    path = os.environ.get("CINDM_STEP2D_F64_JSON")
    if path and _LOG:
        flat = sorted(((v["ratio"], k) for k, v in _LOG.items()), reverse=True)
        by_kernel = {}
        for k, v in _LOG.items():
            by_kernel[k.split("/")[0]] = max(by_kernel.get(k.split("/")[0], 0.0), v["ratio"])
        # one line per (entry, objective, C, size, B, nb): {options: [ratio, output, element index]}
        groups = {}
        for k, v in _LOG.items():
            groups.setdefault(k.split(" ")[0], {})[k.split(" ")[1]] = [v["ratio"], v["output"], v["index"]]
        head = {"metric": "largest |got - ref| / ((n_e + 4) * 2^-24 * A_e) over the elements of every returned tensor; ref, A, n_e: "
                          "f64_reference.step2d_predict_f64 / step2d_update_f64 / step2d_roundings on the library's own U-Net output",
                "slack": R.BOUND_SLACK, "cases_run": len(_LOG), "largest": round(flat[0][0], 4), "largest_by_entry": by_kernel,
                "ten_largest": [dict(case=k, **_LOG[k]) for _, k in flat[:10]]}
        with open(path, "w") as f:
            f.write("{" + "".join(json.dumps(k) + ": " + json.dumps(v) + ",\n" for k, v in head.items()) + '"cases": {\n')
            f.write(",\n".join(json.dumps(g) + ": " + json.dumps(c) for g, c in groups.items()) + "\n}}\n")


_NETS, _DIFF, _E = {}, {}, {}


def _net(device, C, size):
    if (C, size) not in _NETS:
        sd = O.synth_state_dict_2d(O.unet2d_param_shapes(64, MULTS[size], C), 9)
        m = cindm_amd.Unet(dim=64, dim_mults=MULTS[size], channels=C, image_size=size)
        m.load_state_dict(sd, strict=True)
        _NETS[C, size] = m.to(device)
    return _NETS[C, size]


def _diff(device, C, size, obj, share=True, avg=True, S_ddim=None, eta=0.0, T=1000):
    key = (C, size, obj, share, avg, S_ddim, eta, T)
    if key not in _DIFF:
        _DIFF[key] = cindm_amd.GaussianDiffusion(_net(device, C, size), image_size=size, frames=(C - 3) // 3, cond_frames=2, timesteps=T,
                                                 sampling_timesteps=S_ddim, loss_type="l2", objective=obj, beta_schedule=S.BETA_SCHEDULE,
                                                 ddim_sampling_eta=eta, coeff_ratio=S.GUIDED_COEFF_RATIO, share_noise=share,
                                                 use_average_share=avg).to(device)
    return _DIFF[key]


def _state_and_E(device, C, size, B, nb, t, shared):
    """(x [B * nb, C, size, size] on the host, E = model(x, t) on the host): one forward per state, shared by every case on it."""
    key = (C, size, B, nb, t, shared)
    if key not in _E:
        x = S.make_state(C, B, nb, t, shared, size)
        _E[key] = (x, _net(device, C, size)(x.to(device), t).cpu())
    return _E[key]


def _cl(v):
    """[N, C, H, W] -> the library's [N, H * W, C]."""
    n, c, h, w = v.shape
    return v.permute(0, 2, 3, 1).reshape(n, h * w, c)


def _hold(tag, outs, C):
    """outs: {name: (got, ref, n_e, A)}; got on the device, either [N, H * W, CP] from a raw entry (its padding lanes must hold 0) or
    [N, C, H, W]; ref and A float64 [N, C, H, W]."""
    worst = (-1.0, None, None)
    for k, (got, ref, n, A) in outs.items():
        got = got.cpu()
        if got.dim() == 3:
            assert bool((got[:, :, C:] == 0).all()), (tag, k, "padding lanes")
            got, ref, A = got[:, :, :C], _cl(ref), _cl(A)
        assert got.shape == ref.shape and bool(torch.isfinite(got).all()), (tag, k)
        err = (got.double() - ref).abs()
        ratio = torch.where(err == 0, torch.zeros_like(err), err / R.step2d_bound(n, A))
        i = int(ratio.argmax())
        if float(ratio.flatten()[i]) > worst[0]:
            worst = (float(ratio.flatten()[i]), k, [int(q) for q in torch.unravel_index(torch.tensor(i), ratio.shape)])
    print(f"{tag}: err/bound {worst[0]:.4f} at {worst[1]} {worst[2]}")
    _LOG[tag] = {"ratio": round(worst[0], 4), "output": worst[1], "index": worst[2]}
    assert worst[0] <= EXCEPTIONS.get((tag, worst[1]), 1.0), (tag, worst)


def _raw_step(d, shape, x, t, clip, zs, zb):
    """``cindm_ddpm2d_step`` -> (x_out, x0, mean) in the library's layout [B * nb, H * W, CP]."""
    B, nb, C, H, W = shape
    dev = d.betas.device
    xd = to_device_layout(x.to(dev), d.model.padded_channels)
    x0, mean = torch.full_like(xd, SENTINEL), torch.full_like(xd, SENTINEL)
    h, ws = d._prepare(B * nb, dev)
    ns = _state_cl(zs.to(dev)) if t > 0 else None
    nbnd = _boundary_cl(zb.to(dev)) if t > 0 else None
    with torch.cuda.device(dev):
        _ffi.check(_ffi.lib().cindm_ddpm2d_step(h, d.model._h, _ffi.ptr(xd), B, nb, d._share_mode(), int(clip), _ffi.ptr(ns), _ffi.ptr(nbnd),
                                                0, 0, int(t), None, _ffi.ptr(x0), _ffi.ptr(mean), _ffi.ptr(ws), ws.numel(),
                                                _ffi.current_stream(dev)))
    return xd, x0, mean


def _raw_predict(d, shape, x, t, share, clip, rederive):
    """``cindm_ddpm2d_predict`` -> (pred_noise, x_start) in the library's layout."""
    B, nb, C, H, W = shape
    dev = d.betas.device
    xd = to_device_layout(x.to(dev), d.model.padded_channels)
    eps, x0 = torch.full_like(xd, SENTINEL), torch.full_like(xd, SENTINEL)
    h, ws = d._prepare(B * nb, dev)
    with torch.cuda.device(dev):
        _ffi.check(_ffi.lib().cindm_ddpm2d_predict(h, d.model._h, _ffi.ptr(xd), B, nb,
                                                   int(bool(d.use_average_share)) | (_ffi.OBJECTIVES[d.objective] << 4), int(share), int(clip),
                                                   int(rederive), int(t), None, _ffi.ptr(eps), _ffi.ptr(x0), _ffi.ptr(ws), ws.numel(),
                                                   _ffi.current_stream(dev)))
    return eps, x0


def _shapes(options):
    """The grid's (C, size, B, nb, options) points: the full cross at C = 21 and at C = 15, and one 64 x 64 case."""
    pts = [(C, 32, B, nb, o) for C in (S.CHANNELS, S.CHANNELS_ALIGNED) for o in options for (B, nb) in S.BNB]
    pts.append((S.CHANNELS, 64, 2, 3, options[len(options) // 2 + 2]))
    return pts


# ------------------------------------------------------------------ the entry's E is the model's
def test_entry_sees_the_same_E(device):
    """Under pred_x0 with clip off x_start IS the model's output: ``model_predictions(...).pred_x_start`` equals ``model(x, t)`` bit for
    bit, so judging the entry on an E evaluated apart from it charges the entry with nothing of the U-Net's."""
    for C, size, B, nb in ((S.CHANNELS, 32, 2, 3), (S.CHANNELS_ALIGNED, 32, 1, 2), (S.CHANNELS, 64, 1, 2)):
        d = _diff(device, C, size, "pred_x0")
        for t in (0, 500):
            x, E = _state_and_E(device, C, size, B, nb, t, False)
            pr = d.model_predictions((B, nb, C, size, size), x.to(device), torch.full((B * nb,), t, device=device), clip_x_start=False)
            assert torch.equal(pr.pred_x_start.cpu(), E), (C, size, t)
            assert torch.equal(_net(device, C, size)(x.to(device), t).cpu(), E)


# ------------------------------------------------------------------ update2d_kernel
@pytest.mark.parametrize("obj", S.OBJECTIVES)
def test_step_entry(device, obj):
    """``cindm_ddpm2d_step``: share_noise x mean / sum x clip x t in {0, 1, 500, 999} x (B, nb); x_out, x0 and mean, explicit noise.
    And: at t = 0 the state is the mean bit for bit; x0 is ``p_mean_variance``'s bit for bit."""
    pts = _shapes(S.STEP_OPTIONS)
    assert len(pts) == 2 * 32 * 5 + 1
    for C, size, B, nb, (share, avg, clip, t) in pts:
        shape = (B, nb, C, size, size)
        d = _diff(device, C, size, obj, share, avg)
        x, E = _state_and_E(device, C, size, B, nb, t, S.state_is_shared(share, avg, clip))
        zs, zb = S.make_noise(C, B, nb, t, size)
        xo, x0, mean = _raw_step(d, shape, x, t, clip, zs, zb)
        rm, r0, _, A = R.step2d_predict_f64(TAB[obj], shape, x, t, E, objective=obj, share_noise=share, use_average_share=avg, clip=clip)
        n = R.step2d_roundings(nb, obj, share_noise=share, clip=clip)
        rs, As, ns = R.step2d_update_f64("ddpm", rm, A["mean"], n["mean"], z=O.sample_noise_2d(zs, zb).reshape(x.shape), t=t,
                                         logvar=TAB[obj]["posterior_log_variance_clipped"][t])
        tag = f"step/{obj}-C{C}-{size}-B{B}nb{nb} share{int(share)}-avg{int(avg)}-clip{int(clip)}-t{t}"
        _hold(tag, {"x_out": (xo, rs, ns, As), "x_start": (x0, r0, n["x_start"], A["x_start"]), "mean": (mean, rm, n["mean"], A["mean"])}, C)
        if t == 0:
            assert torch.equal(xo, mean), tag
        if (B, nb) == (2, 3):
            pm, _, _, px0 = d.p_mean_variance(shape, x.to(device), t, clip_denoised=clip)
            assert torch.equal(_cl(px0), x0[:, :, :C]) and torch.equal(_cl(pm), mean[:, :, :C]), tag


@pytest.mark.parametrize("rederive", S.REDERIVE, ids=["raw", "rederive"])
@pytest.mark.parametrize("obj", S.OBJECTIVES)
def test_predict_entry(device, obj, rederive):
    """``cindm_ddpm2d_predict``: share_noise x mean / sum x clip x rederive x t x (B, nb); eps_out and x0."""
    pts = _shapes([o for o in S.PREDICT_OPTIONS if o[3] == rederive])
    assert len(pts) == 2 * 32 * 5 + 1
    for C, size, B, nb, (share, avg, clip, red, t) in pts:
        shape = (B, nb, C, size, size)
        d = _diff(device, C, size, obj, True, avg)
        x, E = _state_and_E(device, C, size, B, nb, t, S.state_is_shared(share, avg, clip, red))
        eps, x0 = _raw_predict(d, shape, x, t, share, clip, red)
        _, r0, re, A = R.step2d_predict_f64(TAB[obj], shape, x, t, E, objective=obj, share_noise=share, use_average_share=avg, clip=clip,
                                            rederive=red, entry="model_predictions")
        n = R.step2d_roundings(nb, obj, share_noise=share, clip=clip, rederive=red, entry="model_predictions")
        tag = f"predict/{obj}-C{C}-{size}-B{B}nb{nb} share{int(share)}-avg{int(avg)}-clip{int(clip)}-red{int(red)}-t{t}"
        _hold(tag, {"pred_noise": (eps, re, n["pred_noise"], A["pred_noise"]), "x_start": (x0, r0, n["x_start"], A["x_start"])}, C)


# ------------------------------------------------------------------ the DDIM kernels
def _ddim_case(device, obj, C, size, B, nb, avg, eta, i, shared, fo=None):
    shape = (B, nb, C, size, size)
    d = _diff(device, C, size, obj, True, avg, S.DDIM_S, eta)
    times, coefs = d.ddim_schedule()
    t, tn = times[i], times[i + 1]
    x, E = _state_and_E(device, C, size, B, nb, t, shared)
    zs, zb = S.make_noise(C, B, nb, i, size)
    ss, sb = torch.zeros((i + 1,) + tuple(zs.shape)), torch.zeros((i + 1,) + tuple(zb.shape))
    ss[i], sb[i] = zs, zb
    tape = cindm_amd.NoiseTape2D(None, ss, sb)
    kw = {} if fo is None else dict(design_fn=fo, design_guidance="standard-alpha")
    got = d.ddim_sample(shape, init_img=x.to(device), step_range=(i, i + 1), noise=tape, **kw).reshape(x.shape)
    _, r0, re, A = R.step2d_predict_f64(TAB[obj], shape, x, t, E, objective=obj, share_noise=True, use_average_share=avg, clip=True,
                                        rederive=True, entry="model_predictions")
    n = R.step2d_roundings(nb, obj, share_noise=True, clip=True, rederive=True, entry="model_predictions")
    rs, As, ns = R.step2d_update_f64("ddim", r0, A["x_start"], n["x_start"], z=O.sample_noise_2d(zs, zb).reshape(x.shape), eps=re,
                                     A_eps=A["pred_noise"], n_eps=n["pred_noise"], row=coefs[i], last=tn < 0)
    kernel = "ddim"
    if fo is not None:
        kernel = "ddim_guided"
        g = fo(x.to(device)).cpu()
        assert tuple(g.shape) == tuple(x.shape) and bool(g.abs().max() > 0)
        rs, As, ns = R.step2d_update_f64("guided", rs, As, ns, w=d.ddim_guidance_weights()[i], g=g)
    _hold(f"{kernel}/{obj}-C{C}-{size}-B{B}nb{nb} avg{int(avg)}-eta{eta}-i{i}", {"x_out": (got, rs, ns, As)}, C)


@pytest.mark.parametrize("obj", S.OBJECTIVES)
def test_ddim_update(device, obj):
    """ddim2d_update_kernel: S = 50, pairs {0, 1, 25, 49} (the last with t_next = -1), eta in {0, 0.5}, mean / sum, every (B, nb).
    share_noise False stays refused under DDIM."""
    pts = _shapes(S.DDIM_OPTIONS)
    assert len(pts) == 2 * 16 * 5 + 1
    for C, size, B, nb, (avg, eta, i) in pts:
        _ddim_case(device, obj, C, size, B, nb, avg, eta, i, S.state_is_shared(avg, eta > 0, i))
    d = _diff(device, S.CHANNELS, 32, obj, False, True, S.DDIM_S, 0.5)
    x = S.make_state(S.CHANNELS, 1, 2, 999, True, 32)
    with pytest.raises(NotImplementedError, match=S.REFUSAL_DDIM_NOSHARE):
        d.ddim_sample((1, 2, S.CHANNELS, 32, 32), init_img=x.to(device), step_range=(0, 1))


@pytest.mark.parametrize("obj", S.OBJECTIVES)
def test_ddim_guided_update(device, obj):
    """ddim2d_guided_update_kernel at 64 x 64, the size the surrogate is built for: pairs {0, 25, 49}, eta 0.5, (B, nb) = (1, 2) and
    (2, 2); g is the library's own objective on the step's input (bit-equal to the chain's: test_gpu_ddim_guided_2d.py's
    test_guided_ddim2d_fused_equals_loop_equals_eager relies on the same)."""
    sd = O.synth_state_dict_2d(O.force_unet_param_shapes(), 7)
    fm = cindm_amd.ForceUnet(dim=64, dim_mults=(1, 2, 4, 8), channels=4)
    fm.load_state_dict(sd, strict=True)
    fm = fm.to(device)
    for B, nb in S.GUIDED_BNB:
        fo = cindm_amd.ForceObjective(fm, B, nb, (S.CHANNELS - 3) // 3, p_min=-37.7, p_max=57.6)
        for i in S.GUIDED_PAIRS:
            _ddim_case(device, obj, S.CHANNELS, 64, B, nb, True, S.GUIDED_ETA, i, i == 25, fo=fo)


# ------------------------------------------------------------------ t from device memory
def _tape(seed, B, nb, C, size, T):
    g = torch.Generator().manual_seed(seed)
    init = (torch.randn((B, 1, C - 3, size, size), generator=g), torch.randn((B, nb, 3, size, size), generator=g))
    return cindm_amd.NoiseTape2D(init, torch.randn((T, B, 1, C - 3, size, size), generator=g), torch.randn((T, B, nb, 3, size, size), generator=g))


@pytest.mark.parametrize("share", S.SHARE, ids=["share_noise", "share_mean"])
def test_chain_reads_the_same_t(device, share):
    """The chain route hands update2d_kernel a device pointer to t where the step entry hands it an immediate.  A 4-timestep diffusion
    (as tests/test_gpu_counter_ledger.py builds one): the whole chain equals four step calls on the tape's rows bit for bit, and so
    does every prefix of it (``t_stop``); the first step of a 1000-timestep chain equals the step entry on the tape's init."""
    C, size = S.CHANNELS, 32
    for T in (4, 1000):
        B, nb = (2, 3) if T == 4 else (1, 2)            # (a 1000-row tape is moved to the device whole)
        shape = (B, nb, C, size, size)
        d = _diff(device, C, size, "pred_noise", share, True, T=T)
        tape = _tape(17 + T, B, nb, C, size, 4)
        if T == 1000:       # rows 996 .. 999 of a tape the chain indexes by t
            pad = lambda v: torch.cat([torch.zeros((996,) + tuple(v.shape[1:])), v])
            tape = cindm_amd.NoiseTape2D(tape.init, pad(tape.step_state), pad(tape.step_boundary))
        x = O.sample_noise_2d(*tape.init).reshape(B * nb, C, size, size).to(device)
        for t in reversed(range(T - (4 if T == 4 else 1), T)):
            nz = O.sample_noise_2d(tape.step_state[t], tape.step_boundary[t]).reshape(B * nb, C, size, size)
            x, _ = d.p_sample(shape, x, t, noise=nz.to(device) if t > 0 else None)
            chain = d.p_sample_loop(shape, noise=tape, t_stop=t)
            assert torch.equal(chain.reshape(x.shape), x), (T, t)


def test_exceptions_stay_empty():
    assert EXCEPTIONS == {} and R.BOUND_SLACK == 4
