"""GPU (MI355X): every block of ForceUnet, forward and input gradient, against the float64 reference of oracle/f64_reference.py,
image by image.

The older tests (tests/test_gpu_force.py) compare ``out [N, 2]`` -- two means over at least 64 pixels behind a 512-wide dot
product -- and ``dx`` with the fp32 oracle in the whole-tensor norm at 2e-5; a lost split-fp16 term in one block passes them
(tests/test_f64_reference_host.py keeps the figures).  Here, with the handle's option ``taps`` = 1, for every image ``r``:

    row_err(gpu, f64)[r]  <=  M * max(e32(T), 2^-23)

for T = ``out``, ``dx``, each of the block outputs the oracle names (``init_conv``, ``downs.i.0`` .. ``downs.i.3``, ``mid_block1``,
``mid_attn``, ``mid_block2``) and the gradient of the call's objective with respect to each of them (``grad:<name>``, the reference's
from autograd with ``retain_grad()``).  ``row_err``, ``e32`` and ``M`` are those of tests/test_gpu_f64_budget.py, whose ``_hold`` does
the comparison; a case that has not compared every tap of its model fails.  The gradient at ``mid_block2`` is the head's derivative,
one multiply per element away from ``out``: its e32 is under an ulp, so its yardstick is the ulp, and the ``> 2e-7`` floor on the
yardsticks holds for everything else.

Asserted on the float64 reference of every case: each ``|out[:, 0]|`` is at least 1e-3 of the largest ``|out|`` (the sign of the
objective's ``|.|`` is not in question); for the design gradient no summed and no single clamped boundary value lies within 1e-5 of
0 or 1 (the clamp's indicator is the same in fp32 and float64).  The seeds below were chosen so that both hold.

Images are independent (test_f64_reference_host.py for the reference, test_forceunet_full_batch_repeatable_and_batch_independent
for the library), so the default model's reference is evaluated once per image and shared by every image count and option set.

With CINDM_F64_BUDGET_JSON=<path> this module writes every case's largest ratio there when it finishes
(profiles/f64_budget_force.json is such a run)."""
import os

import pytest
import torch

import cindm_amd
import cindm_oracle as O
import f64_reference as R
from cindm_amd import _ffi
from test_gpu_f64_budget import _dump_log, _hold

pytestmark = pytest.mark.gpu

LAMBDA = 1.3
SEED_X = 37                     # input of the default model: randn((17, 4, 64, 64)), the first n images are used
SEED_DOUT = 12                  # dout [4, 2] of the vjp cases
BELOW_FLOOR = ("grad:mid_block2",)

# Section 5 of the issue: a (case, tap) whose kernel is honestly less accurate gets its own bound, with the derivation.  None taken.
EXCEPTIONS = {}

_LOG = {}


@pytest.fixture(scope="module", autouse=True)
def _write_log():
    yield
    path = os.environ.get("CINDM_F64_BUDGET_JSON")
    if path and _LOG:
        _dump_log(path, _LOG, ("force-64-n4", "force-64-n9", "force-64-n17", "vjp-", "design-"),
                  metric="row_err(gpu, f64) / max(e32(tap), 2^-23); row_err = max|a - ref| / max|ref| per image")


def _flat(run):
    out, dx, act, grad = run
    d = {"out": out, **act}
    if dx is not None:
        d.update({"dx": dx, **{"grad:" + k: v for k, v in grad.items()}})
    return d


class _Reference:
    """(float64 reference, row_err of the fp32 oracle) of one (weights, input, objective), every tap, kept and extended as the cases
    ask for more images.  Images are independent, and each is evaluated ALONE: the fp32 oracle's rounding depends on what its
    convolutions batch together, and a yardstick must not depend on which case asked first."""

    def __init__(self, sd, x, dout=None):
        self.sd, self.x, self.dout, self.have, self.t64, self.r32 = sd, x, dout, 0, {}, {}

    def upto(self, n):
        for i in range(self.have, n):
            s = slice(i, i + 1)
            kw = dict(lambda_force=LAMBDA) if self.dout is None else dict(dout=self.dout[s])
            f64, f32 = _flat(R.force_unet_f64(self.sd, self.x[s], **kw)), _flat(R.force_unet_blocks(self.sd, self.x[s], **kw))
            for k, v in f64.items():
                self.t64[k] = v if i == 0 else torch.cat([self.t64[k], v])
                self.r32[k] = R.row_err(f32[k], v) if i == 0 else torch.cat([self.r32[k], R.row_err(f32[k], v)])
            self.have = i + 1
        out = self.t64["out"][:n]
        small = float((out[:, 0].abs() / out.abs().max()).min())
        assert small >= 1e-3, ("the sign of |out0| is in question at this seed", small)
        return self.t64, self.r32


def _build(device, size=64, mults=(1, 2, 4, 8), seed=7, opts=None):
    sd = O.synth_state_dict_2d(O.force_unet_param_shapes(dim_mults=mults), seed)
    m = cindm_amd.ForceUnet(dim=64, dim_mults=mults, channels=4, image_size=size)
    m.load_state_dict(sd, strict=True)
    m = m.to(device)
    for k, v in (opts or {}).items():
        m.set_option(k, v)
    return m, sd


def _compare(case, m, call, n, t64, r32, forward_only=False):
    """``call()`` -> (out, dx) with taps = 1; every tap of the model (activations only after a forward-only call) held to the budget."""
    m.set_option("taps", 1)
    try:
        out, dx = call()
        want = {k: v for k, v in t64.items() if not forward_only or not (k == "dx" or k.startswith("grad:"))}

        def fetch(k):
            v = out if k == "out" else dx if k == "dx" else m.tap(k[5:], n, grad=True) if k.startswith("grad:") else m.tap(k, n)
            return v.cpu()

        _hold(case, fetch, want, r32, rows=n, need=set(want), log=_LOG, exceptions=EXCEPTIONS, out="out", below_floor=BELOW_FLOOR)
        assert len(_LOG[case]["taps"]) == len(want) and not _LOG[case]["refused"]
        if forward_only:
            with pytest.raises(cindm_amd.CindmError, match="forward-only"):
                m.tap("mid_block1", n, grad=True)
        with pytest.raises(cindm_amd.CindmError, match="unknown tap: ups.0.0"):
            m.tap("ups.0.0", n)
        with pytest.raises(cindm_amd.CindmError, match="tap: image count differs from the last call"):
            m.tap("mid_block1", n + 1)
    finally:
        m.set_option("taps", 0)
    return out, dx


def _same_without_taps(m, call, n, out, dx):
    """taps = 1 copies where taps = 0 shares a gradient buffer: the same arithmetic, bit for bit, in the same workspace."""
    L = _ffi.lib()
    assert m.get_option("taps") == 0
    bytes0 = [L.cindm_forceunet_workspace_bytes(m._h, n, g) for g in (0, 1)]
    out0, dx0 = call()
    assert torch.equal(out0, out) and (dx is None or torch.equal(dx0, dx))
    with pytest.raises(cindm_amd.CindmError, match="unknown tap"):            # a call without the option leaves nothing to serve
        m.tap("mid_block1", n)
    m.set_option("taps", 1)
    try:
        assert [L.cindm_forceunet_workspace_bytes(m._h, n, g) for g in (0, 1)] == bytes0 and min(bytes0) > 0
    finally:
        m.set_option("taps", 0)


# ------------------------------------------------------------------ default model
@pytest.fixture(scope="module")
def force(device):
    m, sd = _build(device)
    x = torch.randn((17, 4, 64, 64), generator=torch.Generator().manual_seed(SEED_X))
    return m, sd, x, _Reference(sd, x)


# 1: no partner at the paired 8 x 8 level;  2 | 3, 4, 8 | 9: even counts pair two images per tile there (conv2d_ws_kernel<CONV_3X3_PAIR>),
# odd ones stay on the fp32 kernel (ws_ok);  8 | 9: 32 tiles per 64 x 64 image -> the 256 persistent workgroups first walk a second tile
# at 9 images;  17: odd, a third tile for some workgroups
@pytest.mark.parametrize("n", [1, 2, 3, 4, 8, 9, 17])
def test_input_grad_image_counts(device, force, n):
    m, _, x, ref = force
    t64, r32 = ref.upto(n)
    xd = x[:n].to(device)
    call = lambda: m.input_grad(xd, lambda_force=LAMBDA)
    out, dx = _compare(f"force-64-n{n}", m, call, n, t64, r32)
    _same_without_taps(m, call, n, out, dx)


@pytest.mark.parametrize("n", [3, 4])
def test_forward_only_call(device, force, n):
    m, _, x, ref = force
    t64, r32 = ref.upto(n)
    xd = x[:n].to(device)
    call = lambda: (m(xd), None)
    out, _ = _compare(f"forward-64-n{n}", m, call, n, t64, r32, forward_only=True)
    _same_without_taps(m, call, n, out, None)


_VJP_REF = []


@pytest.mark.parametrize("route", ["vjp", "autograd"])
def test_vjp_with_mixed_signs(device, force, route):
    """``cindm_forceunet_vjp``: sum(dout * out) for a seeded dout of both signs, called directly and as the backward of ``m(x)`` under
    torch.autograd."""
    m, sd, x, _ = force
    n = 4
    dout = torch.randn((n, 2), generator=torch.Generator().manual_seed(SEED_DOUT))
    assert bool((dout > 0).any(dim=0).all()) and bool((dout < 0).any(dim=0).all())
    if not _VJP_REF:
        _VJP_REF.append(_Reference(sd, x[:n], dout))
    t64, r32 = _VJP_REF[0].upto(n)

    def direct():
        return m._run(x[:n].to(device), dout=dout)

    def autograd():
        xd = x[:n].to(device).requires_grad_(True)
        y = m(xd)
        assert y.requires_grad
        return y.detach(), torch.autograd.grad(y, xd, grad_outputs=dout.to(device))[0]

    call = direct if route == "vjp" else autograd
    out, dx = _compare(f"vjp-{route}-n{n}", m, call, n, t64, r32)
    _same_without_taps(m, call, n, out, dx)


# ------------------------------------------------------------------ option sets
OPTION_SETS = [{"h3": 0, "h3_bwd": 0}, {"gn_bwd_fused": 0}, {"gn_bwd_fused": 1}, {"no_exchange": 1}, {"la_fused": 0}, {"ws_nosplit": 0},
               {"ws_nosplit": 1}]
_OPT_MODEL = {}


def _oid(o):
    return "-".join(f"{k}={v}" for k, v in o.items())


@pytest.mark.parametrize("opts,n", [(o, n) for o in OPTION_SETS for n in (3, 4)], ids=[f"{_oid(o)}-{n}" for o in OPTION_SETS for n in (3, 4)])
def test_option_sets(device, force, opts, n):
    _, sd, x, ref = force
    key = _oid(opts)
    if key not in _OPT_MODEL:           # (one model alive at a time; the two sizes of an option set follow each other)
        _OPT_MODEL.clear()
        _OPT_MODEL[key] = _build(device, opts=opts)[0]
    m = _OPT_MODEL[key]
    for k, v in opts.items():
        assert m.get_option(k) == v
    t64, r32 = ref.upto(n)
    xd = x[:n].to(device)
    call = lambda: m.input_grad(xd, lambda_force=LAMBDA)
    out, dx = _compare(f"opt-{key}-n{n}", m, call, n, t64, r32)
    _same_without_taps(m, call, n, out, dx)
    assert m.recovered == 0 and m.poll_status(device) == 0


# ------------------------------------------------------------------ other instantiations
# (image size, dim_mults, images, input seed): those of test_forceunet_other_image_sizes and the 128-channel LinearAttention site at
# 32 x 32 of test_forceunet_fused_linear_attention_vs_layered; weight seed 5 as there
INSTANCES = [(32, (1, 2, 8), 4, 3), (16, (1, 8), 6, 25), (32, (1, 8), 3, 27), (64, (1, 2, 8), 2, 3), (32, (8,), 2, 3), (128, (1, 2, 4, 8), 1, 3),
             (64, (2, 2, 4, 8), 4, 13)]


@pytest.mark.parametrize("size,mults,n,xseed", INSTANCES, ids=[f"{s}-m{''.join(map(str, mu))}-n{n}" for s, mu, n, _ in INSTANCES])
def test_other_instantiations(device, size, mults, n, xseed):
    m, sd = _build(device, size, mults, seed=5)
    x = torch.randn((n, 4, size, size), generator=torch.Generator().manual_seed(xseed))
    t64, r32 = _Reference(sd, x).upto(n)
    assert len(t64) == 2 + 2 * (4 + 4 * len(mults))
    xd = x.to(device)
    call = lambda: m.input_grad(xd, lambda_force=LAMBDA)
    out, dx = _compare(f"inst-{size}-m{''.join(map(str, mults))}-n{n}", m, call, n, t64, r32)
    _same_without_taps(m, call, n, out, dx)


# ------------------------------------------------------------------ the design gradient
# p_min, p_max and the two lambdas are fp32 numbers: the library is handed C floats.  lambda_overlap is small on purpose: the overlap
# term is a few exact operations per pixel, and at the script's 1.0 it dominates the boundary channels, whose e32 then drops to 1e-7
# -- no yardstick for the surrogate's gradient through the clamped boundary sum, which is what is measured here.
DESIGN_KW = dict(p_min=-37.75, p_max=57.5, lambda_force=0.75, lambda_overlap=0.125)
DESIGN_SEED = {(1, 2, 2): 2, (2, 3, 1): 11}
_DESIGN_REF = {}


def _design_reference(sd, B, nb, frames, sb):
    key = (B, nb, frames, sb)
    if key not in _DESIGN_REF:
        gen = torch.Generator().manual_seed(DESIGN_SEED[(B, nb, frames)])
        x = torch.randn((B * nb, 3 * frames + 3, 64, 64), generator=gen) * 0.5       # (half of the boundary values below the clamp, 2 % above)
        g64 = R.airfoil_design_grad_f64(sd, x, B, nb, frames, sum_boundary=sb, **DESIGN_KW)
        g32 = O.airfoil_design_grad(sd, x, B, nb, frames, sum_boundary=sb, **DESIGN_KW)
        # the inputs' conditions, on the float64 reference's own arguments
        xb = x[:, -3:].double()
        summed = xb.view(B, nb, 3, 64, 64).sum(1)
        for v in (summed, xb[:, 0]):
            assert float(torch.minimum(v.abs(), (v - 1).abs()).min()) > 1e-5, "a clamped boundary value sits at the clamp's edge at this seed"
        frames_out = [R.force_unet_f64(sd, torch.cat([((0.5 * x[:, 2 + 3 * i].double() + 0.5) * (57.5 + 37.75) - 37.75 if sb else x[:, 2 + 3 * i].double())
                                                       .unsqueeze(1), (summed.clamp(0, 1).repeat_interleave(nb, 0) if sb else xb)], 1))[0] for i in range(frames)]
        for out in frames_out:
            assert float((out[:, 0].abs() / out.abs().max()).min()) >= 1e-3, "the sign of |out0| is in question at this seed"
        parts = {"state": slice(0, -3), "boundary": slice(-3, None)}
        _DESIGN_REF[key] = (x, {k: g64[:, s] for k, s in parts.items()}, {k: R.row_err(g32[:, s], g64[:, s]) for k, s in parts.items()})
    return _DESIGN_REF[key]


DESIGN_CASES = [(B, nb, fr, sb, fpp) for (B, nb, fr) in ((1, 2, 2), (2, 3, 1)) for sb in (True, False) for fpp in sorted({fr, 1}, reverse=True)]


@pytest.mark.parametrize("B,nb,frames,sb,fpp", DESIGN_CASES, ids=[f"b{B}-nb{nb}-f{fr}-{'sum' if sb else 'own'}-fpp{fpp}" for B, nb, fr, sb, fpp in DESIGN_CASES])
def test_design_gradient(device, force, B, nb, frames, sb, fpp):
    """``ForceObjective`` (no taps: the design gradient lays out its own workspace) against ``airfoil_design_grad_f64``, image by image,
    state channels (the pressure frames carry the force gradient) and boundary channels (force through the clamped sum, and the overlap
    term) separately."""
    m, sd, _, _ = force
    x, t64, r32 = _design_reference(sd, B, nb, frames, sb)
    fn = cindm_amd.ForceObjective(m, B, nb, frames, frames_per_pass=fpp, sum_boundary=sb, **DESIGN_KW)
    g = fn(x.to(device)).cpu()
    assert tuple(g.shape) == tuple(x.shape)
    _hold(f"design-b{B}-nb{nb}-f{frames}-{'sum' if sb else 'own'}-fpp{fpp}", lambda k: g[:, :-3] if k == "state" else g[:, -3:], t64, r32,
          need={"state", "boundary"}, log=_LOG, exceptions=EXCEPTIONS, out="state")
