"""CPU: the float64 reference of oracle/f64_reference.py and the budget ``row_err <= M * e32`` built on it.

1. Agreement: the float64 forwards restate the same function as the fp32 oracle (5e-6 per row at every tap; the fp32
   oracle's own rounding is 1.7e-6 at most here).
2. Independence: a row's result does not depend on its batch mates, to 1e-12 -- the GPU tests evaluate the reference on a
   subset of a large batch's rows.
3. The budget can tell a lost split-fp16 term from rounding: the input of one convolution rounded to fp16 (what losing
   the low plane of its activations does) moves that block's output by more than 10 x M x e32, while eps, in the
   whole-tensor norm of the older GPU tests, stays under their 2e-5 for the deepest layer -- the blind spot, as a fact.
4. The same three for ForceUnet and its input gradient (``force_unet_f64``: activations and gradients at every block boundary).
   A lost forward plane in ``mid_block1`` or ``downs.1.0`` moves ``out`` by 1.8e-5 / 1.2e-5 -- under the 2e-5 of
   tests/test_gpu_force.py -- and its own tap by 227 / 348 x e32; a lost plane of the gradient entering a block moves the gradient
   tap just upstream by 169 .. 307 x e32."""
import pytest
import torch

import cindm_oracle as O
import f64_reference as R

TOL_FWD = 2e-5            # tests/test_gpu_parity.py (not imported: that module needs the HIP library)


def _fwd1d(sd, x, t, f64):
    taps = {}
    eps = (R.unet1d_forward_f64 if f64 else O.unet1d_forward)(sd, x, t, taps=taps)
    taps["eps"] = eps
    return taps


def _fwd2d(sd, x, t, f64):
    taps = {}
    eps = (R.unet2d_forward_f64 if f64 else O.unet2d_forward)(sd, x, t, taps=taps)
    taps["eps"] = eps
    return taps


@pytest.fixture(scope="module")
def case1d():
    """Default 1-D model (horizon 24, 8 features), 9 rows, t = 500."""
    sd = O.synth_state_dict(O.unet1d_param_shapes(24, 8, attention=True), seed=0)
    x = torch.randn((9, 24, 8), generator=torch.Generator().manual_seed(9))
    t = torch.full((9,), 500, dtype=torch.long)
    return sd, x, t, _fwd1d(sd, x, t, False), _fwd1d(sd, x, t, True)


@pytest.fixture(scope="module")
def case2d():
    """2-D Unet, 2 images of 32x32, t = 500."""
    sd = O.synth_state_dict_2d(O.unet2d_param_shapes(64, (1, 2), 21), 0)
    x = torch.randn((2, 21, 32, 32), generator=torch.Generator().manual_seed(1))
    t = torch.full((2,), 500, dtype=torch.long)
    return sd, x, t, _fwd2d(sd, x, t, False), _fwd2d(sd, x, t, True)


def test_f64_forwards_agree_with_fp32_oracle(case1d, case2d):
    for name, (_, _, _, t32, t64) in (("1d", case1d), ("2d", case2d)):
        assert set(t32) == set(t64) and len(t64) == (33 if name == "1d" else 22)
        for k, ref in t64.items():
            assert ref.dtype == torch.float64 and t32[k].dtype == torch.float32, (name, k)
            assert R.e32(t32[k], ref) < 5e-6, (name, k)


def test_sinusoid_stays_fp32_and_is_the_librarys_table(case1d):
    """The embedding is an input (the library is handed this fp32 table), so the float64 forward must not recompute it in
    float64: time MLP of the fp32 sinusoid cast up, evaluated by hand, equals the reference's ``temb`` exactly."""
    import torch.nn.functional as F
    sd, _, t, _, t64 = case1d
    e = O.sinusoidal_pos_emb(t, 64)
    assert e.dtype == torch.float32
    from cindm_amd.unet1d import sinusoid_table
    assert torch.equal(sinusoid_table(1000, 64)[500], e[0])
    w = {k: v.double() for k, v in sd.items() if k.startswith("time_mlp.")}
    want = F.linear(F.mish(F.linear(e.double(), w["time_mlp.1.weight"], w["time_mlp.1.bias"])), w["time_mlp.3.weight"], w["time_mlp.3.bias"])
    assert torch.equal(t64["temb"], want)


def test_rows_are_independent_in_the_reference(case1d, case2d):
    for fwd, (sd, x, t, _, t64) in ((_fwd1d, case1d), (_fwd2d, case2d)):
        for r in range(x.shape[0]):
            one = fwd(sd, x[r:r + 1], t[r:r + 1], True)
            for k, ref in t64.items():
                assert float(R.row_err(one[k], ref[r:r + 1])) <= 1e-12, (k, r)


LOST_TERM_LAYERS = ["mid_block1.blocks.0", "downs.3.0.blocks.1", "ups.0.0.blocks.0", "downs.2.1.blocks.0", "downs.0.0.blocks.1"]


@pytest.mark.parametrize("layer", LOST_TERM_LAYERS)
def test_budget_sees_a_lost_fp16_plane(monkeypatch, case1d, layer):
    sd, x, t, t32, t64 = case1d
    orig = O.conv1d_block

    def lossy(sdx, p, xx, n_groups=8):
        return orig(sdx, p, xx.half().double() if p == layer else xx, n_groups)

    monkeypatch.setattr(O, "conv1d_block", lossy)
    bad = _fwd1d(sd, x, t, True)
    monkeypatch.undo()
    block = layer.split(".blocks")[0]
    worst = float(R.row_err(bad[block], t64[block]).max())
    budget = R.M * R.e32(t32[block], t64[block])
    print(f"{layer}: row_err at {block} {worst:.3e}, M * e32 {budget:.3e}, ratio {worst / budget:.1f}")
    assert worst >= 10 * budget, (layer, worst, budget)
    if layer == "mid_block1.blocks.0":
        whole = float((bad["eps"] - t64["eps"]).abs().max() / t64["eps"].abs().max())
        print(f"{layer}: eps moves by {whole:.3e} in the whole-tensor norm (TOL_FWD {TOL_FWD:g})")
        assert whole < TOL_FWD          # ... and the older tests, which look at eps only, do not see it
        assert whole > R.M * R.e32(t32["eps"], t64["eps"])       # the per-row budget at eps does


# ------------------------------------------------------------------ ForceUnet: blocks, gradients at the block boundaries, design gradient
FORCE_LAMBDA = 1.3


@pytest.fixture(scope="module")
def caseforce():
    """Default ForceUnet (64 x 64, (1, 2, 4, 8), weight seed 7), 2 images, objective sum(1.3 |out0| + out1): (sd, x, fp32 run, float64
    run), a run = (out, dx, activations, gradients)."""
    sd = O.synth_state_dict_2d(O.force_unet_param_shapes(), 7)
    x = torch.randn((2, 4, 64, 64), generator=torch.Generator().manual_seed(11))
    return sd, x, R.force_unet_blocks(sd, x, FORCE_LAMBDA), R.force_unet_f64(sd, x, FORCE_LAMBDA)


def _flat(run):
    out, dx, act, grad = run
    return {"out": out, "dx": dx, **act, **{"grad:" + k: v for k, v in grad.items()}}


def test_force_f64_agrees_with_fp32_oracle(caseforce):
    """Activations 0.5e-6 .. 1.1e-6, gradients 0.8e-6 .. 1.8e-6, out 2.6e-7 at four images; bounds with a factor of two around them.
    The gradient at mid_block2 is the head's derivative, one multiply per element: under one ulp."""
    _, _, r32, r64 = caseforce
    f32, f64 = _flat(r32), _flat(r64)
    assert set(f32) == set(f64) and len(f64) == 2 + 2 * 20
    for k, ref in f64.items():
        assert ref.dtype == torch.float64 and f32[k].dtype == torch.float32, k
        e = R.e32(f32[k], ref)
        print(f"{k:20s} e32 {e:.3e}")
        if k == "grad:mid_block2":
            assert e < 2.0 ** -23, (k, e)
        elif k == "out":
            assert 1.3e-7 < e < 5.2e-7, (k, e)
        elif k == "dx" or k.startswith("grad:"):
            assert 0.4e-6 < e < 3.6e-6, (k, e)
        else:
            assert 0.25e-6 < e < 2.2e-6, (k, e)


def test_force_images_are_independent_in_the_reference(caseforce):
    sd, x, _, r64 = caseforce
    f64 = _flat(r64)
    for r in range(x.shape[0]):
        one = _flat(R.force_unet_f64(sd, x[r:r + 1], FORCE_LAMBDA))
        for k, ref in f64.items():
            assert float(R.row_err(one[k], ref[r:r + 1])) <= 1e-12, (k, r)


def test_force_vjp_objective_and_forward_only(caseforce):
    """``dout`` = (lambda sign(out0), 1) restates the built-in objective; without an objective nothing is differentiated."""
    sd, x, _, r64 = caseforce
    out = r64[0]
    dout = torch.stack([R._as_f32(FORCE_LAMBDA) * out[:, 0].sign(), torch.ones_like(out[:, 1])], 1)
    v = _flat(R.force_unet_f64(sd, x, dout=dout))
    for k, ref in _flat(r64).items():
        assert float(R.row_err(v[k], ref).max()) <= 1e-12, k
    o, dx, act, grad = R.force_unet_f64(sd, x)
    assert dx is None and grad == {} and torch.equal(o, out) and set(act) == set(r64[2])


def _lose_low_plane(v):
    """What a split-fp16 operand without its low plane is: fp16 after a per-image power-of-two scale."""
    s = torch.exp2(torch.ceil(torch.log2(v.detach().abs().amax(dim=(1, 2, 3), keepdim=True))))
    return (v / s).half().to(v.dtype) * s


@pytest.mark.parametrize("block", ["mid_block1", "downs.1.0"])
def test_force_budget_sees_a_lost_forward_plane_that_out_does_not(monkeypatch, caseforce, block):
    """The activation fed to the first 3x3 convolution of one residual block without its low plane (the residual path exact): far
    above the budget at the block's tap, under the older tests' 2e-5 at ``out`` in their whole-tensor norm."""
    sd, x, r32, r64 = caseforce
    sd64 = {k: v.double() for k, v in sd.items()}
    target, orig = sd64[block + ".block1.proj.weight"], O._ws_conv2d
    monkeypatch.setattr(O, "_ws_conv2d", lambda xx, w, b, padding: orig(_lose_low_plane(xx) if w is target else xx, w, b, padding))
    out, _, act, _ = R.force_unet_blocks(sd64, x.double())
    monkeypatch.undo()
    worst = float(R.row_err(act[block], r64[2][block]).max())
    budget = R.M * max(R.e32(r32[2][block], r64[2][block]), 2.0 ** -23)
    whole = float((out - r64[0]).abs().max() / r64[0].abs().max())
    print(f"{block}: row_err at its tap {worst:.3e}, M * e32 {budget:.3e}, ratio {worst / budget:.1f}; out moves by {whole:.3e}")
    assert worst >= 10 * budget, (block, worst, budget)
    assert whole < TOL_FWD, (block, whole)


# (block whose incoming gradient loses its low plane, the gradient tap just upstream)
LOST_GRAD = [("mid_block1", "downs.3.3"), ("downs.1.0", "downs.0.3"), ("mid_block2", "mid_attn"), ("downs.3.0", "downs.2.3"),
             ("downs.2.1", "downs.2.0"), ("downs.0.1", "downs.0.0")]


@pytest.mark.parametrize("block,upstream", LOST_GRAD, ids=[b for b, _ in LOST_GRAD])
def test_force_budget_sees_a_lost_backward_plane(monkeypatch, caseforce, block, upstream):
    """The gradient entering one block without its low plane (a hook on the tap's gradient) against the budget at the gradient
    tap just upstream."""
    sd, x, r32, r64 = caseforce
    orig = O.force_unet_forward

    def hooked(sdx, xx, taps=None):
        out = orig(sdx, xx, taps=taps)
        taps[block].register_hook(_lose_low_plane)
        return out

    monkeypatch.setattr(O, "force_unet_forward", hooked)
    _, _, _, grad = R.force_unet_f64(sd, x, FORCE_LAMBDA)
    monkeypatch.undo()
    worst = float(R.row_err(grad[upstream], r64[3][upstream]).max())
    budget = R.M * max(R.e32(r32[3][upstream], r64[3][upstream]), 2.0 ** -23)
    print(f"{block}: row_err of the gradient at {upstream} {worst:.3e}, M * e32 {budget:.3e}, ratio {worst / budget:.1f}")
    assert worst >= 10 * budget, (block, worst, budget)


def test_design_gradient_f64_agrees_with_fp32_oracle():
    sd = O.synth_state_dict_2d(O.force_unet_param_shapes(), 7)
    x = torch.randn((2, 9, 64, 64), generator=torch.Generator().manual_seed(5)) * 0.5
    for sb in (True, False):
        g32 = O.airfoil_design_grad(sd, x, 1, 2, 2, -37.75, 57.5, 0.75, 2.0, sum_boundary=sb)
        g64 = R.airfoil_design_grad_f64(sd, x, 1, 2, 2, -37.75, 57.5, 0.75, 2.0, sum_boundary=sb)
        assert g64.dtype == torch.float64 and g32.dtype == torch.float32
        for part in (slice(0, -3), slice(-3, None)):
            assert R.e32(g32[:, part], g64[:, part]) < 5e-6, (sb, part)


def test_budget_constant():
    assert R.M <= 8 and R.M & (R.M - 1) == 0
