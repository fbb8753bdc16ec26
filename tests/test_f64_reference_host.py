"""CPU: the float64 reference of oracle/f64_reference.py and the budget ``row_err <= M * e32`` built on it.

1. Agreement: the float64 forwards restate the same function as the fp32 oracle (5e-6 per row at every tap; the fp32
   oracle's own rounding is 1.7e-6 at most here).
2. Independence: a row's result does not depend on its batch mates, to 1e-12 -- the GPU tests evaluate the reference on a
   subset of a large batch's rows.
3. The budget can tell a lost split-fp16 term from rounding: the input of one convolution rounded to fp16 (what losing
   the low plane of its activations does) moves that block's output by more than 10 x M x e32, while eps, in the
   whole-tensor norm of the older GPU tests, stays under their 2e-5 for the deepest layer -- the blind spot, as a fact."""
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


def test_budget_constant():
    assert R.M <= 8 and R.M & (R.M - 1) == 0
