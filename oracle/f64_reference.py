"""Float64 reference of the two U-Net forwards, and the per-row error budget the HIP kernels are held to.

TEST INFRASTRUCTURE ONLY, like ``cindm_oracle``: a checker for the HIP path, imported by ``tests/`` alone.

Why: the fp32 oracle is itself 0.4e-6 .. 1.7e-6 away from exact arithmetic (per row, largest error over largest
value), which is the level at which the HIP path agrees with it.  A comparison with the fp32 oracle can therefore not
say how accurate a kernel is, and the 2e-5 whole-tensor bounds of the older tests are 20 times looser than what a
reference can resolve: a split-fp16 product that loses its low plane in one deep layer moves eps by 1.4e-5 and passes
them (tests/test_f64_reference_host.py keeps that figure as a fact).

The reference: ``cindm_oracle``'s own functional blocks, which follow the dtype of their arguments, on weights and
inputs cast to float64.  One thing stays fp32: the sinusoidal embedding, computed exactly as ``sinusoidal_pos_emb``
does and then cast up -- the library is handed that fp32 table (``cindm_amd.unet1d.sinusoid_table``), so it is an input
and not rounding to charge to a kernel.  Everything after it, the time MLPs included, is float64.

The budget: for every compared row (1-D) or image (2-D) ``r`` and every tap ``T`` (eps included)

    row_err(gpu, f64)[r]  <=  M * e32(T),        e32(T) = max over the compared rows of row_err(fp32 oracle, f64)

i.e. the kernels' accuracy is stated as a multiple of the fp32 reference's own accuracy at the same block.
"""
import torch

import cindm_oracle as O

# Twice the largest row_err(gpu) / e32 measured over every (case, tap) of tests/test_gpu_f64_budget*.py on an MI355X
# (profiles/f64_budget.json), rounded up to a power of two; one constant for the split-fp16 and the exact-fp32 kernels.
# Measured: 2.005 (the exact-fp32 MFMA kernels, downs.2.0 at 17 rows; the split-fp16 plans stay under 1.71), so 2 x 2.005
# rounds up to 8.  It may not exceed 8: a lost split term sits above 100 x e32 at its block, and
# tests/test_f64_reference_host.py asks for a factor of 10 between that and M * e32.
M = 8


def _f64(sd):
    return {k: v.double() for k, v in sd.items()}


def unet1d_forward_f64(sd, x, t, taps=None):
    """``cindm_oracle.unet1d_forward`` in float64.  ``sd`` of any float dtype, x [B, horizon, F], t [B] int64."""
    return O.unet1d_forward(_f64(sd), x.double(), t, taps=taps)


def unet2d_forward_f64(sd, x, t, taps=None):
    """``cindm_oracle.unet2d_forward`` in float64.  x [B, C, H, W], t [B] int64."""
    return O.unet2d_forward(_f64(sd), x.double(), t, taps=taps)


def row_err(a, ref):
    """Per row (1-D) / per image (2-D) of one tensor: max|a - ref| / max|ref| over that row, in float64 -> [rows]."""
    a = torch.as_tensor(a).detach().cpu().double().reshape(ref.shape[0], -1)
    ref = torch.as_tensor(ref).detach().cpu().double().reshape(ref.shape[0], -1)
    return (a - ref).abs().amax(1) / ref.abs().amax(1)


def e32(o32, ref):
    """The fp32 oracle's own error at one tap: the largest ``row_err`` over the rows compared."""
    return float(row_err(o32, ref).max())
