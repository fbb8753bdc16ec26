"""Float64 reference of the two U-Net forwards and of ForceUnet with its input gradient, and the per-row error budget the HIP kernels are held to.

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

ForceUnet (``force_unet_f64``, ``airfoil_design_grad_f64``) adds the backward: the taps are the block outputs AND the gradient of
the call's objective with respect to each of them (autograd with ``retain_grad()`` on the oracle's taps), ``out`` and ``dx``.  There
the yardstick is ``max(e32(T), 2^-23)``: the gradient at ``mid_block2`` is the head's derivative, one multiply per element, and its
e32 (6e-8) is under one ulp.  Scalars (lambda, p_min, p_max) enter as the C floats the library is handed.
"""
import torch

import cindm_oracle as O

# Twice the largest row_err(gpu) / e32 measured over every (case, tap) of tests/test_gpu_f64_budget*.py on an MI355X
# (profiles/f64_budget.json), rounded up to a power of two; one constant for the split-fp16 and the exact-fp32 kernels.
# Measured: 2.005 (the exact-fp32 MFMA kernels, downs.2.0 at 17 rows; the split-fp16 plans stay under 1.71), so 2 x 2.005
# rounds up to 8.  It may not exceed 8: a lost split term sits above 100 x e32 at its block, and
# tests/test_f64_reference_host.py asks for a factor of 10 between that and M * e32.
# ForceUnet (tests/test_gpu_f64_budget_force.py, profiles/f64_budget_force.json) is held to the same 8 and was not allowed to move
# it: largest 4.332, the gradient at downs.3.2 with an odd image count, where the 512-channel 8 x 8 level runs the exact-fp32
# MFMA convolutions (one fp32 accumulator over 4608 products); every convolution on the split-fp16 kernels: 1.91 at most.  The
# margin left there is 1.85 instead of 2, and an emulated lost plane sits at 169 .. 348 x e32 (>= 21 x M x e32).
M = 8


def _f64(sd):
    return {k: v.double() for k, v in sd.items()}


def unet1d_forward_f64(sd, x, t, taps=None):
    """``cindm_oracle.unet1d_forward`` in float64.  ``sd`` of any float dtype, x [B, horizon, F], t [B] int64."""
    return O.unet1d_forward(_f64(sd), x.double(), t, taps=taps)


def unet2d_forward_f64(sd, x, t, taps=None):
    """``cindm_oracle.unet2d_forward`` in float64.  x [B, C, H, W], t [B] int64."""
    return O.unet2d_forward(_f64(sd), x.double(), t, taps=taps)


def _as_f32(v):
    """A scalar as the library is handed it (a C float): an input, like the sinusoid table, and no rounding to charge to a kernel."""
    return float(torch.tensor(float(v), dtype=torch.float32))


def force_unet_blocks(sd, x, lambda_force=None, dout=None):
    """``cindm_oracle.force_unet_forward`` in the dtype of ``sd`` and ``x``, with the gradient of the objective
    ``sum(lambda_force * |out[:, 0]| + out[:, 1])`` (what ``cindm_forceunet_grad`` differentiates) or ``sum(dout * out)``
    (``cindm_forceunet_vjp``) at the input and at every block boundary: autograd with ``retain_grad()`` on the oracle's taps.
    -> out [N, 2], dx (None without an objective), {tap: activation}, {tap: gradient}."""
    with_grad = lambda_force is not None or dout is not None
    x = x.detach().clone().requires_grad_(with_grad)
    taps = {}
    with torch.enable_grad():
        out = O.force_unet_forward(sd, x, taps=taps)
        if with_grad:
            for v in taps.values():
                v.retain_grad()
            obj = dout.to(out.dtype) * out if dout is not None else _as_f32(lambda_force) * out[:, 0].abs() + out[:, 1]
            obj.sum().backward()
    return out.detach(), x.grad, {k: v.detach() for k, v in taps.items()}, {k: v.grad for k, v in taps.items()} if with_grad else {}


def force_unet_f64(sd, x, lambda_force=None, dout=None):
    """``force_unet_blocks`` on weights and input cast to float64 (``dout`` too: it is an input).  The same function on the fp32
    arguments gives e32."""
    return force_unet_blocks(_f64(sd), x.double(), lambda_force, None if dout is None else dout.double())


def airfoil_design_grad_f64(sd, x, batch_size, num_boundaries, frames, p_min, p_max, lambda_force=1.0, lambda_overlap=1.0,
                            downsampling_factor=4, sum_boundary=True):
    """``cindm_oracle.airfoil_design_grad`` on float64 weights and state; the four scalars as the library is handed them."""
    return O.airfoil_design_grad(_f64(sd), x.double(), batch_size, num_boundaries, frames, _as_f32(p_min), _as_f32(p_max),
                                 _as_f32(lambda_force), _as_f32(lambda_overlap), downsampling_factor, sum_boundary=sum_boundary)


def row_err(a, ref):
    """Per row (1-D) / per image (2-D) of one tensor: max|a - ref| / max|ref| over that row, in float64 -> [rows]."""
    a = torch.as_tensor(a).detach().cpu().double().reshape(ref.shape[0], -1)
    ref = torch.as_tensor(ref).detach().cpu().double().reshape(ref.shape[0], -1)
    return (a - ref).abs().amax(1) / ref.abs().amax(1)


def e32(o32, ref):
    """The fp32 oracle's own error at one tap: the largest ``row_err`` over the rows compared."""
    return float(row_err(o32, ref).max())
