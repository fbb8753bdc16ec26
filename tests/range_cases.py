"""The cases of tests/test_f64_range_host.py (CPU) and tests/test_gpu_f64_range.py (MI355X): the edges of the split-fp16 range rule.

Plain helper: no test, no fixture.  The rule (``max_abs_in_fp16_window``, csrc/handle_core.inc) keeps a tensor on the split-fp16
kernels while 2^-12 <= max|w| <= 2^15.  ``to_edge`` puts a tensor's largest magnitude exactly on an edge or one fp32 number beyond
it; ``split_planes`` is the host model of the two fp16 planes; ``ruled_*`` restate which tensors each finalize inspects; the case
tables below say which tensors are moved, at which sizes they run and what ``range_fallback`` must read.

A convolution that is moved keeps its function up to a constant: its bias is multiplied by the same factor as its weight (the
GroupNorm / LayerNorm behind it removes the constant; behind ``final_conv`` it scales eps).  Without that the bias, left at unit
scale, would be 100 times the products at the lower edge and hide them from every tap.
"""
import numpy as np
import torch

import cindm_oracle as O

LO = 2.0 ** -12                 # the window of max_abs_in_fp16_window
HI = 2.0 ** 15
FP16_MIN_NORMAL = 2.0 ** -14
H3_SCALE = 2048.0               # lo = fp16((v - hi) * 2^11)
WS_TINY = 2.0 ** -24            # factor of the .proj. weights in the ws-tiny cases


def beyond(edge):
    """The fp32 neighbour of ``edge`` on the far side of the window: nextafter(2^-12, 0) / nextafter(2^15, inf)."""
    e = np.float32(edge)
    return float(np.nextafter(e, np.float32(0.0 if edge < 1.0 else np.inf)))


def to_edge(w, edge, outside=False):
    """fp32(w * edge / max|w|), computed in float64 and clamped to +-edge, the element of largest magnitude exactly +-edge.
    ``outside``: that element is the fp32 neighbour beyond the edge instead (``beyond``), every other one clamped to it."""
    w64 = w.detach().double()
    i = int(w64.abs().argmax())
    top = beyond(edge) if outside else float(edge)
    out = (w64 * (float(edge) / float(w64.abs().flatten()[i]))).float().clamp(-top, top)
    out.view(-1)[i] = top if float(w64.flatten()[i]) > 0 else -top
    return out.contiguous()


def split_planes(w, flush):
    """Host model of the planes the pack writes: hi = fp16(w), lo = fp16((w - hi) * 2^11), both from fp32 arithmetic as in the
    library's pack loops.  ``flush``: fp16 subnormals (|v| < 2^-14) become 0, as a pipeline without subnormal support would leave
    them -- True: in both planes (at max|w| = 2^-12 a quarter of the tensor is lost outright); "lo": in the low plane only, the
    subtle form (the 2^-24 promise becomes 2^-13).  -> (hi, lo) as float64; the product uses hi + lo / 2^11."""
    w = w.detach().float()
    hi = w.half()
    lo = ((w - hi.float()) * H3_SCALE).half()
    hi, lo = hi.double(), lo.double()
    if flush and flush != "lo":
        hi = torch.where(hi.abs() < FP16_MIN_NORMAL, torch.zeros_like(hi), hi)
    if flush:
        lo = torch.where(lo.abs() < FP16_MIN_NORMAL, torch.zeros_like(lo), lo)
    return hi, lo


def planes_value(w, flush):
    hi, lo = split_planes(w, flush)
    return hi + lo / H3_SCALE


def plane_error(w, flush):
    """max|w - (hi + lo / 2^11)| / max|w|."""
    return float((w.double() - planes_value(w, flush)).abs().max() / w.double().abs().max())


def ws_folded(w):
    """WeightStandardizedConv2d folded into the weights, as the 2-D finalizes do: (w - mean) / sqrt(var + 1e-5) per filter, fp32."""
    w = w.float()
    mean = w.mean(dim=(1, 2, 3), keepdim=True)
    var = w.var(dim=(1, 2, 3), unbiased=False, keepdim=True)
    return (w - mean) * (var + 1e-5).rsqrt()


# ------------------------------------------------------------------ which tensors each finalize inspects
def ruled_1d(sd):
    """cindm_unet1d_finalize: ``shape.size() >= 2`` and no ``time_mlp`` in the name."""
    return [k for k, v in sd.items() if v.dim() >= 2 and "time_mlp" not in k]


def ruled_2d(sd):
    """unet2d_finalize_pack, unfolded tensors: ``shape.size() == 4`` and no ``.proj.`` in the name (the ``.proj.`` ones are checked
    after the weight standardisation is folded in: ``ws_folded``)."""
    return [k for k, v in sd.items() if v.dim() == 4 and ".proj." not in k]


def ruled_force(sd):
    """cindm_forceunet_finalize: the same filter as the 2-D U-Net's."""
    return ruled_2d(sd)


def gauge_1d(sd):
    """The ruled 1-D tensors with ``.block.0.`` in their name: a GroupNorm follows them, so their scale is free."""
    return [k for k in ruled_1d(sd) if ".block.0." in k]


def moved(sd, names, edge, outside=()):
    """``sd`` with the tensors ``names`` at ``edge`` (those of ``outside`` one float beyond it) and their biases scaled alike."""
    out = dict(sd)
    for k in names:
        out[k] = to_edge(sd[k], edge, outside=k in outside)
        b = k[:-len(".weight")] + ".bias" if k.endswith(".weight") else None
        if b in sd:
            out[b] = (sd[b].double() * (float(edge) / float(sd[k].double().abs().max()))).float()
    return out


# ------------------------------------------------------------------ 1-D: TemporalUnet1D(24, 8), weight seed 0, t = 77, x = randn, seed 4100 + B
T_1D = 77
SEED_X_1D = 4100
DEEP_1D = "downs.3.0.blocks.0.block.0.weight"
# one tensor per kernel family: level0, level1, dconv2, dconv2 (bottleneck), ups tail / last, final
SINGLE_1D = ["downs.0.0.blocks.0.block.0.weight", "downs.1.0.blocks.0.block.0.weight", DEEP_1D, "mid_block1.blocks.0.block.0.weight",
             "ups.2.1.blocks.1.block.0.weight", "final_conv.0.block.0.weight"]
# the option sets of test_gpu_paths.PATHS_1D that change which kernel stages weight planes
OPTIONS_1D = [{"local_gn": 0}, {"attn_site": 0}, {"level0": 0}, {"level1": 0}, {"level1": 2}, {"ups_last": 0}, {"ups_tail": 0}, {"dconv2": 0},
              {"dresample": 0}, {"dconv": 0}, {"attn_head": 0}, {"attn_head": 2}, {"dconv": 0, "level0": 0, "attn_head": 0}, {"no_exchange": 1}]


def base_1d():
    return O.synth_state_dict(O.unet1d_param_shapes(24, 8, attention=True), seed=0)


def scaled_1d(scale_w=1.0, gamma=None):
    """``_scaled`` of tests/test_gpu_range.py: every ``.block.0.`` tensor (weight and bias) x scale_w, GroupNorm gains x gamma."""
    out = {}
    for k, v in base_1d().items():
        out[k] = v * scale_w if ".block.0." in k else v * gamma if (gamma is not None and ".block.2.weight" in k) else v
    return out


def _edge_1d(edge, outside=()):
    sd = base_1d()
    return moved(sd, gauge_1d(sd) + ["final_conv.1.weight"], edge, outside)


def _all_ruled_lo():
    sd = base_1d()
    return moved(sd, ruled_1d(sd), LO)


def _single(name):
    sd = base_1d()
    return moved(sd, [name], LO)


# name -> (weights, rows, expected range_fallback, input amplitude or None[, input seed base])
# (1d-scale-1e-4, 1d-amp-6e4: at seed 4100 + 5 a fourth tap, downs.0.3, has e32 1.9e-7 / 2.2e-7, under or at the floor of the
# yardsticks; the seeds moved -- there it is above 2.6e-7 -- and the condition of BELOW_FLOOR did not)
CASES_1D = {
    "1d-lo-in": (lambda: _edge_1d(LO), (9, 17, 321), 0, None),
    "1d-hi-in": (lambda: _edge_1d(HI), (9, 17), 0, None),
    "1d-lo-out": (lambda: _edge_1d(LO, (DEEP_1D,)), (17,), 1, None),
    "1d-hi-out": (lambda: _edge_1d(HI, (DEEP_1D,)), (17,), 1, None),
    "1d-all-ruled-lo": (_all_ruled_lo, (17,), 0, None),
    **{"1d-one-" + n[:-len(".block.0.weight")]: ((lambda n=n: _single(n)), (17,), 0, None) for n in SINGLE_1D},
    # tests/test_gpu_range.py's own scales, with the fallback that file states
    "1d-scale-100": (lambda: scaled_1d(100.0), (5,), 0, None),
    "1d-scale-3e3": (lambda: scaled_1d(3.0e3), (5,), 0, None),
    "1d-scale-1e-3": (lambda: scaled_1d(1.0e-3), (5,), 1, None),
    "1d-scale-1e-4": (lambda: scaled_1d(1.0e-4), (5,), 1, None, 4400),
    "1d-scale-1e6": (lambda: scaled_1d(1.0e6), (5,), 1, None),
    "1d-gamma-50": (lambda: scaled_1d(gamma=50.0), (5,), 0, None),
    "1d-amp-6e4": (lambda: scaled_1d(), (5,), 0, 6.0e4, 4500),
    "1d-amp-1e-3": (lambda: scaled_1d(), (5,), 0, 1.0e-3),
}


def input_1d(B, amp=None, seed=SEED_X_1D):
    x = torch.randn((B, 24, 8), generator=torch.Generator().manual_seed(seed + B))
    return x if amp is None else (x / x.abs().max()) * amp


def rows_compared(B):
    """As tests/test_gpu_f64_budget.py: all rows up to 65; above, the first 17, the last 17 and every 29th in between."""
    return list(range(B)) if B <= 65 else list(range(17)) + list(range(17, B - 17, 29)) + list(range(B - 17, B))


# ------------------------------------------------------------------ 2-D: Unet(64, (1, 2), 21), weight seed 3, two images, t = 500
T_2D = 500
SEED_X_2D = 5700


def base_2d():
    return O.synth_state_dict_2d(O.unet2d_param_shapes(64, (1, 2), 21), 3)


def ws_tiny(sd):
    return {k: (v * WS_TINY if k.endswith(".proj.weight") else v) for k, v in sd.items()}


def _hi_names_2d(sd):
    """The tensors a LayerNorm follows (the four LinearAttention output projections) and the last convolution."""
    return [k for k in sd if k.endswith(".to_out.0.weight")] + ["final_conv.weight"]


def _2d(names_of, edge, outside=()):
    sd = base_2d()
    return moved(sd, names_of(sd), edge, outside)


OPTIONS_2D = [{"conv_ws": 0}, {"tail_h3": 0}, {"la_site": 0}, {"ws_nosplit": 1}]

# name -> (weights, image size, expected range_fallback)
CASES_2D = {
    "2d-lo-in-32": (lambda: _2d(ruled_2d, LO), 32, 0),
    "2d-lo-in-64": (lambda: _2d(ruled_2d, LO), 64, 0),
    "2d-lo-out": (lambda: _2d(ruled_2d, LO, ("downs.1.3.weight",)), 32, 1),
    "2d-hi-in": (lambda: _2d(_hi_names_2d, HI), 32, 0),
    "2d-hi-out": (lambda: _2d(_hi_names_2d, HI, ("final_conv.weight",)), 32, 1),
    "2d-ws-tiny": (lambda: ws_tiny(base_2d()), 32, 1),
}


def input_2d(size, n=2):
    return torch.randn((n, 21, size, size), generator=torch.Generator().manual_seed(SEED_X_2D + size))


# ------------------------------------------------------------------ ForceUnet: default model, weight seed 7, input seed 37, lambda_force 0.9
SEED_X_FORCE = 37
LAMBDA_FORCE = 0.9
IMAGES_FORCE = (2, 3)


def base_force():
    return O.synth_state_dict_2d(O.force_unet_param_shapes(), 7)


def _force(names_of, edge):
    sd = base_force()
    return moved(sd, names_of(sd), edge)


# name -> (weights, expected range_fallback)
CASES_FORCE = {
    "force-lo-in": (lambda: _force(ruled_force, LO), 0),
    "force-hi-in": (lambda: _force(lambda sd: [k for k in sd if k.endswith(".to_out.0.weight")], HI), 0),
    "force-ws-tiny": (lambda: ws_tiny(base_force()), 1),
}


def input_force():
    return torch.randn((max(IMAGES_FORCE), 4, 64, 64), generator=torch.Generator().manual_seed(SEED_X_FORCE))


# ------------------------------------------------------------------ taps whose fp32-oracle error is under the 2e-7 floor of ``_hold``
# tests/test_gpu_f64_budget.py::_hold asserts that every yardstick e32 is above 2e-7, except at the taps it is told about; there the
# yardstick is one fp32 ulp, 2^-23.  Pinned by tests/test_f64_range_host.py::test_yardsticks, measured on the CPU (largest e32 over the
# case's sizes, in 1e-7: lo-in / lo-out 1.7 2.0 2.0; scale-1e-3 1.2 1.6 1.6; scale-1e-4 1.1 1.2 1.5; amp-6e4 1.3 1.2 1.5).  The first
# block's GroupNorms see a variance near their eps of 1e-5 there and hand on little more than their bias.  THE CONDITION: at most three
# taps per case, each of them ``init_conv`` or a ``downs.0.*`` tap -- never eps / out / dx or a deeper tap.
# (The fp32 oracle's rounding depends on how torch splits its convolutions over CPU threads: the figures are those of 4, 8 and 16
# threads, which agree on the pinned sets; a single thread rounds eps of the two small-scale cases less, 1.0e-7.)
_FIRST_LEVEL = ("downs.0.0", "downs.0.1", "downs.0.2")
BELOW_FLOOR = {"1d-lo-in": _FIRST_LEVEL, "1d-lo-out": _FIRST_LEVEL, "1d-scale-1e-3": _FIRST_LEVEL, "1d-scale-1e-4": _FIRST_LEVEL,
               "1d-amp-6e4": _FIRST_LEVEL}
# ForceUnet: the gradient at mid_block2 is the head's derivative, one multiply per element (tests/test_gpu_f64_budget_force.py leaves
# it out for every case).  force-ws-tiny is outside the condition and no seed can bring it in: with the folded .proj. weights at 1e-6
# every Block hands on SiLU(beta) and the bottleneck no longer depends on the image -- ``out`` moves by 1e-2 of itself between images,
# and the gradient at mid_attn is the same tensor for every image, one addition away from the one at mid_block2 (e32 1.08e-7 at every
# input seed tried; ``out`` 1.4e-7 .. 1.9e-7; the gradients at mid_block1 and downs.3.3, two and three such steps upstream, 2.1e-7 ..
# 2.9e-7, on either side of the floor).  test_yardsticks asserts that image-independence instead.
BELOW_FLOOR_FORCE = ("grad:mid_block2",)
DEGENERATE = {"force-ws-tiny": ("out", "grad:mid_attn", "grad:mid_block1", "grad:downs.3.3")}
