"""The case grid of tests/test_step2d_f64_host.py (CPU, a pixel-wise toy model) and tests/test_gpu_step2d_f64.py (MI355X, the library):
the 2-D reverse-step updates under every option that decides which copy, which divisor, which x, which clamp order and which noise.
Data, the seeded states and the toy model; nothing here touches a device."""

OBJECTIVES = ("pred_noise", "pred_x0", "pred_v")
X_SCALE = 0.7                   # seeded normal states
BNB = ((1, 1), (1, 2), (2, 3), (3, 2), (1, 5))       # (designs, boundary copies): no sharing at all | the goldens' | odd, B < nb | B > nb | one design, five copies
STEP_T = (0, 1, 500, 999)
SHARE, AVG, CLIP, REDERIVE = (True, False), (True, False), (True, False), (False, True)
CHANNELS = 21                   # CP = 24: group 4 (channels 16-19) straddles the state / boundary seam at 18, group 5 is one channel and three pads
CHANNELS_ALIGNED = 15           # CP = 16: the seam (12) is a group boundary, one pad lane
BETA_SCHEDULE = "sigmoid"       # GaussianDiffusion's default

# update2d_kernel: (share_noise, use_average_share, clip, t) through the step entry, (.., rederive, t) through the predict entry
STEP_OPTIONS = [(s, a, c, t) for s in SHARE for a in AVG for c in CLIP for t in STEP_T]
PREDICT_OPTIONS = [(s, a, c, r, t) for s in SHARE for a in AVG for c in CLIP for r in REDERIVE for t in STEP_T]

# ddim2d_update_kernel: S = 50, the pairs (the last one has time_next = -1), eta, mean / sum
DDIM_S, DDIM_PAIRS, DDIM_ETA = 50, (0, 1, 25, 49), (0.0, 0.5)
DDIM_OPTIONS = [(a, eta, i) for a in AVG for eta in DDIM_ETA for i in DDIM_PAIRS]
# ddim2d_guided_update_kernel (64 x 64, the size the surrogate is built for)
GUIDED_PAIRS, GUIDED_ETA, GUIDED_BNB, GUIDED_COEFF_RATIO = (0, 25, 49), 0.5, ((1, 2), (2, 2)), 0.05
REFUSAL_DDIM_NOSHARE = "DDIM with share_noise=False"


def state_is_shared(*flags):
    """Half of the cases run on a state whose state channels are shared over the boundary copies of a design (what a chain reaches),
    half on one where every copy has its own (what tells copy k's x from copy 0's): by the parity of the case's option flags."""
    return sum(int(bool(f)) for f in flags) % 2 == 0


def make_state(C, B, nb, t, shared, size):
    """x [B * nb, C, size, size] fp32, normal x 0.7, seeded per argument tuple."""
    import torch
    g = torch.Generator().manual_seed(1000003 * C + 10007 * B + 1009 * nb + 7 * t + 3 * size + int(shared))
    x = torch.randn((B, nb, C, size, size), generator=g) * X_SCALE
    if shared:
        x[:, :, :-3] = x[:, :1, :-3]
    return x.reshape(B * nb, C, size, size).contiguous()


def make_noise(C, B, nb, t, size):
    """The step's draw as sample_noise shapes it: (state [B, 1, C - 3, size, size], boundary [B, nb, 3, size, size])."""
    import torch
    g = torch.Generator().manual_seed(900001 + 1000003 * C + 10007 * B + 1009 * nb + 7 * t + 3 * size)
    return torch.randn((B, 1, C - 3, size, size), generator=g), torch.randn((B, nb, 3, size, size), generator=g)


def toy_model(x, t):
    """A pixel-wise stand-in for the U-Net: every output element depends on two OTHER channels of its own pixel and on t (an output
    that follows its own channel cancels against x in predict_start_from_noise / _from_v and leaves the clamp nothing to do).  Only
    sums, products, a quotient and a square root, each correctly rounded in float64 and taken in a fixed order: the same bits on
    every machine, so a golden file need not carry it, and (rounded last) the same fp32 value whatever the batch.  |E| < 1.8, above
    1 on about half of the elements of a 0.7-sigma state: the clamp acts on part of x_start under every objective at t = 500."""
    import torch
    xd = x.double()
    y = 0.8 * torch.roll(xd, 1, dims=1) - 0.6 * torch.roll(xd, 5, dims=1)
    y = 1.5 * y + 0.3 * (t.double().view(-1, 1, 1, 1) / 1000.0)
    return (1.8 * y / torch.sqrt(1.0 + y * y)).to(x.dtype)


# ---- the golden of oracle/make_golden_step2d.py (tests/golden/step2d_grid.npz): the reference's own execution on the toy model.
# Every option combination of the two update2d grids above under every objective at every (B, nb) of BNB (1440 records), on
# GOLDEN_SIZE x GOLDEN_SIZE images with un-shared states.  Why not 8 x 8: a record is two or three tensors of B * nb * 21 * size^2
# floats; the grid is 72 MB of floats at 8 x 8 and 4.5 MB at 2 x 2, and the committed-file limit is 1 MiB (at 1 x 1: 0.25 MB packed).
# The toy model is pixel-wise, so a 1 x 1 image is one pixel of an 8 x 8 one: the reference's arithmetic per element -- which copies,
# which divisor, which x, where the clamp sits -- is the same, every record still has B * nb * 21 elements, and the fp32 oracle, which
# the golden pins, runs the same grid at 8 x 8 in the test itself.
GOLDEN_SIZE = 1
HOST_SIZE = 8


def golden_records():
    """[(name, entry, objective, share_noise, avg, clip, rederive, t, B, nb)] in file order."""
    out = []
    for obj in OBJECTIVES:
        for (s, a, c, t) in STEP_OPTIONS:
            for B, nb in BNB:
                out.append((f"step.{obj}.s{int(s)}a{int(a)}c{int(c)}.t{t}.B{B}nb{nb}", "p_mean_variance", obj, s, a, c, False, t, B, nb))
    for obj in OBJECTIVES:
        for (s, a, c, r, t) in PREDICT_OPTIONS:
            for B, nb in BNB:
                out.append((f"predict.{obj}.s{int(s)}a{int(a)}c{int(c)}r{int(r)}.t{t}.B{B}nb{nb}", "model_predictions", obj, s, a, c, r, t, B, nb))
    return out
