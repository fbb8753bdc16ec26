"""The descriptor grid of tests/test_compose_f64_host.py (CPU, toy model) and tests/test_gpu_compose_f64.py (MI355X, the library).
Data only: a descriptor is (mode, n_bodies, n_windows, compose_start_step, cond_steps); the window is 24 everywhere."""

WINDOW = 24
X_SCALE = 0.7              # seeded normal states and conditions: the clamp bites on part of x_start, not on all of it
OBJECTIVES = ("pred_noise", "pred_x0", "pred_v")
WINDOWED = ("mean-inside", "sum-inside", "mean", "noise_sum")
OUTSIDE = ("mean", "noise_sum")
REFUSAL_OUTSIDE_COND = "outside composition with conditioned_steps > 0 is not supported"

# ---- the full cross: pred_noise, clip on, t = 500, B = 3
CROSS_T, CROSS_B = 500, 3
CROSS_NB = (2, 3, 4, 8)
CROSS_WCS = ((1, 4), (2, 24), (3, 16), (3, 4), (4, 1))        # one window | abutting (coverage 1 everywhere) | two strides | stride 1 (coverage up to 4)
CROSS_COND = (0, 4)
CROSS = [(m, nb, w, cs, k) for m in WINDOWED for nb in CROSS_NB for (w, cs) in CROSS_WCS for k in CROSS_COND]

# ---- the descriptors crossed with objective x clip x t x B
DESCRIPTORS = {
    "plain": ("plain", 2, 1, 0, 0),
    "mean-inside-nb2-w1": ("mean-inside", 2, 1, 4, 0),
    "sum-inside-nb2-w1": ("sum-inside", 2, 1, 4, 0),
    "mean-nb2-w1": ("mean", 2, 1, 4, 0),
    "noise_sum-nb2-w1": ("noise_sum", 2, 1, 4, 0),
    "sum-inside-nb3-w3-cs4": ("sum-inside", 3, 3, 4, 0),
    "noise_sum-nb4-w2-cs24-cond4": ("noise_sum", 4, 2, 24, 4),          # refused: REFUSAL_OUTSIDE_COND
    "mean-nb4-w3-cs16": ("mean", 4, 3, 16, 0),
    "mean-inside-nb8-w4-cs1": ("mean-inside", 8, 4, 1, 0),
    # noise_sum with more than one term per element under the three objectives: the per-pair pred_noise is re-derived from each
    # pair's x_start BEFORE the sum and x_start is predict_start_from_noise of the sum (model/diffusion_1d.py:1442-1459)
    "noise_sum-nb3-w2-cs10": ("noise_sum", 3, 2, 10, 0),
}
DESC_CLIP = (True, False)
DESC_T = (0, 1, 500, 999)
DESC_B = (1, 3)

# ---- multibody: p_mean_variance with the single-body model set (four bodies, cond 4, image_size 20), and gradient()
MB_COND, MB_T, MB_B = 4, (0, 200, 400), (1, 5)
GRADIENT_NB, GRADIENT_B, GRADIENT_T = (3, 4), (1, 5, 20), 200

# ---- the library's options under which the descriptors run once more at pred_noise
OPTIONS = ({"fuse_gather": 0}, {"no_exchange": 1})

# ---- the golden of oracle/make_golden_compose.py (tests/golden/compose_grid.npz): batch 2, t = 500, pred_noise, clip on
GOLDEN_T, GOLDEN_B = 500, 2
GOLDEN = {
    "sum-inside-nb3-w3-cs16": ("sum-inside", 3, 3, 16, 0),
    "noise_sum-nb4-w2-cs10": ("noise_sum", 4, 2, 10, 0),
    "mean-nb3-w2-cs24": ("mean", 3, 2, 24, 0),
    "mean-inside-nb2-w2-cs10-cond4": ("mean-inside", 2, 2, 10, 4),
    "mean-nb2-w2-cs10-cond4": ("mean", 2, 2, 10, 4),                    # the reference raises: the key "<name>.raises" holds its message
}


def make_state(desc, t, B):
    """(x [B, state rows, 4 nb], cond [B, cond_steps, 4 nb] | None), fp32: seeded per (descriptor, t, B), the same on both sides."""
    import torch
    mode, nb, w, cs, k = desc
    seed = 1000003 * (WINDOWED + ("plain", "multibody")).index(mode) + 10007 * nb + 1009 * w + 101 * cs + 11 * k + 7 * t + B
    g = torch.Generator().manual_seed(seed)
    rows = WINDOW + (w - 1) * cs - k
    x = torch.randn((B, rows, 4 * nb), generator=g) * X_SCALE
    cond = torch.randn((B, k, 4 * nb), generator=g) * X_SCALE if k else None
    return x, cond
