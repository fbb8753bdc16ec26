"""Host model (numpy) of the library's counter-based Gaussian generator, written from cindm_amd/csrc/kernels.h
(philox4x32_10, counter_normal, counter_normal4, fill_normal_kernel) and kernels2d.h (noise2d_state4, noise2d_bound4,
fill_noise2d_kernel), plus the ledger of every keyed stream the sampling chains draw from.  Checker only.

Three layers:
  * ``philox4x32_10``: the integer core (Random123's Philox4x32 with 10 rounds), vectorised over uint32 arrays;
  * ``uniform24``: the uniforms exactly as the kernel forms them, in fp32: u = (float(r >> 8) + 0.5f) * 2^-24.  For
    r >> 8 >= 2^23 the sum k + 0.5 does not fit 24 bits and rounds to even, so u reaches exactly 1.0 (k = 2^24 - 1: radius 0);
    the smallest u is 2^-25, so |z| <= sqrt(-2 ln 2^-25) = 5.887...;  a model that formed u in float64 would differ from the
    kernel by O(1e-7) in u;
  * Box-Muller in float64 from those fp32 inputs (the device's logf / sqrtf / sincosf are not correctly rounded, so a device
    draw equals the model only to a few fp32 ulps of the result -- tests/test_gpu_counter_ledger.py measures it).
"""
import numpy as np

M32 = 0xFFFFFFFF
M64 = 0xFFFFFFFFFFFFFFFF
PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85
TWO_PI_F32 = np.float32(6.283185307179586)
Z_MAX = float(np.sqrt(-2.0 * np.log(2.0 ** -25)))          # 5.8871...

# seed words of the streams (xor'd into the seed; the 32-bit ones touch the low key word only)
RELAX_XOR = 0x7f4a7c15                  # kernels.h compose_update_element: relaxation draws
INPAINT_XOR = 0x5bd1e995                # kernels.h compose_update_element: inpainting rows
KNOWN1D_XOR = 0x6b6e6f776e316421        # kernels.h kKnown1dSeed
BOUND2D_XOR = 0x9e3779b97f4a7c15        # kernels2d.h noise2d_bound4
KNOWN2D_XOR = 0x6b6e6f776e326421        # kernels2d.h kKnown2dSeed
SEGMENT_STRIDE = 0x9E3779B97F4A7C15     # diffusion1d.autoregress_segment_seeds
RELAX_WORD = 0x10000                    # relaxation r of the step at t: word RELAX_WORD * (r + 1) + t
ULA_WORD = 0x80000000                   # Langevin iteration l of timestep t: word ULA_WORD + 65536 * l + t


def philox4x32_10(c0, c1, c2, c3, k0, k1, rounds=10):
    """Philox4x32-R on uint32 arrays (broadcast against each other); returns the four output words as uint32 arrays."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & np.uint64(M32) for c in (c0, c1, c2, c3))
    c0, c1, c2, c3 = np.broadcast_arrays(c0, c1, c2, c3)
    k0, k1 = int(k0) & M32, int(k1) & M32
    m32 = np.uint64(M32)
    for _ in range(rounds):
        p0 = np.uint64(PHILOX_M0) * c0                       # 32 x 32 -> 64 bits: no overflow in uint64
        p1 = np.uint64(PHILOX_M1) * c2
        n0 = (p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0)
        n1 = p1 & m32
        n2 = (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1)
        n3 = p0 & m32
        c0, c1, c2, c3 = n0, n1, n2, n3
        k0, k1 = (k0 + PHILOX_W0) & M32, (k1 + PHILOX_W1) & M32
    return tuple(c.astype(np.uint32) for c in (c0, c1, c2, c3))


def uniform24(r):
    """The kernel's uniform of one 32-bit output, in fp32: (float(r >> 8) + 0.5f) * 2^-24, each operation rounded to fp32."""
    k = (np.asarray(r, dtype=np.uint32) >> np.uint32(8)).astype(np.float32)          # < 2^24: exact
    return (k + np.float32(0.5)) * np.float32(1.0 / 16777216.0)


def box_muller(u1, u2):
    """(radius * cos, radius * sin) in float64 from the fp32 uniforms; the angle is the fp32 product 2 pi_f32 * u2."""
    u1, u2 = np.asarray(u1, dtype=np.float32), np.asarray(u2, dtype=np.float32)
    ang = (TWO_PI_F32 * u2).astype(np.float32).astype(np.float64)
    rad = np.sqrt(-2.0 * np.log(u1.astype(np.float64)))
    return rad * np.cos(ang), rad * np.sin(ang)


def counter_words(seed, sample, word, elem4):
    """The four Philox outputs of (seed, sample, word, group of four elements): counter (elem >> 2, sample & M32, word,
    sample >> 32), key (seed & M32, seed >> 32).  ``sample`` and ``elem4`` may be arrays (uint64 / any integer)."""
    seed = int(seed) & M64
    sample = np.asarray(sample, dtype=np.uint64)
    return philox4x32_10(np.asarray(elem4, dtype=np.uint64), sample & np.uint64(M32), np.uint64(int(word) & M32),
                         sample >> np.uint64(32), seed & M32, seed >> 32)


def counter_normal(seed, sample, word, elem):
    """float64 model of counter_normal(seed, sample, step = word, elem): element j of a group of four uses the outputs
    (r[j & 2], r[(j & 2) + 1]) -- cosine for even j, sine for odd."""
    elem = np.asarray(elem, dtype=np.uint64)
    sample = np.asarray(sample, dtype=np.uint64)
    elem, sample = np.broadcast_arrays(elem, sample)
    r = counter_words(seed, sample, word, elem >> np.uint64(2))
    j = (elem & np.uint64(3)).astype(np.int64)
    hi = (j & 2) != 0
    ra, rb = np.where(hi, r[2], r[0]), np.where(hi, r[3], r[1])
    c, s = box_muller(uniform24(ra), uniform24(rb))
    return np.where((j & 1) != 0, s, c)


def fill_normal(B, per, seed, offset, word):
    """What cindm_fill_normal writes: [B, per] float64, out[b, e] = counter_normal(seed, offset + b, word, e)."""
    sample = (np.uint64(int(offset) & M64) + np.arange(B, dtype=np.uint64))[:, None]
    return counter_normal(seed, sample, word, np.arange(per, dtype=np.uint64)[None, :])


def noise2d_state(seed, design, word, pix, G, g):
    """noise2d_state4: the four normals of channel group g of pixel pix, keyed by the DESIGN; [..., 4]."""
    e4 = np.asarray(pix, dtype=np.uint64) * np.uint64(G) + np.asarray(g, dtype=np.uint64)
    return counter_normal(seed, np.asarray(design, dtype=np.uint64)[..., None], word,
                          e4[..., None] * np.uint64(4) + np.arange(4, dtype=np.uint64))


def noise2d_bound(seed, image, word, pix, G, g):
    """noise2d_bound4: as noise2d_state, keyed by the IMAGE under seed ^ BOUND2D_XOR."""
    return noise2d_state((int(seed) ^ BOUND2D_XOR) & M64, image, word, pix, G, g)


def fill_noise2d(B, nb, HW, C, CP, seed, offset, word):
    """What cindm_fill_noise2d writes: [B * nb, HW, CP] float64 (channel-last, CP = C padded to a multiple of 4).  Channels
    c < C - 3 (state) are keyed by the design offset + b and so equal over its nb boundary copies; channels C - 3 .. C - 1
    (boundary) by the image (offset + b) * nb + k under the xor'd seed; the padding lanes c >= C hold 0."""
    G, Cs = CP // 4, C - 3
    im = np.arange(B * nb, dtype=np.uint64)[:, None, None]
    pix = np.arange(HW, dtype=np.uint64)[None, :, None]
    g = np.arange(G, dtype=np.uint64)[None, None, :]
    im, pix, g = np.broadcast_arrays(im, pix, g)
    b = im // np.uint64(nb)
    design = np.uint64(int(offset) & M64) + b
    image = design * np.uint64(nb) + (im - b * np.uint64(nb))
    zs = noise2d_state(seed, design, word, pix, G, g).reshape(B * nb, HW, CP)
    zb = noise2d_bound(seed, image, word, pix, G, g).reshape(B * nb, HW, CP)
    c = np.arange(CP)[None, None, :]
    return np.where(c >= C, 0.0, np.where(c < Cs, zs, zb))


# ---------------------------------------------------------------------------------------------------------------------
# The draw ledger: every keyed stream of the sampling chains, read off the kernels (the code is the authority; DESIGN 4.4
# prints this table and tests/test_counter_noise_host.py checks the two against each other).
#   seed_word(seed)        the 64-bit key
#   step_word(t, r, l, T)  the third counter word: t the timestep (DDIM: the step's timestep, not its index), r the relaxation
#                          index, l the Langevin inner iteration, T = num_timesteps
#   sample / element       what the second / first counter words index
#   tape                   the NoiseTape / NoiseTape2D field an explicit tape feeds the same draw through
def _x(c):
    return lambda seed: (int(seed) ^ c) & M64


STREAMS = [
    dict(name="x_T", seed_xor=0, seed_word=_x(0), step_word=lambda t, r, l, T: T,
         step="T", sample="sample_offset + b", element="l * F + f of the (composed) state", tape="init",
         where="fill_normal_kernel, autoregress_handover_kernel; diffusion1d._init_state"),
    dict(name="step", seed_xor=0, seed_word=_x(0), step_word=lambda t, r, l, T: t,
         step="t  (DDPM: t > 0; DDIM: only where sigma != 0)", sample="sample_offset + b",
         element="l * F + f of the composed state", tape="step[t]  (DDIM: step[i])",
         where="compose_update_element; ups_last_kernel's fused tail"),
    dict(name="relaxation", seed_xor=RELAX_XOR, seed_word=_x(RELAX_XOR), step_word=lambda t, r, l, T: RELAX_WORD * (r + 1) + t,
         step="0x10000 * (r + 1) + t", sample="sample_offset + b", element="l * F + f of the composed state",
         tape="recur[t][r]  (DDIM: recur[i][r])", where="compose_update_element; ddpm1d_host.inc recur_tag"),
    dict(name="inpainting", seed_xor=INPAINT_XOR, seed_word=_x(INPAINT_XOR), step_word=lambda t, r, l, T: t,
         step="t", sample="sample_offset + b", element="l * F + f of the state row (l < the condition's rows)",
         tape="cond[t]  (DDIM: cond[i])", where="compose_update_element"),
    dict(name="known-1d-init", seed_xor=KNOWN1D_XOR, seed_word=_x(KNOWN1D_XOR), step_word=lambda t, r, l, T: T,
         step="T", sample="sample_offset + b", element="l * F + f of the full state", tape="known_init",
         where="known1d_kernel mode 1"),
    dict(name="known-1d-step", seed_xor=KNOWN1D_XOR, seed_word=_x(KNOWN1D_XOR), step_word=lambda t, r, l, T: t,
         step="the level reached (DDPM: t - 1; DDIM: t_next), >= 0", sample="sample_offset + b",
         element="l * F + f of the full state", tape="known_step[t]  (DDIM: known_step[i])", where="known1d_kernel mode 0"),
    dict(name="known-1d-relaxation", seed_xor=KNOWN1D_XOR, seed_word=_x(KNOWN1D_XOR),
         step_word=lambda t, r, l, T: RELAX_WORD * (r + 1) + t,
         step="0x10000 * (r + 1) + t", sample="sample_offset + b", element="l * F + f of the full state",
         tape="known_recur[t][r]  (DDIM: known_recur[i][r])", where="known1d_kernel mode 2"),
    dict(name="langevin", seed_xor=0, seed_word=_x(0), step_word=lambda t, r, l, T: ULA_WORD + 65536 * l + t,
         step="0x80000000 + 65536 * l + t", sample="sample_offset + b",
         element="l * F + f of the full state, conditioning rows included", tape="ula[N - 1 - t][l]", where="ula_update_kernel"),
    dict(name="2d-state", seed_xor=0, seed_word=_x(0), step_word=lambda t, r, l, T: t,
         step="t  (x_T: T)", sample="design: sample_offset + b", element="pix * CP + c, c < C - 3", tape="init[0], step_state",
         where="noise2d_state4; update2d / ddim2d kernels, fill_noise2d_kernel"),
    dict(name="2d-boundary", seed_xor=BOUND2D_XOR, seed_word=_x(BOUND2D_XOR), step_word=lambda t, r, l, T: t,
         step="t  (x_T: T)", sample="image: (sample_offset + b) * nb + k", element="pix * CP + c, C - 3 <= c < C",
         tape="init[1], step_boundary", where="noise2d_bound4"),
    dict(name="known-2d-state", seed_xor=KNOWN2D_XOR, seed_word=_x(KNOWN2D_XOR), step_word=lambda t, r, l, T: t,
         step="the level reached (rule 1: T)", sample="design", element="as 2d-state", tape="known_init[0], known_state",
         where="known2d_kernel"),
    dict(name="known-2d-boundary", seed_xor=KNOWN2D_XOR ^ BOUND2D_XOR, seed_word=_x(KNOWN2D_XOR ^ BOUND2D_XOR),
         seed_text=f"seed ^ {KNOWN2D_XOR:#x} ^ {BOUND2D_XOR:#x}", step_word=lambda t, r, l, T: t,
         step="the level reached (rule 1: T)", sample="image", element="as 2d-boundary", tape="known_init[1], known_boundary",
         where="known2d_kernel"),
]
for _s in STREAMS:       # the 1-D and the 2-D chains are different models: no chain draws from both families
    _s["family"] = "2d" if "2d-" in _s["name"] else "1d"
STREAM = {s["name"]: s for s in STREAMS}
# which arguments a stream's word ranges over (the others are fixed): used by the disjointness test
STREAM_AXES = {"x_T": "", "step": "t", "relaxation": "tr", "inpainting": "t", "known-1d-init": "", "known-1d-step": "t",
               "known-1d-relaxation": "tr", "langevin": "tl", "2d-state": "t", "2d-boundary": "t", "known-2d-state": "t",
               "known-2d-boundary": "t"}


def segment_seed(seed, k):
    """Segment k of the autoregressive rollout draws every stream above under this seed (autoregress_segment_seeds)."""
    return (int(seed) + k * SEGMENT_STRIDE) & M64


def stream_words(name, T, n_relax, n_langevin):
    """Every step word the stream can take for t < T (x_T streams: the tag T, and the 2-D streams: t <= T), relaxation
    r < n_relax and Langevin iteration l < n_langevin."""
    s, ax = STREAM[name], STREAM_AXES[name]
    ts = range(T + 1) if name.startswith(("2d-", "known-2d-")) else range(T) if "t" in ax else (0,)
    rs = range(n_relax) if "r" in ax else (0,)
    ls = range(n_langevin) if "l" in ax else (0,)
    return {s["step_word"](t, r, l, T) & M32 for t in ts for r in rs for l in ls}


def ledger_markdown():
    """The table DESIGN 4.4 holds, generated from STREAMS."""
    rows = ["| stream | seed word | step word | sample | element | tape field | where |", "|---|---|---|---|---|---|---|"]
    for s in STREAMS:
        sw = s.get("seed_text") or ("seed" if s["seed_xor"] == 0 else f"seed ^ {s['seed_xor']:#x}")
        rows.append(f"| {s['name']} | `{sw}` | {s['step']} | {s['sample']} | {s['element']} | `{s['tape']}` | {s['where']} |")
    # (a rule on the seed, not a stream of its own: segment_seed)
    rows.append(f"| autoregressive segment k | `(seed + k * {SEGMENT_STRIDE:#x}) mod 2^64` in place of `seed` | as x_T / step | as x_T / step "
                "| as x_T / step | `init[k]`, `step[k][i]` | autoregress_segment_seeds; cindm_ddpm1d_sample_autoregress |")
    return "\n".join(rows)
