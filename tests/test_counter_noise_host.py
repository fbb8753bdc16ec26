"""CPU: the host model of the counter-based generator (oracle/counter_noise.py) and the draw ledger.

The model is the reference of tests/test_gpu_counter_ledger.py; here it is pinned on its own: the integer core against the
published Random123 known-answer vectors of philox4x32_10, the fp32 uniforms at their rounding edges, the moments of its
normals (test_counter_noise's bounds), and the ledger -- every keyed stream of the sampling chains as data -- for pairwise
disjoint (seed word, step word) pairs over the supported range, with the limits where disjointness ends stated as
assertions on the formulas."""
import itertools
import os

import numpy as np

import counter_noise as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ the integer core
def test_philox_known_answer_vectors():
    """Random123's kat_vectors for philox4x32_10: counter 0 / key 0, and the digits of pi."""
    out = N.philox4x32_10(0, 0, 0, 0, 0, 0)
    assert [int(o) for o in out] == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    out = N.philox4x32_10(0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344, 0xa4093822, 0x299f31d0)
    assert [int(o) for o in out] == [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]
    # (the third published vector: all ones)
    out = N.philox4x32_10(0xffffffff, 0xffffffff, 0xffffffff, 0xffffffff, 0xffffffff, 0xffffffff)
    assert [int(o) for o in out] == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
    # fewer rounds give other words: the vectors above pin the round count
    assert [int(o) for o in N.philox4x32_10(0, 0, 0, 0, 0, 0, rounds=9)] != [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]


def test_philox_is_vectorised_consistently():
    """Array arguments give what the scalar calls give (the fills below rely on it)."""
    c0 = np.array([0, 1, 0xffffffff, 12345], dtype=np.uint64)
    c1 = np.array([7, 0xfffffffe, 0, 3], dtype=np.uint64)
    vec = N.philox4x32_10(c0, c1, 1000, 1, 5, 0x80000000)
    for i in range(4):
        one = N.philox4x32_10(int(c0[i]), int(c1[i]), 1000, 1, 5, 0x80000000)
        assert [int(v[i]) for v in vec] == [int(o) for o in one]


def test_counter_layout():
    """counter = (elem >> 2, sample & M32, word, sample >> 32), key = (seed & M32, seed >> 32): the sample's high half and the
    seed's high half reach the generator, and the four elements of a group share one Philox call."""
    seed, sample, word = (1 << 63) + 12345, (1 << 32) + 5, 0x80000000 + 65536 + 402
    r = N.counter_words(seed, sample, word, 9)
    want = N.philox4x32_10(9, 5, word, 1, 12345, 1 << 31)
    assert [int(a) for a in r] == [int(b) for b in want]
    assert [int(a) for a in N.counter_words(seed, 5, word, 9)] != [int(b) for b in want]            # a truncated sample index
    assert [int(a) for a in N.counter_words(12345, sample, word, 9)] != [int(b) for b in want]      # a dropped high seed word
    z = N.counter_normal(seed, sample, word, np.arange(36, 40))
    c0, s0 = N.box_muller(N.uniform24(want[0]), N.uniform24(want[1]))
    c1, s1 = N.box_muller(N.uniform24(want[2]), N.uniform24(want[3]))
    assert np.array_equal(z, np.array([c0, s0, c1, s1]).reshape(4))


# ------------------------------------------------------------------ the uniforms
EDGE_K = (0, 1, 2 ** 23 - 1, 2 ** 23, 2 ** 24 - 1)


def test_uniform_edges():
    """u = (float(r >> 8) + 0.5f) * 2^-24 in fp32: exact below k = 2^23, round-to-even from there on, so u lies in (0, 1] and
    reaches 1.0 exactly; the low 8 bits of r do not matter."""
    r = np.array([(k << 8) | 0xff for k in EDGE_K], dtype=np.uint32)
    u = N.uniform24(r)
    assert u.dtype == np.float32
    assert np.array_equal(u, N.uniform24(np.array([k << 8 for k in EDGE_K], dtype=np.uint32)))
    want = [2.0 ** -25, 1.5 * 2.0 ** -24, (2.0 ** 23 - 0.5) * 2.0 ** -24, 0.5, 1.0]
    assert [float(v) for v in u] == want
    # a float64 model differs at and above k = 2^23: (2^23 + 0.5) / 2^24 != 0.5
    assert (EDGE_K[3] + 0.5) / 2.0 ** 24 != float(u[3]) and (EDGE_K[4] + 0.5) / 2.0 ** 24 != float(u[4])
    # every k: u in (0, 1]
    k = np.concatenate([np.arange(0, 4096), np.arange(2 ** 23 - 2048, 2 ** 23 + 2048), np.arange(2 ** 24 - 4096, 2 ** 24)])
    uu = N.uniform24((k.astype(np.uint64) << np.uint64(8)).astype(np.uint32))
    assert float(uu.min()) > 0.0 and float(uu.max()) == 1.0
    assert bool(np.all(np.diff(uu.astype(np.float64)) >= 0))


def test_normals_are_finite_and_bounded_at_the_edges():
    """|z| <= sqrt(-2 ln 2^-25) = 5.8871 and finite for every pair of edge uniforms (u1 = 1: radius 0; u1 = 2^-25: the largest
    radius; u2 = 1: the angle 2 pi in fp32) and over a block of ordinary draws."""
    assert abs(N.Z_MAX - 5.8871) < 1e-4
    ku = np.array([(k << 8) for k in EDGE_K], dtype=np.uint32)
    for a, b in itertools.product(ku, ku):
        c, s = N.box_muller(N.uniform24(a), N.uniform24(b))
        assert np.isfinite(c) and np.isfinite(s) and abs(c) <= 5.8871 and abs(s) <= 5.8871
    c, s = N.box_muller(N.uniform24(np.uint32((2 ** 24 - 1) << 8)), N.uniform24(np.uint32(12345 << 8)))
    assert c == 0.0 and s == 0.0                                                       # u1 == 1.0 exactly: radius 0
    c, _ = N.box_muller(N.uniform24(np.uint32(0)), N.uniform24(np.uint32(0)))
    assert abs(c) > 5.88                                                               # the bound is reached, not just respected
    z = N.fill_normal(8, 4096, 5, 0, 1000)
    assert bool(np.isfinite(z).all()) and float(np.abs(z).max()) <= 5.8871


def test_model_moments():
    """2 * 10^5 draws of the host model: test_counter_noise's bounds (tests/test_gpu_parity.py).  A sanity check of the model."""
    a = N.fill_normal(1024, 192, 5, 0, 1000)
    assert a.size >= 190000 and a.shape == (1024, 192)
    assert abs(float(a.mean())) < 0.01 and abs(float(a.var()) - 1.0) < 0.02
    assert abs(float((a ** 4).mean()) - 3.0) < 0.15
    assert float(np.abs(a).max()) < 7.0
    flat = a.ravel()
    assert abs(float((flat[:-1] * flat[1:]).mean())) < 0.01
    # a pure function of the global sample index: the second half of the batch is the batch at offset 512
    assert np.array_equal(a[512:], N.fill_normal(512, 192, 5, 512, 1000))


def test_fill_noise2d_model_structure():
    """The 2-D fill of the model: state channels shared over the boundary copies of a design, boundary channels per image under
    the xor'd seed, padding lanes zero, and a batch at offset 1 is the tail of the batch at offset 0."""
    B, nb, HW, C, CP = 3, 3, 16, 21, 24
    x = N.fill_noise2d(B, nb, HW, C, CP, 11, 0, 1000).reshape(B, nb, HW, CP)
    assert np.array_equal(x[:, 0, :, :18], x[:, 1, :, :18]) and np.array_equal(x[:, 0, :, :18], x[:, 2, :, :18])
    assert not np.array_equal(x[:, 0, :, 18:21], x[:, 1, :, 18:21])
    assert not np.array_equal(x[0, :, :, :18], x[1, :, :, :18])
    assert bool((x[..., 21:] == 0).all()) and bool((x[..., :21] != 0).all())
    assert np.array_equal(N.fill_noise2d(2, nb, HW, C, CP, 11, 1, 1000).reshape(2, nb, HW, CP), x[1:])
    # written out for one element of each kind: (design 1, copy 2, pixel 5) channel 7 (state) and channel 19 (boundary)
    assert x[1, 2, 5, 7] == float(N.counter_normal(11, 1, 1000, 5 * CP + 7))
    assert x[1, 2, 5, 19] == float(N.counter_normal(11 ^ N.BOUND2D_XOR, 1 * nb + 2, 1000, 5 * CP + 19))


# ------------------------------------------------------------------ the ledger
T_MAX, R_MAX, L_MAX = 1000, 16, 16


def test_ledger_streams_are_pairwise_disjoint():
    """Within one seed and one family of chains (1-D, 2-D), two streams never share a (seed word, step word) pair for T <= 1000,
    at most 16 relaxations and at most 16 Langevin iterations per timestep.  The seed words are xors of the seed with distinct
    constants, so they are compared through the constants."""
    for fam in ("1d", "2d"):
        streams = [s for s in N.STREAMS if s["family"] == fam]
        assert len(streams) >= 4
        words = {s["name"]: N.stream_words(s["name"], T_MAX, R_MAX, L_MAX) for s in streams}
        for a, b in itertools.combinations(streams, 2):
            for seed in (0, 5, (1 << 63) + 12345, N.M64):
                assert (a["seed_word"](seed) == b["seed_word"](seed)) == (a["seed_xor"] == b["seed_xor"])
            if a["seed_xor"] != b["seed_xor"]:
                continue
            hit = words[a["name"]] & words[b["name"]]
            assert not hit, (a["name"], b["name"], sorted(hit)[:4])
    # and within a stream with two axes, the word is injective on the range: no two (t, r) / (t, l) share a draw
    for name, n in (("relaxation", T_MAX * R_MAX), ("known-1d-relaxation", T_MAX * R_MAX), ("langevin", T_MAX * L_MAX)):
        assert len(N.stream_words(name, T_MAX, R_MAX, L_MAX)) == n


def test_ledger_limits_where_disjointness_ends():
    """The supported range is bounded by the word formulas themselves: these equalities are where two draws start to coincide."""
    w = lambda name, t=0, r=0, l=0, T=T_MAX: N.STREAM[name]["step_word"](t, r, l, T) & N.M32
    # t >= 0x10000: a step word reaches the first relaxation's words (same seed word for the known region's two streams)
    assert w("known-1d-step", t=0x10000) == w("known-1d-relaxation", t=0, r=0)
    assert w("step", t=0x10000) == w("relaxation", t=0, r=0)
    assert w("relaxation", t=0x10000, r=0) == w("relaxation", t=0, r=1)
    assert w("langevin", t=0x10000, l=0) == w("langevin", t=0, l=1)
    assert w("known-1d-step", t=0xffff) != w("known-1d-relaxation", t=0, r=0)
    # r + 1 >= 0x8000: a relaxation word reaches the Langevin words' base
    assert w("relaxation", t=7, r=0x8000 - 1) == w("langevin", t=7, l=0)
    assert w("relaxation", t=7, r=0x8000 - 2) < N.ULA_WORD
    # l >= 0x8000: the Langevin word wraps round 2^32 onto the step words (same seed word: a real collision)
    assert w("langevin", t=7, l=0x8000) == w("step", t=7)
    assert w("langevin", t=7, l=0x8000 - 1) >= N.ULA_WORD
    # T itself is the x_T tag: a chain with more than T_MAX levels would need t == T to collide, which no step has (t < T)
    assert w("x_T") == T_MAX and max(N.stream_words("step", T_MAX, R_MAX, L_MAX)) == T_MAX - 1
    assert N.STREAM["x_T"]["seed_xor"] == N.STREAM["step"]["seed_xor"] == N.STREAM["langevin"]["seed_xor"] == 0


def test_ledger_constants_are_the_codes():
    """The code is the authority: every constant of the ledger stands in the kernels, and the Python face mirrors the same ones."""
    from cindm_amd import diffusion1d, diffusion2d
    assert diffusion1d.KNOWN_SEED == N.KNOWN1D_XOR and diffusion2d.KNOWN_SEED == N.KNOWN2D_XOR
    assert diffusion1d._SEGMENT_SEED_STRIDE == N.SEGMENT_STRIDE
    assert diffusion1d.autoregress_segment_seeds(N.M64 - 3, 3) == [N.segment_seed(N.M64 - 3, k) for k in range(3)]
    csrc = os.path.join(ROOT, "cindm_amd", "csrc")
    k1 = open(os.path.join(csrc, "kernels.h")).read()
    k2 = open(os.path.join(csrc, "kernels2d.h")).read()
    host = open(os.path.join(csrc, "ddpm1d_host.inc")).read()
    for text, needle in ((k1, "dseed ^ 0x7f4a7c15u"), (k1, "dseed ^ 0x5bd1e995u"), (k1, "kKnown1dSeed = 0x6b6e6f776e316421ull"),
                         (k1, "0x80000000u + (uint32_t)l * 65536u + (uint32_t)t"), (k1, "0x10000u * (uint32_t)(a.relax_idx + 1)"),
                         (k1, "0xD2511F53u"), (k1, "0xCD9E8D57u"), (k1, "0x9E3779B9u"), (k1, "0xBB67AE85u"),
                         (k2, "seed ^ 0x9e3779b97f4a7c15ull"), (k2, "kKnown2dSeed = 0x6b6e6f776e326421ull"),
                         (host, "0x10000u * (uint32_t)(r + 1)")):
        assert needle in text, needle


def test_design_holds_the_ledger():
    """DESIGN 4.4 prints the table generated from the data above."""
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec = design.split("### 4.4 Counter-based noise", 1)[1].split("\n### ", 1)[0]
    assert N.ledger_markdown() in sec
