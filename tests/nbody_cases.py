"""Host statement of the n-body re-simulation rule, the case generator and the analytic cases.

Not a test module: tests/test_nbody_sim_host.py tests the statement itself, tests/test_gpu_nbody_sim.py holds the kernel to it.
The statement is written from the rule alone, in plain loops over Python floats (IEEE float64, every operation rounded once),
and shares no code with cindm_amd.

The rule.  Equal, frictionless, perfectly elastic discs of radius ``radius`` in a box whose walls have half-thickness
``wall_radius``: centres live in [lo, hi] = [radius + wall_radius, extent - radius - wall_radius] per axis.  Frame i is the state at
i * dt, recorded before stepping.  Inside a frame: rem = dt; enumerate candidates (walls first, body-major, x before y; then pairs
(i, j), i < j, lexicographic); take the earliest, ties to the first in that order; t > rem (or none): advance by rem, frame ends;
else advance by t, rem -= t, resolve, repeat -- at most ``max_events`` times, after which the frame ends ballistically.
A candidate whose time is NaN is no candidate."""
import math

import numpy as np

WIDTH = HEIGHT = 200.0
RADIUS = 20.0
WALL_RADIUS = 1.0
DT = 1.0 / 60.0
ULP = 2.0 ** -52


def simulate_one(feat, n_steps, width=WIDTH, height=HEIGHT, radius=RADIUS, wall_radius=WALL_RADIUS, dt=DT, max_events=64):
    """feat [nb, 4] -> (out [n_steps, nb, 4] float64, status, events, min_gap).  min_gap: the smallest difference between the two
    earliest candidate times at any resolved event (inf when no event had a second candidate)."""
    feat = np.asarray(feat, dtype=np.float64)
    nb = feat.shape[0]
    out = np.empty((n_steps, nb, 4), dtype=np.float64)
    if not np.isfinite(feat).all():
        out[:] = np.nan
        return out, 8, 0, math.inf
    x = [float(feat[i, 0]) for i in range(nb)]
    y = [float(feat[i, 1]) for i in range(nb)]
    vx = [float(feat[i, 2]) for i in range(nb)]
    vy = [float(feat[i, 3]) for i in range(nb)]
    lo = (radius + wall_radius, radius + wall_radius)
    hi = (width - radius - wall_radius, height - radius - wall_radius)
    four_r2 = 4.0 * radius * radius
    status, events, min_gap = 0, 0, math.inf
    for i in range(nb):
        if x[i] < lo[0] or x[i] > hi[0] or y[i] < lo[1] or y[i] > hi[1]:
            status |= 1
        for j in range(i + 1, nb):
            dx, dy = x[j] - x[i], y[j] - y[i]
            if dx * dx + dy * dy - four_r2 < 0.0:
                status |= 1
    for f in range(n_steps):
        for i in range(nb):
            out[f, i, 0], out[f, i, 1], out[f, i, 2], out[f, i, 3] = x[i], y[i], vx[i], vy[i]
        if f == n_steps - 1:
            break
        rem = dt
        n_frame = 0
        while True:
            if n_frame == max_events:
                status |= 2
                break
            best_t, best, second = math.inf, None, math.inf
            # candidates in the fixed order; a strict "<" keeps the first of equal times
            cands = []
            for i in range(nb):
                for a in range(2):
                    p, v = (x[i], vx[i]) if a == 0 else (y[i], vy[i])
                    if v > 0.0:
                        t = (hi[a] - p) / v
                    elif v < 0.0:
                        t = (lo[a] - p) / v
                    else:
                        continue
                    if t < 0.0:
                        t = 0.0
                    cands.append((t, ("wall", i, a)))
            for i in range(nb):
                for j in range(i + 1, nb):
                    dx, dy = x[j] - x[i], y[j] - y[i]
                    wx, wy = vx[j] - vx[i], vy[j] - vy[i]
                    b = dx * wx + dy * wy
                    if not b < 0.0:
                        continue
                    c = dx * dx + dy * dy - four_r2
                    if c <= 0.0:
                        t = 0.0
                    else:
                        aq = wx * wx + wy * wy
                        disc = b * b - aq * c
                        if disc < 0.0:
                            continue
                        t = c / (-b + math.sqrt(disc))
                    cands.append((t, ("pair", i, j)))
            for t, what in cands:
                if t != t:
                    continue
                if best is None or t < best_t:
                    if best is not None:
                        second = best_t
                    best_t, best = t, what
                elif t < second:
                    second = t
            if best is None or best_t > rem:
                break
            t = best_t
            for i in range(nb):
                x[i] = x[i] + vx[i] * t
                y[i] = y[i] + vy[i] * t
            rem = rem - t
            if best[0] == "wall":
                _, i, a = best
                if a == 0:
                    vx[i] = -vx[i]
                else:
                    vy[i] = -vy[i]
            else:
                _, i, j = best
                dx, dy = x[j] - x[i], y[j] - y[i]
                wx, wy = vx[j] - vx[i], vy[j] - vy[i]
                dd = dx * dx + dy * dy
                if dd == 0.0:
                    status |= 4
                    break
                k = (dx * wx + dy * wy) / dd
                vx[i] = vx[i] + k * dx
                vy[i] = vy[i] + k * dy
                vx[j] = vx[j] - k * dx
                vy[j] = vy[j] - k * dy
            min_gap = min(min_gap, second - best_t)
            events += 1
            n_frame += 1
        for i in range(nb):
            x[i] = x[i] + vx[i] * rem
            y[i] = y[i] + vy[i] * rem
    return out, status, events, min_gap


def simulate(features, n_steps, **kw):
    """features [B, nb, 4] -> (out [B, n_steps, nb, 4], status [B] int32, events [B] int32, min_gap [B])."""
    features = np.asarray(features, dtype=np.float64)
    res = [simulate_one(f, n_steps, **kw) for f in features]
    return (np.stack([r[0] for r in res]), np.array([r[1] for r in res], dtype=np.int32),
            np.array([r[2] for r in res], dtype=np.int32), np.array([r[3] for r in res], dtype=np.float64))


_SIGNS = (lambda n: np.ones(n), lambda n: -np.ones(n), lambda n: np.where(np.arange(n) % 2 == 0, 1.0, -1.0),
          lambda n: np.where(np.arange(n) % 2 == 0, -1.0, 1.0))


def sensitivity(feat, n_steps, base=None, **kw):
    """s_case: the statement's own largest deviation under a relative perturbation of +-2^-52 of every input, maximised over four
    sign patterns (all +, all -, alternating from +, alternating from -)."""
    feat = np.asarray(feat, dtype=np.float64)
    if base is None:
        base = simulate_one(feat, n_steps, **kw)[0]
    s = 0.0
    for sg in _SIGNS:
        pert = feat * (1.0 + ULP * sg(feat.size).reshape(feat.shape))
        s = max(s, float(np.abs(simulate_one(pert, n_steps, **kw)[0] - base).max()))
    return s


def generate(rng, nb, n_cases, width=WIDTH, height=HEIGHT, radius=RADIUS, wall_radius=WALL_RADIUS):
    """n_cases placements of nb bodies: positions uniform in [lo, hi]^2, the whole placement redrawn until every pair is at least
    2 radius + 0.5 apart; velocities U(-100, 100) (the range of the reference's data/nbody_simulation.py:62-63); cast to fp32."""
    lo = radius + wall_radius
    hx, hy = width - radius - wall_radius, height - radius - wall_radius
    out = np.empty((n_cases, nb, 4), dtype=np.float32)
    for c in range(n_cases):
        while True:
            pos = np.stack([rng.uniform(lo, hx, nb), rng.uniform(lo, hy, nb)], 1)
            d = np.sqrt(((pos[:, None, :] - pos[None, :, :]) ** 2).sum(-1)) + np.eye(nb) * 1e9
            if d.min() >= 2 * radius + 0.5:
                break
        vel = rng.uniform(-100.0, 100.0, (nb, 2))
        out[c] = np.concatenate([pos, vel], 1).astype(np.float32)
    return out          # lo and hi are fp32 numbers and rounding is monotonic: the cast leaves every centre inside [lo, hi]


_GEN_CACHE = {}


def generator_cases(nb, n_cases, seed=0):
    """One stream per (seed, body count): the same cases wherever they are asked for (read-only)."""
    key = (seed, nb, n_cases)
    if key not in _GEN_CACHE:
        a = generate(np.random.default_rng([seed, nb]), nb, n_cases)
        a.setflags(write=False)
        _GEN_CACHE[key] = a
    return _GEN_CACHE[key]


# ---- analytic cases ---------------------------------------------------------------------------------------------------------------
LO, HI = RADIUS + WALL_RADIUS, WIDTH - RADIUS - WALL_RADIUS       # 21, 179


def triangle_wave(p0, v, t, lo=LO, hi=HI):
    """Position and velocity at time t of a point bouncing between lo and hi, from p0 with velocity v (float64 closed form)."""
    span = hi - lo
    s = (p0 - lo + v * t) % (2.0 * span)
    if s <= span:
        return lo + s, v
    return hi - (s - span), -v


def wall_case(speed):
    """One body, both axes moving: (features [1, 1, 4], closed form f(frame) -> (x, y, vx, vy))."""
    feat = np.array([[[60.0, 130.0, speed, -0.3 * speed]]])

    def closed(i):
        t = i * DT
        x, vx = triangle_wave(60.0, speed, t)
        y, vy = triangle_wave(130.0, -0.3 * speed, t)
        return np.array([x, y, vx, vy])
    return feat, closed


def head_on_case():
    """Two bodies on y = 100 approaching at 60 and -40 px/s with 61 px between their rims: contact after gap / closing speed
    (0.61 s = 36.6 frames: no frame falls on the contact)."""
    feat = np.array([[[50.0, 100.0, 60.0, 0.0], [151.0, 100.0, -40.0, 0.0]]])
    t_c = (101.0 - 2 * RADIUS) / 100.0
    return feat, t_c


def glancing_case():
    """Body 0 moves along +x at 80 px/s towards a resting body 1 offset by 2 radius sin(30 deg) in y: the contact normal makes 30 degrees
    with x, body 1 leaves along the normal with 80 cos 30, body 0 along the tangent with 80 sin 30."""
    off = 2 * RADIUS * 0.5
    feat = np.array([[[40.0, 100.0, 80.0, 0.0], [120.0, 100.0 + off, 0.0, 0.0]]])
    nx, ny = math.cos(math.radians(30.0)), math.sin(math.radians(30.0))
    vn = 80.0 * nx
    v1 = np.array([vn * nx, vn * ny])
    v0 = np.array([80.0, 0.0]) - v1
    t_c = (80.0 - 2 * RADIUS * nx) / 80.0
    return feat, t_c, v0, v1


def line_case():
    """Three bodies on y = 100, 0 moving at 90 px/s, 1 and 2 at rest: the velocity is handed 0 -> 1 -> 2 (contacts at 10.67 and
    22.67 frames)."""
    feat = np.array([[[30.0, 100.0, 90.0, 0.0], [86.0, 100.0, 0.0, 0.0], [144.0, 100.0, 0.0, 0.0]]])
    t1 = (56.0 - 2 * RADIUS) / 90.0
    t2 = t1 + (58.0 - 2 * RADIUS) / 90.0
    return feat, t1, t2


def edge_cases():
    """name -> features [1, nb, 4] of the defined edge behaviour."""
    return {
        "overlap_approaching": np.array([[[80.0, 100.0, 30.0, 0.0], [110.0, 100.0, -30.0, 0.0]]]),
        "overlap_separating": np.array([[[80.0, 100.0, -30.0, 0.0], [110.0, 100.0, 30.0, 0.0]]]),
        "outside_outbound": np.array([[[185.0, 100.0, 50.0, 0.0]]]),
        "fast": np.array([[[60.0, 130.0, 20000.0, -6000.0]]]),
        # approaching centres 1e-170 px apart (at the origin, where such a difference exists): d.w < 0 but d.d underflows to 0, the
        # one way to a pair event with d.d == 0; both move into the box, so no wall event comes first
        "coincident": np.array([[[0.0, 0.0, 20.0, 5.0], [1e-170, 0.0, 10.0, 5.0]]]),
    }
