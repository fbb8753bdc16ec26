// Event-driven re-simulation of the n-body designs: the scene utils.py:1009-1033 of the reference builds -- equal,
// frictionless, perfectly elastic discs in a box, no gravity, no damping -- advanced in continuous time: between two frames (dt apart)
// the earliest wall or pair contact is found in closed form, every body is moved to it, the contact is resolved, and the search repeats.
// This is NOT Chipmunk's fixed-step impulse solver (which the reference runs through pymunk); it is the dynamics that solver discretises.
//
// One wavefront per design, four designs per workgroup; nothing is shared between wavefronts (no LDS, no barrier).
//   lanes 0 .. 7      own body `lane`'s state (x, y, vx, vy) in registers;
//   lanes 0 .. 15     evaluate the wall candidate of body lane / 2 on axis lane % 2 (the enumeration order: body-major, x before y);
//   lanes 16 .. 43    evaluate the pair candidate p = lane - 16, pairs (i, j), i < j, in lexicographic order;
// so a candidate's index in the enumeration order IS its lane number where the candidate exists.  The operands of a candidate come from
// the owner lanes by __shfl; the earliest candidate, ties to the lowest index, by a 64-lane __shfl_xor minimum over (t, lane), after
// which every lane holds the same (t, lane) and control flow is uniform over the wavefront.  All arithmetic is float64, every product,
// sum, quotient and square root rounded once (the library is built without contraction), in the order of tests/nbody_cases.py.
// Every loop is bounded: n_steps - 1 frames, at most max_events searches per frame.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace cindm {

struct NBodyArgs {
    const double* features;     // [B, nb, 4]
    double* out;                // [B, n_steps, nb, 4]
    int32_t* status;            // [B]
    int32_t* events;            // [B]
    int64_t B;
    double lox, hix, loy, hiy;  // where centres live
    double four_r2;             // (2 radius)^2
    double dt;
    int nb, n_steps, max_events;
};

constexpr int NBODY_NONE = 1 << 30;      // the index of "no candidate"

__global__ __launch_bounds__(256) void nbody_simulate_kernel(const NBodyArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= a.B) return;                                   // the whole wavefront leaves
    const int nb = a.nb, n_pairs = nb * (nb - 1) / 2;
    const bool owner = lane < nb;
    const bool wall = lane < 2 * nb, pair = lane >= 16 && lane < 16 + n_pairs;
    int ci = 0, cj = 0;                                      // the bodies this lane's candidate reads
    if (wall) ci = cj = lane >> 1;
    if (pair) {
        int r = lane - 16;
        while (r >= nb - 1 - ci) { r -= nb - 1 - ci; ++ci; }      // at most nb - 2 rounds
        cj = ci + 1 + r;
    }
    const int axis = lane & 1;
    double x = 0.0, y = 0.0, vx = 0.0, vy = 0.0;
    if (owner) {
        const double* f = a.features + (b * nb + lane) * 4;
        x = f[0]; y = f[1]; vx = f[2]; vy = f[3];
    }
    double* o = a.out + b * (int64_t)a.n_steps * nb * 4 + lane * 4;
    const int64_t frame_stride = (int64_t)nb * 4;

    const double inf = __builtin_huge_val();
    const bool finite = !owner || (fabs(x) < inf && fabs(y) < inf && fabs(vx) < inf && fabs(vy) < inf);      // false for NaN too
    if (!__all(finite)) {
        if (owner) {
            const double q = __builtin_nan("");
            for (int f = 0; f < a.n_steps; ++f, o += frame_stride) { o[0] = q; o[1] = q; o[2] = q; o[3] = q; }
        }
        if (lane == 0) { a.status[b] = 8; a.events[b] = 0; }
        return;
    }
    int st = 0, n_events = 0;
    {   // bit 1: a centre outside the box or a pair that overlaps at the start
        bool bad = owner && (x < a.lox || x > a.hix || y < a.loy || y > a.hiy);
        const double xi = __shfl(x, ci), yi = __shfl(y, ci), xj = __shfl(x, cj), yj = __shfl(y, cj);
        if (pair) {
            const double dx = xj - xi, dy = yj - yi;
            bad = dx * dx + dy * dy - a.four_r2 < 0.0;
        }
        if (__any(bad)) st |= 1;
    }

    for (int f = 0; f < a.n_steps; ++f, o += frame_stride) {
        if (owner) { o[0] = x; o[1] = y; o[2] = vx; o[3] = vy; }       // frame f is the state BEFORE stepping
        if (f == a.n_steps - 1) break;
        double rem = a.dt;
        for (int e = 0; ; ++e) {
            if (e == a.max_events) { st |= 2; break; }                  // the cap: the rest of the frame is ballistic
            const double xi = __shfl(x, ci), yi = __shfl(y, ci), vxi = __shfl(vx, ci), vyi = __shfl(vy, ci);
            const double xj = __shfl(x, cj), yj = __shfl(y, cj), vxj = __shfl(vx, cj), vyj = __shfl(vy, cj);
            double t = inf;
            bool valid = false;
            if (wall) {
                const double p = axis ? yi : xi, v = axis ? vyi : vxi;
                const double lo = axis ? a.loy : a.lox, hi = axis ? a.hiy : a.hix;
                if (v > 0.0) { t = (hi - p) / v; valid = true; }
                else if (v < 0.0) { t = (lo - p) / v; valid = true; }
                if (valid && t < 0.0) t = 0.0;                          // outside and outbound: reflects at once
            } else if (pair) {
                const double dx = xj - xi, dy = yj - yi, wx = vxj - vxi, wy = vyj - vyi;
                const double bq = dx * wx + dy * wy;
                if (bq < 0.0) {
                    const double c = dx * dx + dy * dy - a.four_r2;
                    if (c <= 0.0) { t = 0.0; valid = true; }            // overlapping and approaching: collides at once
                    else {
                        const double aq = wx * wx + wy * wy, disc = bq * bq - aq * c;
                        if (!(disc < 0.0)) { t = c / (-bq + sqrt(disc)); valid = true; }
                    }
                }
            }
            int idx = (valid && t == t) ? lane : NBODY_NONE;            // a NaN time is no candidate
            if (idx == NBODY_NONE) t = inf;
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) {
                const double ot = __shfl_xor(t, m);
                const int oi = __shfl_xor(idx, m);
                if (ot < t || (ot == t && oi < idx)) { t = ot; idx = oi; }
            }
            if (idx == NBODY_NONE || t > rem) break;
            if (owner) { x = x + vx * t; y = y + vy * t; }
            rem = rem - t;
            const int ei = __shfl(ci, idx), ej = __shfl(cj, idx);      // idx < 44: the winning lane
            if (idx < 16) {
                if (lane == ei) { if (idx & 1) vy = -vy; else vx = -vx; }
            } else {
                const double pxi = __shfl(x, ei), pyi = __shfl(y, ei), pvxi = __shfl(vx, ei), pvyi = __shfl(vy, ei);
                const double pxj = __shfl(x, ej), pyj = __shfl(y, ej), pvxj = __shfl(vx, ej), pvyj = __shfl(vy, ej);
                const double dx = pxj - pxi, dy = pyj - pyi, wx = pvxj - pvxi, wy = pvyj - pvyi;
                const double dd = dx * dx + dy * dy;
                if (dd == 0.0) { st |= 4; break; }                      // coincident centres: skipped, the frame ends ballistically
                const double k = (dx * wx + dy * wy) / dd;
                if (lane == ei) { vx = vx + k * dx; vy = vy + k * dy; }
                if (lane == ej) { vx = vx - k * dx; vy = vy - k * dy; }
            }
            ++n_events;
        }
        if (owner) { x = x + vx * rem; y = y + vy * rem; }
    }
    if (lane == 0) { a.status[b] = st; a.events[b] = n_events; }
}

}  // namespace cindm
