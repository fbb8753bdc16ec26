// cindm_nbody_simulate (include/cindm_hip.h): argument checks and the one launch of nbody_simulate_kernel (nbody.h).  No handle, no
// allocation, no synchronisation: the call is ordered on the caller's stream like any kernel launch.

extern "C" int cindm_nbody_simulate(const cindm_nbody_desc* d, const double* features, int64_t B, int32_t n_bodies, int32_t n_steps,
                                    double* out, int32_t* status, int32_t* events, void* stream) {
    REQUIRE(d && features && out && status && events, "cindm_nbody_simulate: null argument");
    REQUIRE(n_bodies >= 1 && n_bodies <= 8, "cindm_nbody_simulate: n_bodies must be in 1 .. 8");
    REQUIRE(n_steps >= 1 && n_steps <= 65535, "cindm_nbody_simulate: n_steps must be in 1 .. 65535");
    REQUIRE(B >= 1 && B <= ((int64_t)1 << 22), "cindm_nbody_simulate: B must be in 1 .. 2^22");
    NBodyArgs a;
    a.lox = d->radius + d->wall_radius; a.hix = d->width - d->radius - d->wall_radius;
    a.loy = a.lox;                      a.hiy = d->height - d->radius - d->wall_radius;
    REQUIRE(d->radius > 0.0 && d->wall_radius >= 0.0, "cindm_nbody_simulate: radius must be positive and wall_radius non-negative");
    REQUIRE(a.hix > a.lox && a.hiy > a.loy && std::isfinite(a.hix) && std::isfinite(a.hiy),
            "cindm_nbody_simulate: the box leaves no room for a centre (need width, height > 2 (radius + wall_radius))");
    REQUIRE(d->dt > 0.0 && std::isfinite(d->dt), "cindm_nbody_simulate: dt must be positive and finite");
    REQUIRE(d->max_events_per_frame >= 1 && d->max_events_per_frame <= 4096, "cindm_nbody_simulate: max_events_per_frame must be in 1 .. 4096");
    a.features = features; a.out = out; a.status = status; a.events = events; a.B = B;
    a.four_r2 = 4.0 * d->radius * d->radius;
    a.dt = d->dt;
    a.nb = n_bodies; a.n_steps = n_steps; a.max_events = d->max_events_per_frame;
    hipLaunchKernelGGL(nbody_simulate_kernel, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, (hipStream_t)stream, a);
    HIPCHK(hipGetLastError());
    return 0;
}
