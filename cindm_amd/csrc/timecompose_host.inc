// ---- GaussianDiffusion1D: parallel time composition, the seventh 1-D sampling chain ------------------------------------------------------
// Textually included by cindm_hip.hip right after ddpm1d_host.inc, whose Chain1D, chain1_refuse, chain_io, ddim_tables1, loop_steps
// and run_chain_with_recovery it runs on; run_step launches timecompose_update_kernel in place of compose_update_kernel when the
// StepIO carries `tc` (DESIGN 4.5p).
//
// composing_time_sample (model/diffusion_1d.py:1807-1854): ONE unguided DDIM chain on n_seg * B rows, segment-major.  The chain's
// Chain1D is laid out for n_seg * B rows and its condition is cond_buf [n_seg * B, Lc, F]: rows 0 .. B hold the caller's cond, row
// (k + 1, b) the last Lc rows of row (k, b)'s current state, written by the update that produced them (and by the init kernel from
// x_T).  Like the rollout the body draws every x_T itself, so it is a pure function of its inputs and a time-out re-runs all of it
// once on the exchange-free kernels.  The segment seeds live in the workspace's second state buffer (the guided chains' staging
// slice, unused by an unguided chain): the captured update reads them from there, so one graph serves every seed.
extern "C" int cindm_ddpm1d_sample_timecompose(cindm_ddpm1d* h, cindm_unet1d* pair, cindm_unet1d* uncond, const cindm_compose_desc* c,
                                               float* x, const float* cond, float* cond_buf, int32_t n_seg, int32_t n_steps,
                                               const int32_t* times, const float* coefs, const uint64_t* seeds, const float* init_tape,
                                               const float* noise_steps, int64_t sample_offset, int64_t B, void* ws, size_t ws_bytes,
                                               void* stream_, int32_t use_graph) {
    ChainArmed took(h);
    REQUIRE(n_seg >= 2 && B >= 1 && (int64_t)n_seg * B <= 65535, "n_seg must be >= 2 and n_seg * B <= 65535 (the update derives a row's segment by a 32-bit multiply)");
    Chain1D ch(h, pair, uncond, c, (int64_t)n_seg * B, ws, ws_bytes, nullptr, use_graph);
    const Ddim1Call dd{n_steps, times, coefs};
    if (took.refuse_all_but(0, "the parallel time composition hands rows of one segment's state over to the next one's condition at every "
                               "step: a region of one [B, rows, F] state does not name a place in its n_seg * B rows") != 0) return -1;
    REQUIRE(h && pair && c && x && cond && cond_buf && times && coefs && seeds, "null argument");
    REQUIRE(c->mode == CINDM_COMPOSE_PLAIN || c->mode == CINDM_COMPOSE_MULTIBODY, "the time composition runs the plain (or multibody) prediction");
    REQUIRE(c->cond_steps >= 1, "conditioned_steps == 0: the reference's img_infered[:, -0:] hands over the whole state and its slice assignment fails");
    const int R = state_len(pair, c), Lc = c->cond_steps, F = c->n_bodies * 4;
    REQUIRE(R >= Lc, "image_size < conditioned_steps: the next segment's condition would be shorter than the model's horizon needs");
    for (const void* p : {(const void*)x, (const void*)cond, (const void*)cond_buf, (const void*)init_tape, (const void*)noise_steps})
        REQUIRE(((uintptr_t)p & 15) == 0, "x, cond, cond_buf, init_tape and noise_steps must be 16-byte aligned");
    if (chain1_refuse(ch, x, cond_buf, &dd) != 0) return -1;
    if (took.rec.on()) REQUIRE(n_steps >= 1, "n_steps must be >= 1");
    if (rec_begin(took, x, n_steps, ch.n_state()) != 0) return -1;
    if (chain_stream(h, stream_, use_graph, &ch.stream) != 0) return -1;
    const int64_t n_state = ch.n_state();
    hipStream_t stream = ch.stream;
    // (no inpainting; the chain's (seed, sample_offset) words carry the offset, the seed per segment comes from the table below)
    StepIO io = chain_io(ch, x, cond_buf, noise_steps, seeds[0], sample_offset, nullptr, 0, nullptr);
    if (ddim_tables1(ch, dd, io) != 0) return -1;
    unsigned long long* seeds_dev = ch.at<unsigned long long>(ch.s.off_tmp);      // n_state * 4 bytes >= n_seg * 16
    HIPCHK(hipMemcpyAsync(seeds_dev, seeds, (size_t)n_seg * sizeof(uint64_t), hipMemcpyHostToDevice, stream));
    HIPCHK(hipStreamSynchronize(stream));            // the caller's host array may go out of scope
    TimeComposeArgs tc;
    std::memset(&tc, 0, sizeof(tc));
    tc.cond_buf = cond_buf; tc.seeds = seeds_dev; tc.Bseg = B; tc.n_seg = n_seg;
    tc.seg_magic = ((1ull << 32) + (unsigned long long)B - 1) / (unsigned long long)B;
    io.tc = &tc;
    const unsigned iblocks = (unsigned)((n_state / 4 + 255) / 256);
    return rec_done(took, run_chain_with_recovery(ch, x, [&]() -> int {
        if (prepare_step_ws(ch) != 0) return -1;
        hipLaunchKernelGGL(timecompose_init_kernel, dim3(iblocks), dim3(256), 0, stream, x, cond_buf, cond, init_tape,
                           (const unsigned long long*)seeds_dev, B, tc.seg_magic, (int)n_seg, R, F, Lc, sample_offset, (uint32_t)h->T);
        HIPCHK(hipGetLastError());
        return loop_steps(ch, io, 5, (int)times[0], n_steps, seeds[0], sample_offset);
    }));
}
