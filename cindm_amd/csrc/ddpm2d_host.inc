// ---- GaussianDiffusion (2-D): the reverse step and the four sampling chains ------------------------------------------------------------
// Textually included by cindm_hip.hip after forceunet_host.inc (the guided chains call the surrogate's cindm_airfoil_design_grad).
// Each fact is stated once:
//   ddpm2d_layout              the diffusion workspace, [eps | U-Net workspace | x_T snapshot]
//   Chain2D                    what every helper below is handed unchanged, and the slices of that workspace
//   run_step2, run_ddim_step2  one DDPM / DDIM step: forward, update, counter
//   step2_refuse               what a step refuses of its Chain2D and state
//   chain2_refuse, force_refuse   what a chain entry refuses, on top of that, before it touches the device
//   ForceGuide                 the airfoil objective of a guided chain and its one cindm_airfoil_design_grad call
//   ddim_args2                 the Ddim2dArgs of a DDIM chain
//   known2_begin, known2_node  the known region of a chain (cindm_ddpm1d_set_known2d): its check against the state, and its launch
//   ddpm_step2, ddim_step2     the captured step: [gradient,] step, [shift,] [known node,] [record node]
//   run_chain2                 the tail: counter, rec_arm, [known node: rule 1,] replay -- under force_chain_with_recovery when guided -- and rec_done
//   ms_begin2, ms_tables2      the multistep solver of a DDIM chain (cindm_ddpm1d_set_multistep): its checks, and kappa behind the caller's tables
// An entry is: ChainArmed (everything armed on the handle, chain_host.inc), refuse_all_but what it serves, its other refusals, (DDIM: ms_begin2,)
// rec_begin2, known2_begin, chain_stream,
// (DDIM: upload_ddim_tables, ms_tables2,) build the step, run_chain2.

// Returns the bytes of a diffusion workspace for `images` images; the offsets of its second and third slice go to *o_unet / *o_xT.
// The x_T snapshot serves the guided chains' recovery (force_chain_with_recovery): no allocation after *_create.
static size_t ddpm2d_layout(const cindm_unet2d* u, int64_t images, size_t* o_unet = nullptr, size_t* o_xT = nullptr) {
    auto al = [](size_t v) { return (v + 255) / 256 * 256; };
    const size_t st = al((size_t)images * u->d.image_size * u->d.image_size * u->CP() * sizeof(float));
    const size_t uw = al(cindm_unet2d_workspace_bytes(u, images));
    if (o_unet) *o_unet = st;
    if (o_xT) *o_xT = st + uw;
    return 2 * st + uw + 256;
}
extern "C" size_t cindm_ddpm2d_workspace_bytes(const cindm_unet2d* u, int64_t images) { return u ? ddpm2d_layout(u, images) : 0; }

// What the 2-D steps and chains hand unchanged to every helper below them.  share: the use_average_share word.
struct Chain2D {
    cindm_ddpm1d* s; cindm_unet2d* u; int64_t B; int nb; int share; void* ws; size_t ws_bytes; hipStream_t stream; int use_graph;
    size_t need = 0, o_unet = 0, o_xT = 0;      // ddpm2d_layout of B * nb images (0 while u or the batch is refused anyway)
    Chain2D(cindm_ddpm1d* s_, cindm_unet2d* u_, int64_t B_, int nb_, int share_, void* ws_, size_t ws_bytes_, hipStream_t stream_, int use_graph_)
        : s(s_), u(u_), B(B_), nb(nb_), share(share_), ws(ws_), ws_bytes(ws_bytes_), stream(stream_), use_graph(use_graph_) {
        if (u && B > 0 && nb >= 1) need = ddpm2d_layout(u, NI(), &o_unet, &o_xT);
    }
    int64_t NI() const { return B * nb; }                                   // images
    int HW() const { return u->d.image_size * u->d.image_size; }
    int CP() const { return u->CP(); }
    int64_t state_floats() const { return NI() * (int64_t)HW() * CP(); }      // floats of the state x, [B * nb][H * W][padded channels]
    float* eps() const { return (float*)ws; }
    void* unet_ws() const { return (char*)ws + o_unet; }
    size_t unet_ws_bytes() const { return ws_bytes - o_unet; }
    float* xT() const { return reinterpret_cast<float*>((char*)ws + o_xT); }
    unsigned update_blocks() const { return (unsigned)((B * (int64_t)HW() * (CP() / 4) + 255) / 256); }      // one thread per float4 of a design
};

// per-step tapes (or counter noise keyed by seed and offset) of a chain
struct Draws2 { const float* state_steps; const float* boundary_steps; uint64_t seed; int64_t sample_offset; };

struct Step2IO {
    const float* x; float* x_out; float* x0_out; float* mean_out;
    float* eps_out = nullptr; int predict = 0, rederive = 0;      // cindm_ddpm2d_predict
    const float* noise_state; int64_t ns_stride; const float* noise_bound; int64_t nb_stride;
    uint64_t seed; int64_t off; int add_noise; int dec_t;
};

// What a step refuses of its Chain2D and state: run_step2's own checks (cindm_ddpm2d_step and _predict reach it directly), which the
// chain entries make up front (chain2_refuse).
static int step2_refuse(const Chain2D& ch, const float* x) {
    // the share word: bit 0 = mean (1) / sum (0) over the boundary copies, bit 1 = share_noise False, bits 4-5 = objective (0 pred_noise,
    // 1 pred_x0, 2 pred_v).  Anything else is a caller error, not a silent x_start of 0 (objective 3) or a silent "sum" (2 for "true")
    REQUIRE(((ch.share >> 4) & 3) <= 2 && (ch.share & ~0x33) == 0, "bad use_average_share word (bit 0 mean / sum, bit 1 share_noise off, bits 4-5 objective 0..2)");
    REQUIRE(ch.s && ch.u && x && ch.ws, "null argument");
    REQUIRE(ch.B > 0 && ch.nb >= 1, "bad batch");
    REQUIRE(ch.s->T <= ch.u->d.timesteps, "the diffusion has more timesteps than the Unet's per-timestep table (construct Unet(..., timesteps=T))");
    REQUIRE(ch.state_floats() < (1ll << 31), "state too large for one launch");
    REQUIRE(ch.ws_bytes >= ch.need, "workspace too small");
    return 0;
}

static int run_step2(const Chain2D& ch, const Step2IO& io, int clip, int32_t t, const int32_t* t_dev) {
    cindm_ddpm1d* s = ch.s; cindm_unet2d* u = ch.u;
    if (step2_refuse(ch, io.x) != 0) return -1;
    REQUIRE(t_dev || (t >= 0 && t < s->T), "timestep out of range");
    if (cindm_unet2d_forward(u, io.x, t, t_dev, ch.eps(), ch.NI(), ch.unet_ws(), ch.unet_ws_bytes(), ch.stream) != 0) return -1;
    Update2dArgs a; std::memset(&a, 0, sizeof(a));
    a.x = io.x; a.eps = ch.eps(); a.x_out = io.x_out; a.x0_out = io.x0_out; a.mean_out = io.mean_out;
    a.eps_out = io.eps_out; a.predict = io.predict; a.rederive = io.rederive;
    a.B = (int)ch.B; a.nb = ch.nb; a.HW = ch.HW(); a.C = u->d.channels; a.CP = ch.CP(); a.use_avg = ch.share; a.clip = clip; a.add_noise = io.add_noise;
    const float* tb = s->tab; const size_t T = s->T;
    a.sqrt_recip = tb + 6 * T; a.sqrt_recipm1 = tb + 7 * T; a.logvar = tb + 9 * T; a.coef1 = tb + 10 * T; a.coef2 = tb + 11 * T;
    a.sqrt_ac = tb + 3 * T; a.sqrt_1mac = tb + 4 * T;
    a.t_ptr = t_dev; a.t_imm = t;
    a.noise_state = io.noise_state; a.ns_t_stride = io.ns_stride; a.noise_bound = io.noise_bound; a.nb_t_stride = io.nb_stride;
    a.seed = io.seed; a.sample_off = io.off;
    hipLaunchKernelGGL(update2d_kernel, dim3(ch.update_blocks()), dim3(256), 0, ch.stream, a);
    if (io.dec_t) hipLaunchKernelGGL(step_counter_kernel, dim3(1), dim3(64), 0, ch.stream, s->t_dev, (const int*)nullptr, (int*)nullptr, (int*)nullptr);
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int cindm_ddpm2d_step(cindm_ddpm1d* s, cindm_unet2d* u, float* x, int64_t B, int32_t nb, int32_t use_average_share,
                                 int32_t clip_denoised, const float* noise_state, const float* noise_boundary, uint64_t seed,
                                 int64_t sample_offset, int32_t t, const int32_t* t_dev, float* x0_out, float* mean_out,
                                 void* ws, size_t ws_bytes, void* stream) {
    Step2IO io{};
    io.x = x; io.x_out = x; io.x0_out = x0_out; io.mean_out = mean_out;
    io.noise_state = noise_state; io.noise_bound = noise_boundary; io.ns_stride = 0; io.nb_stride = 0;
    io.seed = seed; io.off = sample_offset; io.add_noise = 1;
    return run_step2(Chain2D(s, u, B, nb, use_average_share, ws, ws_bytes, (hipStream_t)stream, 0), io, clip_denoised, t, t_dev);
}

// model_predictions (:727-754): the U-Net and the boundary sharing of its output, x_start, optional clamp / re-derived noise
extern "C" int cindm_ddpm2d_predict(cindm_ddpm1d* s, cindm_unet2d* u, const float* x, int64_t B, int32_t nb, int32_t use_average_share,
                                    int32_t share_noise, int32_t clip_x_start, int32_t rederive_pred_noise, int32_t t,
                                    const int32_t* t_dev, float* pred_noise_out, float* x_start_out, void* ws, size_t ws_bytes,
                                    void* stream) {
    Step2IO io{};
    io.x = x; io.x_out = nullptr; io.x0_out = x_start_out; io.mean_out = nullptr;
    io.eps_out = pred_noise_out; io.predict = 1; io.rederive = (clip_x_start && rederive_pred_noise) ? 1 : 0;
    io.add_noise = 0;
    const int share = ((use_average_share & ~0x30) ? 1 : 0) | (share_noise ? 0 : 2) | (use_average_share & 0x30);
    return run_step2(Chain2D(s, u, B, nb, share, ws, ws_bytes, (hipStream_t)stream, 0), io, clip_x_start, t, t_dev);
}

// ---- the chains --------------------------------------------------------------------------------------------------------------------------
// What a DDIM entry is handed on top of a DDPM one.  weights: the guided chain's per-step guidance weights (else null).
struct Ddim2dCall { int32_t n_steps; const int32_t* times; const float* coefs; const float* weights; void* tab; size_t tab_bytes; };

// What every chain entry refuses before it touches the device: step2_refuse and the DDPM range t_start .. t_end or, for a DDIM chain
// (dd), its share word and table buffer (n_steps < 1 and the schedule itself are refused by upload_ddim_tables, before anything is copied).
static int chain2_refuse(const Chain2D& ch, const float* x, const Ddim2dCall* dd, int t_start = 0, int t_end = 0) {
    if (dd) {
        REQUIRE(dd->times && dd->coefs && dd->tab, "null argument");
        REQUIRE(((ch.share >> 4) & 3) <= 2 && (ch.share & ~0x31) == 0,
                "bad use_average_share word (bit 0 mean / sum, bits 4-5 objective 0..2; DDIM has no share_noise False)");
        REQUIRE(dd->tab_bytes >= (size_t)std::max(dd->n_steps, 0) * 5 * sizeof(float) && ((uintptr_t)dd->tab & 15) == 0, "DDIM table buffer too small or not 16-byte aligned");
    }
    if (step2_refuse(ch, x) != 0) return -1;
    if (!dd) REQUIRE(t_start < ch.s->T && t_end >= 0 && t_end <= t_start, "bad timestep range");
    return 0;
}

// The airfoil objective of a guided chain: g = d(force + overlap)/dx at the chain's x, into `grad` (cindm_airfoil_design_grad).
struct ForceGuide {
    cindm_forceunet* f; int frames; float p_min, p_max, lambda_force, lambda_overlap; int down_factor, sum_boundary;
    float* grad; void* ws_force; size_t ws_force_bytes;
    int gradient(const Chain2D& ch, const float* x) const {
        return cindm_airfoil_design_grad(f, x, ch.B, ch.nb, frames, ch.CP(), p_min, p_max, lambda_force, lambda_overlap, down_factor, sum_boundary,
                                         grad, ws_force, ws_force_bytes, ch.stream);
    }
};

// What a guided entry refuses on top of chain2_refuse (after it).  per_step: the entry's own table, eta (DDPM) or weights (DDIM).
static int force_refuse(const Chain2D& ch, const ForceGuide& g, const float* x, const float* per_step) {
    REQUIRE(g.f && per_step && g.grad && g.ws_force, "null argument");
    REQUIRE(g.f->finalized, "cindm_forceunet_finalize has not been called");
    REQUIRE(ch.u->d.image_size == g.f->d.image_size, "Unet and ForceUnet image sizes differ");
    REQUIRE(g.frames >= 1 && ch.u->d.channels == 3 * g.frames + 3, "state channels must be 3 * frames + 3");
    REQUIRE(g.f->d.channels == 4, "the airfoil objective feeds (pressure, 3 boundary channels): ForceUnet(channels=4)");
    REQUIRE(g.down_factor >= 1 && ch.u->d.image_size % g.down_factor == 0, "downsampling_factor must divide the image size");
    REQUIRE((((uintptr_t)x | (uintptr_t)g.grad | (uintptr_t)ch.ws) & 15) == 0, "x, grad and ws must be 16-byte aligned");
    REQUIRE(((uintptr_t)g.ws_force & 255) == 0 && g.ws_force_bytes >= cindm_airfoil_design_workspace_bytes(g.f, ch.B, ch.nb, 1),
            "surrogate workspace too small (cindm_airfoil_design_workspace_bytes) or not 256-byte aligned");
    return 0;
}

// why a 2-D entry refuses an armed 1-D known region
static const char* const kKnown1Not2D = "it belongs to the 1-D chains (cindm_ddpm1d_sample / _sample_guided / _sample_ddim / _sample_ddim_guided); the 2-D chains take theirs from cindm_ddpm1d_set_known2d";

// the recorder of a 2-D chain: one record is the whole state in the library's layout, [B * nb][H * W][padded channels]
static const char* const kNoX0Ddim2d = "recorder: the 2-D DDIM update kernels have no x0 operand: the x0 stream is served by the DDPM entries only";
static int rec_begin2(ChainArmed& took, const Chain2D& ch, const float* x, int n_steps, const char* x0_refusal = nullptr) {
    return took.rec.on() ? rec_begin(took, x, n_steps, ch.state_floats(), x0_refusal) : 0;
}

// The known region of a 2-D chain (DESIGN 4.5n): checked against the chain's state before the entry's first launch or copy, then held
// by the handle for the whole call.  The draws are the chain's own (seed, sample_offset), under known2d_kernel's seed word.
static int known2_begin(ChainArmed& took, const Chain2D& ch, const float* x, const Draws2& z) {
    if (!took.kn.on()) return 0;
    Known2D& k = took.kn;
    if (k.images != ch.NI() || k.hw != ch.HW() || k.cp != ch.CP())
        return fail("known region: made for " + std::to_string(k.images) + " images of " + std::to_string(k.hw) + " pixels x " + std::to_string(k.cp) +
                    " padded channels, the chain runs " + std::to_string(ch.NI()) + " x " + std::to_string(ch.HW()) + " x " + std::to_string(ch.CP()));
    if (((uintptr_t)x & 15) != 0) return fail("known region: the state x must be 16-byte aligned (the node moves 16 bytes per lane)");
    if (k.z_state && (k.zs_stride < ch.B * (int64_t)ch.HW() * (ch.u->d.channels - 3) || k.zb_stride < ch.NI() * (int64_t)ch.HW() * 3))
        return fail("known region: a tape stride is smaller than one row ([B, H*W, C-3] state floats, [B*nb, H*W, 3] boundary floats)");
    k.seed = z.seed; k.sample_off = z.sample_offset;
    took.h->kn = &took.kn;
    return 0;
}

// the known node: init = 1 is rule 1 (the chain body's, at the first timestep), init = 0 the step's (after its counter launch)
static int known2_node(const Chain2D& ch, float* x, int init) {
    const Known2D& k = *ch.s->kn;
    Known2dArgs a; std::memset(&a, 0, sizeof(a));
    a.x = x; a.known = k.known; a.mask = k.mask;
    a.B = (int)ch.B; a.nb = ch.nb; a.HW = ch.HW(); a.C = ch.u->d.channels; a.CP = ch.CP();
    a.sqrt_ac = ch.s->tab + 3 * (size_t)ch.s->T; a.sqrt_1mac = ch.s->tab + 4 * (size_t)ch.s->T;
    a.t_dev = ch.s->t_dev; a.tnext = k.tnext; a.init = init; a.init_tag = (uint32_t)ch.s->T;
    a.zi_state = k.zi_state; a.zi_bound = k.zi_bound; a.z_state = k.z_state; a.zs_stride = k.zs_stride; a.z_bound = k.z_bound; a.zb_stride = k.zb_stride;
    a.seed = k.seed; a.sample_off = k.sample_off;
    hipLaunchKernelGGL(known2d_kernel, dim3(ch.update_blocks()), dim3(256), 0, ch.stream, a);
    HIPCHK(hipGetLastError());
    return 0;
}

// the Step2IO of a 2-D sample loop: in-place state, per-step tapes (or counter noise), the device counter decremented by the step
static Step2IO chain_io2(const Chain2D& ch, float* x, const Draws2& z) {
    Step2IO io{};
    io.x = x; io.x_out = x;
    if (ch.s->rec) io.x0_out = ch.s->rec->x0_stage;
    io.noise_state = z.state_steps; io.ns_stride = ch.B * (int64_t)ch.HW() * (ch.u->d.channels - 3);
    io.noise_bound = z.boundary_steps; io.nb_stride = ch.NI() * (int64_t)ch.HW() * 3;
    io.seed = z.seed; io.off = z.sample_offset; io.add_noise = 1; io.dec_t = 1;
    return io;
}

// the Ddim2dArgs of a DDIM chain: in-place state, the schedule's tables, the per-step tables uploaded to the caller's buffer, the draws
static Ddim2dArgs ddim_args2(const Chain2D& ch, float* x, const Ddim2dCall& dd, const int* tn_dev, const Draws2& z) {
    Ddim2dArgs a; std::memset(&a, 0, sizeof(a));
    a.x = x; a.x_out = x; a.eps = ch.eps();
    a.B = (int)ch.B; a.nb = ch.nb; a.HW = ch.HW(); a.C = ch.u->d.channels; a.CP = ch.CP(); a.use_avg = ch.share;
    const float* tb = ch.s->tab; const size_t T = ch.s->T;
    a.sqrt_recip = tb + 6 * T; a.sqrt_recipm1 = tb + 7 * T; a.sqrt_ac = tb + 3 * T; a.sqrt_1mac = tb + 4 * T;
    a.t_dev = ch.s->t_dev; a.tab = (const float*)dd.tab; a.tnext = tn_dev;
    a.noise_state = z.state_steps; a.ns_t_stride = ch.B * (int64_t)ch.HW() * (ch.u->d.channels - 3);
    a.noise_bound = z.boundary_steps; a.nb_t_stride = ch.NI() * (int64_t)ch.HW() * 3;
    a.seed = z.seed; a.sample_off = z.sample_offset;
    return a;
}

// The multistep solver of a 2-D DDIM chain: the fourth word of a table row carries the guidance weight here, so kappa is a table of
// its own behind the rows and the next-times (a sixth word per step of the caller's buffer).  *kappa_dev stays null without it.
static int ms_tables2(const Chain2D& ch, const Ddim2dCall& dd, const float** kappa_dev) {
    *kappa_dev = nullptr;
    const Multistep* m = ch.s->ms;
    if (!m) return 0;
    float* dst = (float*)dd.tab + (size_t)dd.n_steps * 5;
    HIPCHK(hipMemcpyAsync(dst, m->kappa.data(), m->kappa.size() * sizeof(float), hipMemcpyHostToDevice, ch.stream));
    HIPCHK(hipStreamSynchronize(ch.stream));
    *kappa_dev = dst;
    return 0;
}

// what a 2-D DDIM entry checks of an armed multistep solver, after chain2_refuse
static int ms_begin2(ChainArmed& took, const Chain2D& ch, const Ddim2dCall& dd, const float* x) {
    if (!took.ms.on()) return 0;
    REQUIRE(dd.tab_bytes >= (size_t)dd.n_steps * 6 * sizeof(float), "multistep solver: the DDIM table buffer needs 6 words per step (24 bytes)");
    REQUIRE(((uintptr_t)x & 15) == 0, "multistep solver: the state x must be 16-byte aligned");
    return ms_begin(took, dd.n_steps, dd.coefs, ch.state_floats(), x);
}

// One DDIM step of the 2-D path (ddim_sample; DESIGN 4.5g): the U-Net + ddim2d_update_kernel + step_counter_kernel (t and the step
// index advance on the device from the time_next table).  With grad, the update is ddim2d_guided_update_kernel, which carries the
// guidance shift (DESIGN 4.5k).
// kappa (device, [n_steps]) and hist: the multistep solver's operands (DESIGN 4.5r), or null: its forms of the two update kernels.
static int run_ddim_step2(const Chain2D& ch, const Ddim2dArgs& a, const float* grad = nullptr, const float* kappa = nullptr, float* hist = nullptr) {
    if (cindm_unet2d_forward(ch.u, a.x, 0, ch.s->t_dev, ch.eps(), ch.NI(), ch.unet_ws(), ch.unet_ws_bytes(), ch.stream) != 0) return -1;
    if (kappa && grad) hipLaunchKernelGGL(ddim2d_ms_update_kernel<true>, dim3(ch.update_blocks()), dim3(256), 0, ch.stream, a, grad, kappa, hist);
    else if (kappa) hipLaunchKernelGGL(ddim2d_ms_update_kernel<false>, dim3(ch.update_blocks()), dim3(256), 0, ch.stream, a, (const float*)nullptr, kappa, hist);
    else if (grad) hipLaunchKernelGGL(ddim2d_guided_update_kernel, dim3(ch.update_blocks()), dim3(256), 0, ch.stream, a, grad);
    else hipLaunchKernelGGL(ddim2d_update_kernel, dim3(ch.update_blocks()), dim3(256), 0, ch.stream, a);
    hipLaunchKernelGGL(step_counter_kernel, dim3(1), dim3(64), 0, ch.stream, ch.s->t_dev, a.tnext, (int*)nullptr, (int*)nullptr);
    HIPCHK(hipGetLastError());
    return 0;
}

// The captured step of a DDPM chain.  Guided (inference/inverse_design_2d.py:236-244 with design_guidance = "standard-alpha",
// model/diffusion_2d.py:788-845), per reverse step
//     g = d(force + overlap)/dx at x_t      (cindm_airfoil_design_grad: 6 surrogate forward + input-gradient passes)
//     x_{t-1} = p_sample(x_t)               (Unet forward, boundary sharing, posterior mean + sigma_t z)
//     x_{t-1} -= eta[t] * g                 (eta = coeff_ratio * betas.flip(0), a device table of the caller; guided_shift2d_kernel)
// as ONE hipGraph replayed once per timestep -- no host code, no layout conversion between the three parts.
static auto ddpm_step2(const Chain2D& ch, const Step2IO& io, float* x, const ForceGuide* g = nullptr, const float* eta = nullptr) {
    return [=](int) -> int {
        if (g && g->gradient(ch, x) != 0) return -1;
        if (run_step2(ch, io, 1, 0, ch.s->t_dev) != 0) return -1;
        if (g) {
            const int64_t n4 = ch.state_floats() / 4;
            hipLaunchKernelGGL(guided_shift2d_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, ch.stream, x, g->grad, eta, ch.s->t_dev, n4);
            HIPCHK(hipGetLastError());
        }
        // (after the step's counter launch: the word is the next timestep; the shift is a guided step's last writer of the state,
        // the known node, when a region is armed, the step's)
        if (ch.s->kn && known2_node(ch, x, 0) != 0) return -1;
        return ch.s->rec ? rec_node(ch.s, x, 0, ch.stream) : 0;
    };
}

// The captured step of a DDIM chain.  Guided (DESIGN 4.5k), per DDIM step i, pair (t, t_next),
//     g = d(force + overlap)/dx at x_t      (cindm_airfoil_design_grad)
//     x' = the DDIM update of x_t           (Unet forward + the unguided chain's update, the same draws)
//     x_next = x' - weights[i] * g          (in the same launch: ddim2d_guided_update_kernel)
// weights ride in the 4th word of the caller's per-step table rows.
static auto ddim_step2(const Chain2D& ch, const Ddim2dArgs& a, float* x, const ForceGuide* g = nullptr, const float* kappa = nullptr,
                       float* hist = nullptr) {
    return [=](int) -> int {
        if (g && g->gradient(ch, x) != 0) return -1;
        if (run_ddim_step2(ch, a, g ? g->grad : nullptr, kappa, hist) != 0) return -1;
        if (ch.s->kn && known2_node(ch, x, 0) != 0) return -1;
        return ch.s->rec ? rec_node(ch.s, x, 0, ch.stream) : 0;
    };
}

// A surrogate-guided 2-D chain with its recovery (as run_chain_with_recovery of the 1-D path): the surrogate's GroupNorm derivative
// exchanges partial sums between the workgroups of an image (fu_gn_silu_bwd_cluster_kernel); a partner kept off the chip by foreign load
// times out, poisons that image's gradient with NaN and raises the handle's error word.  x_T is kept in its slice of the caller's
// diffusion workspace; a chain that ends with the word raised is re-run ONCE from it on the exchange-free derivative (counter-based
// noise / read-only tapes: the same draws).  chain() sets the device counter and replays the steps.
template <typename ChainFn>
static int force_chain_with_recovery(const Chain2D& ch, cindm_forceunet* f, float* x, ChainFn chain) {
    const size_t bytes = (size_t)ch.state_floats() * sizeof(float);
    const bool guard = f->O("gn_bwd_fused") >= 2 && !f->O("no_exchange");
    REQUIRE(ch.ws && ch.ws_bytes >= ch.need, "workspace too small (cindm_ddpm2d_workspace_bytes)");
    if (guard) HIPCHK(hipMemcpyAsync(ch.xT(), x, bytes, hipMemcpyDeviceToDevice, ch.stream));
    if (chain() != 0) return -1;
    if (!guard) return 0;
    const int st = cindm_forceunet_status(f, ch.stream);       // (synchronises: an eager chain is handed back checked too)
    if (st < 0) return -1;
    if (st == 0) return 0;
    if (!f->O("recover")) return fail("an in-kernel exchange of the surrogate's GroupNorm derivative timed out (foreign load on the device); "
                                      "option recover = 0: not re-run");
    if (ch.s->ms && ch.s->ms->kappa[0] != 0.f)
        return fail("an in-kernel exchange of the surrogate's GroupNorm derivative timed out, and the chain's first step reads a multistep "
                    "history that the run has overwritten: restore the history and call again");
    HIPCHK(hipMemcpyAsync(x, ch.xT(), bytes, hipMemcpyDeviceToDevice, ch.stream));
    f->nx_force = 1; ++f->recovered;
    const int rc2 = chain();
    f->nx_force = 0;
    if (rc2 != 0) return -1;
    if (cindm_forceunet_status(f, ch.stream) == 1) return fail("an exchange timed out during the exchange-free re-run (internal error)");
    return 0;
}

// The tail of every entry: the device counter at t0, the recorder armed, `step` replayed nsteps times (one hipGraph with use_graph);
// a guided chain runs that under force_chain_with_recovery, behind the x_T snapshot.  ddim: the counter's word is the step index.
template <typename StepFn>
static int run_chain2(ChainArmed& took, const Chain2D& ch, const ForceGuide* g, float* x, int t0, bool ddim, int nsteps, StepFn step) {
    auto chain = [&]() -> int {
        hipLaunchKernelGGL(set_counter_kernel, dim3(1), dim3(64), 0, ch.stream, ch.s->t_dev, t0, 0ull, 0ll);
        rec_arm(ch.s, ddim ? -1 : t0, ddim ? 2 : 0, 0, ch.stream);
        if (ch.s->kn && known2_node(ch, x, 1) != 0) return -1;      // (rule 1; a recovery re-run starts from it again)
        return replay_once(ch.stream, nsteps, ch.use_graph, step);
    };
    return rec_done(took, g ? force_chain_with_recovery(ch, g->f, x, chain) : chain());
}

extern "C" int cindm_ddpm2d_sample(cindm_ddpm1d* s, cindm_unet2d* u, float* x, int64_t B, int32_t nb, int32_t use_average_share,
                                   const float* noise_state_steps, const float* noise_boundary_steps, uint64_t seed,
                                   int64_t sample_offset, int32_t t_start, int32_t t_end, void* ws, size_t ws_bytes,
                                   void* stream_, int32_t use_graph) {
    ChainArmed took(s);
    if (took.refuse_all_but(kServesKnown2, kKnown1Not2D) != 0) return -1;
    Chain2D ch(s, u, B, nb, use_average_share, ws, ws_bytes, nullptr, use_graph);
    const int nsteps = t_start - t_end + 1;
    if (chain2_refuse(ch, x, nullptr, t_start, t_end) != 0) return -1;
    const Draws2 z{noise_state_steps, noise_boundary_steps, seed, sample_offset};
    if (rec_begin2(took, ch, x, nsteps) != 0 || known2_begin(took, ch, x, z) != 0) return -1;
    if (chain_stream(s, stream_, use_graph, &ch.stream) != 0) return -1;
    const Step2IO io = chain_io2(ch, x, z);
    return run_chain2(took, ch, nullptr, x, t_start, false, nsteps, ddpm_step2(ch, io, x));
}

extern "C" int cindm_ddpm2d_sample_ddim(cindm_ddpm1d* s, cindm_unet2d* u, float* x, int64_t B, int32_t nb, int32_t use_average_share,
                                        int32_t n_steps, const int32_t* times, const float* coefs, void* tab, size_t tab_bytes,
                                        const float* noise_state_steps, const float* noise_boundary_steps, uint64_t seed,
                                        int64_t sample_offset, void* ws, size_t ws_bytes, void* stream_, int32_t use_graph) {
    ChainArmed took(s);
    if (took.refuse_all_but(kServesKnown2 | kServesMultistep, kKnown1Not2D) != 0) return -1;
    Chain2D ch(s, u, B, nb, use_average_share, ws, ws_bytes, nullptr, use_graph);
    const Ddim2dCall dd{n_steps, times, coefs, nullptr, tab, tab_bytes};
    if (chain2_refuse(ch, x, &dd) != 0 || ms_begin2(took, ch, dd, x) != 0) return -1;
    if (took.rec.on()) REQUIRE(n_steps >= 1, "n_steps must be >= 1");
    const Draws2 z{noise_state_steps, noise_boundary_steps, seed, sample_offset};
    if (rec_begin2(took, ch, x, n_steps, kNoX0Ddim2d) != 0 || known2_begin(took, ch, x, z) != 0) return -1;
    if (chain_stream(s, stream_, use_graph, &ch.stream) != 0) return -1;
    int* tn_dev = nullptr;      // the per-step tables go to the caller's device buffer
    if (upload_ddim_tables(s->T, n_steps, times, coefs, (float*)tab, ch.stream, &tn_dev) != 0) return -1;
    const float* kappa_dev = nullptr;
    if (ms_tables2(ch, dd, &kappa_dev) != 0) return -1;
    took.kn.tnext = tn_dev;
    const Ddim2dArgs a = ddim_args2(ch, x, dd, tn_dev, z);
    return run_chain2(took, ch, nullptr, x, times[0], true, n_steps, ddim_step2(ch, a, x, nullptr, kappa_dev, kappa_dev ? took.ms.hist : nullptr));
}

// Design-guided 2-D sampling with the airfoil objective INSIDE the captured step (ddpm_step2)
extern "C" int cindm_ddpm2d_sample_force(cindm_ddpm1d* s, cindm_unet2d* u, cindm_forceunet* f, float* x, int64_t B, int32_t nb,
                                         int32_t use_average_share, const float* noise_state_steps,
                                         const float* noise_boundary_steps, uint64_t seed, int64_t sample_offset,
                                         int32_t t_start, int32_t t_end, int32_t frames, float p_min, float p_max,
                                         float lambda_force, float lambda_overlap, int32_t down_factor, int32_t sum_boundary,
                                         const float* eta, float* grad, void* ws, size_t ws_bytes, void* ws_force,
                                         size_t ws_force_bytes, void* stream_, int32_t use_graph) {
    ChainArmed took(s);
    if (took.refuse_all_but(kServesKnown2, kKnown1Not2D) != 0) return -1;
    Chain2D ch(s, u, B, nb, use_average_share, ws, ws_bytes, nullptr, use_graph);
    const ForceGuide g{f, frames, p_min, p_max, lambda_force, lambda_overlap, down_factor, sum_boundary, grad, ws_force, ws_force_bytes};
    const int nsteps = t_start - t_end + 1;
    if (chain2_refuse(ch, x, nullptr, t_start, t_end) != 0 || force_refuse(ch, g, x, eta) != 0) return -1;
    const Draws2 z{noise_state_steps, noise_boundary_steps, seed, sample_offset};
    if (rec_begin2(took, ch, x, nsteps) != 0 || known2_begin(took, ch, x, z) != 0) return -1;
    if (chain_stream(s, stream_, use_graph, &ch.stream) != 0) return -1;
    const Step2IO io = chain_io2(ch, x, z);
    return run_chain2(took, ch, &g, x, t_start, false, nsteps, ddpm_step2(ch, io, x, &g, eta));
}

// Guided DDIM of the 2-D path with the airfoil objective inside the captured step (ddim_step2)
extern "C" int cindm_ddpm2d_sample_ddim_force(cindm_ddpm1d* s, cindm_unet2d* u, cindm_forceunet* f, float* x, int64_t B, int32_t nb,
                                              int32_t use_average_share, int32_t n_steps, const int32_t* times, const float* coefs,
                                              const float* weights, void* tab, size_t tab_bytes, const float* noise_state_steps,
                                              const float* noise_boundary_steps, uint64_t seed, int64_t sample_offset, int32_t frames,
                                              float p_min, float p_max, float lambda_force, float lambda_overlap, int32_t down_factor,
                                              int32_t sum_boundary, float* grad, void* ws, size_t ws_bytes, void* ws_force,
                                              size_t ws_force_bytes, void* stream_, int32_t use_graph) {
    ChainArmed took(s);
    if (took.refuse_all_but(kServesKnown2 | kServesMultistep, kKnown1Not2D) != 0) return -1;
    Chain2D ch(s, u, B, nb, use_average_share, ws, ws_bytes, nullptr, use_graph);
    const Ddim2dCall dd{n_steps, times, coefs, weights, tab, tab_bytes};
    const ForceGuide g{f, frames, p_min, p_max, lambda_force, lambda_overlap, down_factor, sum_boundary, grad, ws_force, ws_force_bytes};
    if (chain2_refuse(ch, x, &dd) != 0 || force_refuse(ch, g, x, weights) != 0 || ms_begin2(took, ch, dd, x) != 0) return -1;
    if (took.rec.on()) REQUIRE(n_steps >= 1, "n_steps must be >= 1");
    const Draws2 z{noise_state_steps, noise_boundary_steps, seed, sample_offset};
    if (rec_begin2(took, ch, x, n_steps, kNoX0Ddim2d) != 0 || known2_begin(took, ch, x, z) != 0) return -1;
    if (chain_stream(s, stream_, use_graph, &ch.stream) != 0) return -1;
    int* tn_dev = nullptr;
    if (upload_ddim_tables(s->T, n_steps, times, coefs, (float*)tab, ch.stream, &tn_dev, weights) != 0) return -1;
    const float* kappa_dev = nullptr;
    if (ms_tables2(ch, dd, &kappa_dev) != 0) return -1;
    took.kn.tnext = tn_dev;
    const Ddim2dArgs a = ddim_args2(ch, x, dd, tn_dev, z);
    return run_chain2(took, ch, &g, x, times[0], true, n_steps, ddim_step2(ch, a, x, &g, kappa_dev, kappa_dev ? took.ms.hist : nullptr));
}
