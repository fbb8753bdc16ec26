// ---- GaussianDiffusion1D: the schedule handle, the reverse step and the six sampling chains --------------------------------------------
// Textually included by cindm_hip.hip after chain_host.inc (the chain driver, the recorder, the design tables) and before the 2-D host
// files (run_chain2 launches set_counter_kernel, which is defined here).  Each fact is stated once:
//   state_len                  the state length per sample that a compose descriptor implies
//   compose_direct             when the U-Net reads the state in place: no gather launch, no gathered-input slice
//   step_layout                the step workspace, [pair in | pair eps | single in | single eps | U-Net workspaces | staging | x_T | DDIM tables]
//   Chain1D                    what every helper below is handed unchanged, that layout (computed once, by its constructor) and its slices
//   step1_refuse               what a step refuses of its Chain1D and state
//   run_step                   one step: [gather,] U-Net(s), update, [counter,] [known node,] [record node]
//   known1_begin, known1_node  the known region of a chain (cindm_ddpm1d_set_known1d): its check against the state, and its launch
//   chain1_refuse, guided_refuse   what a chain entry refuses, on top of that, before it touches the device
//   start_loop, replay_steps, run_chain_with_recovery   step state, replay (graph cached by key, ping-pong pair + odd tail, flag polls), recovery
//   chain_io, key_common       the StepIO every chain sets the same way, and what of it a captured step embeds
//   ddim_tables1               the DDIM preamble: per-step tables into the workspace's slice
//   loop_steps, loop_chain     the unguided loop and the chain that is one such loop
//   guided_step, guided_chain  the recurrence iterations of a guided step and the guided chains' tail
// An entry is: ChainArmed (everything armed on the handle, chain_host.inc), Chain1D, refuse_all_but what it serves, its other refusals, rec_begin,
// known1_begin, (DDIM: ms_begin,) chain_stream, (DDIM: ddim_tables1,) chain_io plus what it adds, and one call of loop_chain, guided_chain or its own body (the rollout).

extern "C" int cindm_ddpm1d_create(const cindm_sched_desc* d, cindm_ddpm1d** out) {
    REQUIRE(d && out && d->timesteps > 0, "bad schedule descriptor");
    const float* src[13] = {d->betas, d->alphas_cumprod, d->alphas_cumprod_prev, d->sqrt_alphas_cumprod,
                            d->sqrt_one_minus_alphas_cumprod, d->log_one_minus_alphas_cumprod,
                            d->sqrt_recip_alphas_cumprod, d->sqrt_recipm1_alphas_cumprod, d->posterior_variance,
                            d->posterior_log_variance_clipped, d->posterior_mean_coef1, d->posterior_mean_coef2,
                            d->loss_weight};
    for (auto p : src) REQUIRE(p, "null schedule table");
    auto* h = new cindm_ddpm1d();
    h->T = d->timesteps;
    if (hipMalloc((void**)&h->tab, 13 * (size_t)h->T * sizeof(float)) != hipSuccess ||
        hipMalloc((void**)&h->t_dev, 256) != hipSuccess) { delete h; return fail("hipMalloc failed"); }
    for (int i = 0; i < 13; ++i)
        if (hipMemcpy(h->tab + (size_t)i * h->T, src[i], h->T * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) {
            delete h; return fail("hipMemcpy failed");
        }
    *out = h;
    return 0;
}

extern "C" void cindm_ddpm1d_destroy(cindm_ddpm1d* h) {
    if (!h) return;
    if (h->tab) (void)hipFree(h->tab);
    if (h->t_dev) (void)hipFree(h->t_dev);
    h->drop_graph();
    if (h->own) (void)hipStreamDestroy(h->own);
    delete h;
}

// state length per sample is implied by the compose descriptor
static int state_len(const cindm_unet1d* pair, const cindm_compose_desc* c) {
    if (c->mode == CINDM_COMPOSE_PLAIN || c->mode == CINDM_COMPOSE_MULTIBODY) return pair->d.horizon - c->cond_steps;
    return c->window + (c->n_windows - 1) * c->compose_start_step - c->cond_steps;
}

// The U-Net reads the state x directly -- no compose_gather_kernel launch, no gathered-input slice -- when nothing is prepended and
// the gathered batch would BE the state: plain mode, or a composition of one window and one pair.
static bool compose_direct(const cindm_compose_desc* c) {
    return c->cond_steps == 0 && (c->mode == CINDM_COMPOSE_PLAIN || (c->mode >= 1 && c->mode <= 4 && c->n_windows == 1 && c->n_bodies == 2));
}

struct StepLayout {
    int64_t pair_rows = 0, single_rows = 0;
    int pair_F = 0, Tw = 0, Lfull = 0;
    int Ltot = 0; int64_t n_state = 0;      // state_len, and the floats of the state x: [B][Ltot][n_bodies * 4]
    size_t off_pair_in = 0, off_pair_eps = 0, off_single_in = 0, off_single_eps = 0, off_ws_pair = 0, off_ws_single = 0, off_tmp = 0, total = 0;
    size_t off_xT = 0, off_ddim = 0;      // the chain's x_T snapshot (recovery, DESIGN 4.12) and the DDIM loop's per-step tables: caller-owned too
    bool direct = false;     // compose_direct
};

static int step_layout(const cindm_unet1d* pair, const cindm_unet1d* uncond, const cindm_compose_desc* c, int64_t B, StepLayout& s) {
    REQUIRE(pair && c && B > 0, "null argument");
    REQUIRE(pair->finalized, "pair model not finalized");
    const int nb = c->n_bodies, F = nb * 4;
    s.Ltot = state_len(pair, c); s.n_state = B * (int64_t)s.Ltot * F;
    s.Lfull = s.Ltot + c->cond_steps;
    if (c->mode == CINDM_COMPOSE_PLAIN) {
        REQUIRE(pair->d.transition_dim == F, "plain mode: model transition_dim must equal 4*n_bodies");
        REQUIRE(pair->d.horizon == s.Lfull, "plain mode: model horizon must equal cond_steps + state length");
        s.pair_rows = B; s.pair_F = F; s.Tw = s.Lfull;
    } else if (c->mode == CINDM_COMPOSE_MULTIBODY) {
        REQUIRE(uncond && uncond->finalized, "multibody mode needs a finalized unconditioned model");
        REQUIRE(nb >= 2 && pair->d.transition_dim == 8 && uncond->d.transition_dim == 4, "multibody: pair model F=8, single model F=4");
        REQUIRE(pair->d.horizon == s.Lfull && uncond->d.horizon == s.Lfull, "multibody: model horizon must equal cond_steps + state length");
        s.pair_rows = (int64_t)nb * (nb - 1) / 2 * B; s.single_rows = (int64_t)nb * B; s.pair_F = 8; s.Tw = s.Lfull;
    } else {
        REQUIRE(c->mode >= 1 && c->mode <= 4, "unknown compose mode");
        REQUIRE(nb >= 2 && pair->d.transition_dim == 8, "composition needs a 2-body (F=8) model");
        REQUIRE(c->window == pair->d.horizon, "window must equal the model horizon");
        REQUIRE(c->n_windows >= 1 && (c->n_windows - 1) * c->compose_start_step + c->window == s.Lfull,
                "state length must be window + n_composed * compose_start_step");
        REQUIRE(c->n_windows == 1 || (c->compose_start_step >= 1 && c->compose_start_step <= c->window), "windows must cover every step");
        REQUIRE(!(c->mode >= 3 && c->cond_steps > 0), "outside composition with conditioned_steps > 0 is not supported");
        s.pair_rows = (int64_t)c->n_windows * (nb * (nb - 1) / 2) * B; s.pair_F = 8; s.Tw = c->window;
    }
    s.direct = compose_direct(c);
    auto al = [](size_t v) { return (v + 255) / 256 * 256; };
    size_t o = 0;
    s.off_pair_in = o; if (!s.direct) o += al((size_t)s.pair_rows * s.Tw * s.pair_F * 4);
    s.off_pair_eps = o; o += al((size_t)s.pair_rows * s.Tw * s.pair_F * 4);
    s.off_single_in = o; o += al((size_t)s.single_rows * s.Tw * 4 * 4);
    s.off_single_eps = o; o += al((size_t)s.single_rows * s.Tw * 4 * 4);
    s.off_ws_pair = o; o += al(cindm_unet1d_workspace_bytes(pair, s.pair_rows));
    s.off_ws_single = o; if (s.single_rows) o += al(cindm_unet1d_workspace_bytes(uncond, s.single_rows));
    s.off_tmp = o; o += al((size_t)s.n_state * 4);       // guided steps: x_out staging (the gradient reads neighbours of x); guided DDIM: the second state buffer
    // the sample loops keep the chain's initial state for the exchange-free re-run and the DDIM loop its per-step tables
    // ([T][4] floats + [T] ints): both live in the caller's workspace -- no allocation after *_create (SURVEY section 8b)
    s.off_xT = o; o += al((size_t)s.n_state * 4);
    s.off_ddim = o; o += al((size_t)pair->d.timesteps * 5 * 4);
    s.total = o + 256;
    return 0;
}

extern "C" size_t cindm_ddpm1d_workspace_bytes(const cindm_ddpm1d* h, const cindm_unet1d* pair, const cindm_unet1d* uncond,
                                               const cindm_compose_desc* c, int64_t B) {
    (void)h;
    StepLayout s;
    if (!pair || !c) return 0;
    return step_layout(pair, uncond, c, B, s) == 0 ? s.total : 0;
}

extern "C" int cindm_ddpm1d_launches_per_step(const cindm_ddpm1d*, const cindm_unet1d* pair, const cindm_unet1d* uncond,
                                              const cindm_compose_desc* c) {
    if (!pair || !c) return 0;
    int n = pair->launches + 1;                       // U-Net + update
    if (!compose_direct(c)) n += 1;                   // gather
    if (c->mode == CINDM_COMPOSE_MULTIBODY && uncond) n += uncond->launches;
    return n;
}

// Kernel launches of the reverse step emitted last (gather + U-Net(s) + update + step counter, as launched -- not a
// model of it), and whether its update ran inside ups_last_kernel.  The captured graph replays exactly that sequence.
extern "C" int cindm_ddpm1d_last_step_info(const cindm_ddpm1d* h, int32_t* launches, int32_t* fused_update) {
    REQUIRE(h && launches && fused_update, "null argument");
    *launches = h->last_step_launches; *fused_update = h->last_step_fused;
    return 0;
}

// What the 1-D steps and chains hand unchanged to every helper below them, with the layout of the workspace.  The constructor
// computes the layout ONCE per entry call (two cindm_unet1d_workspace_bytes look-ups); nothing below it computes one.  That holds
// for the whole call because the layout depends only on the handles' pack generation, the row counts and the run-time
// "no_exchange" option: cindm_unet1d_workspace_bytes returns the larger of the exchange and the exchange-free plan, so the recovery
// re-run and the crowded-device demotion inside run_chain_with_recovery see the same offsets.  It is not kept across entry calls.
// A layout that step_layout refuses leaves its text in `refusal`, which step1_refuse hands out before anything reads a slice.
struct Chain1D {
    cindm_ddpm1d* h; cindm_unet1d* pair; cindm_unet1d* uncond; const cindm_compose_desc* c;
    int64_t B; void* ws; size_t ws_bytes; hipStream_t stream; int use_graph;
    StepLayout s; std::string refusal;
    Chain1D(cindm_ddpm1d* h_, cindm_unet1d* pair_, cindm_unet1d* uncond_, const cindm_compose_desc* c_, int64_t B_, void* ws_, size_t ws_bytes_,
            hipStream_t stream_, int use_graph_)
        : h(h_), pair(pair_), uncond(uncond_), c(c_), B(B_), ws(ws_), ws_bytes(ws_bytes_), stream(stream_), use_graph(use_graph_) {
        if (step_layout(pair, uncond, c, B, s) != 0) refusal = g_err;
    }
    cindm_unet1d* un() const { return c->mode == CINDM_COMPOSE_MULTIBODY ? uncond : nullptr; }      // the second model a chain really runs
    int Ltot() const { return s.Ltot; }
    int64_t n_state() const { return s.n_state; }             // floats of the state x
    template <typename T = float> T* at(size_t off) const { return reinterpret_cast<T*>((char*)ws + off); }
    float* pair_in() const { return s.direct ? nullptr : at(s.off_pair_in); }      // (direct: the U-Net reads x)
    float* pair_eps() const { return at(s.off_pair_eps); }
    float* single_in() const { return at(s.off_single_in); }
    float* single_eps() const { return at(s.off_single_eps); }
    void* ws_pair() const { return at<char>(s.off_ws_pair); }
    size_t ws_pair_bytes() const { return ws_bytes - s.off_ws_pair; }
    void* ws_single() const { return at<char>(s.off_ws_single); }
    size_t ws_single_bytes() const { return ws_bytes - s.off_ws_single; }
    float* stage() const { return at(s.off_tmp); }      // the guided steps' staging slice / the guided DDIM chain's second state buffer
    float* xT() const { return at(s.off_xT); }
    float* ddim_tab() const { return at(s.off_ddim); }
};

struct StepIO {
    const float* x; const float* cond; float* mean_out; float* x0_out; float* eps_out; float* x_out;
    const float* noise; int64_t noise_t_stride; uint64_t seed; int64_t sample_off; int add_noise;
    const float* inp_cond; int inp_steps; const float* inp_noise; int64_t inp_noise_t_stride;
    int dec_t;              // sample loop: decrement the device step counter at the end of the step
    const float* ddim_tab; const int* ddim_tnext;      // DDIM loop: per-step coefficient / time_next tables (device)
    const unsigned long long* dyn;                     // sample loops: (seed, sample_off) live in device memory
    const cindm_design_desc* dz;                       // built-in design objective (guided loop) or null
    int relax; const float* recur_noise; int64_t recur_t_stride; uint32_t recur_tag;
    const float* iso; int iso_steps;
    int pingpong, parity;   // plain sample loop: step state in two slots, advanced by the update itself (no step_counter launch)
    int state_pp;           // guided DDIM loop: x_out is the OTHER of two state buffers -- the update writes it directly (no staging, no copy)
    const float* ula_tab; int ula_L, ula_t_hi;         // Langevin loop: per-timestep (scalar, ss, std, -) rows (device), inner count, first timestep
    int rec;                // recorded chain: the recorder's stream mask on the call that ends a step (chain_record_kernel follows it), else 0
    int kn, relax_idx;      // chain with a known region: known1d_kernel follows every update; the relaxation's index (a constant of the captured iteration)
    const TimeComposeArgs* tc;     // parallel time composition (timecompose_host.inc): its update kernel's own operands, or null
    float* ms_hist;         // DDIM chain with the multistep solver: the history its update reads and writes (kappa rides in the table rows), or null
};

// What a step refuses of its Chain1D and state (x, and cond where the descriptor prepends it): run_step's own checks
// (cindm_ddpm1d_step and _predict reach it directly), which the chain entries make up front (chain1_refuse).
static int step1_refuse(const Chain1D& ch, const float* x, const float* cond) {
    REQUIRE(ch.h && ch.pair && ch.c && x && ch.ws, "null argument");
    // the U-Net's time path is a per-timestep table of d.timesteps rows: a longer diffusion would index past it
    REQUIRE(ch.h->T <= ch.pair->d.timesteps && (!ch.uncond || ch.h->T <= ch.uncond->d.timesteps),
            "the diffusion has more timesteps than the U-Net's per-timestep table (construct TemporalUnet1D(..., timesteps=T))");
    REQUIRE(ch.c->cond_steps == 0 || cond, "cond_steps > 0 requires cond");
    REQUIRE(((uintptr_t)ch.ws & 255) == 0, "workspace must be 256-byte aligned");
    if (!ch.refusal.empty()) return fail(ch.refusal);
    REQUIRE(ch.Ltot() > 0, "empty state");
    REQUIRE(ch.ws_bytes >= ch.s.total, "workspace too small (cindm_ddpm1d_workspace_bytes)");
    return 0;
}

// clears the exchange regions of the U-Net workspaces inside a step workspace (before a step is captured into a graph)
static int prepare_step_ws(const Chain1D& ch) {
    if (unet1d_prepare_ws(ch.pair, ch.ws_pair(), ch.s.pair_rows, ch.stream) != 0) return -1;
    if (ch.s.single_rows && unet1d_prepare_ws(ch.uncond, ch.ws_single(), ch.s.single_rows, ch.stream) != 0) return -1;
    return 0;
}

// The known region of a 1-D chain (DESIGN 4.5o): checked against the chain's state before the entry's first launch or copy, then held
// by the handle for the whole call.  recur_iters: the iterations per step of a guided chain (a relaxation tape holds that many records
// per row), 0 for the unguided ones.
static int known1_begin(ChainArmed& took, const Chain1D& ch, const float* x, int recur_iters) {
    if (!took.kn1.on()) return 0;
    const Known1D& k = took.kn1;
    const int F = ch.c->n_bodies * 4;
    if (k.batch != ch.B || k.rows != ch.Ltot() || k.feats != F)
        return fail("known region (1-D): made for " + std::to_string(k.batch) + " designs of " + std::to_string(k.rows) + " rows x " +
                    std::to_string(k.feats) + " features, the chain's state is " + std::to_string(ch.B) + " x " + std::to_string(ch.Ltot()) +
                    " x " + std::to_string(F));
    REQUIRE((((uintptr_t)x | (uintptr_t)ch.stage()) & 15) == 0, "known region (1-D): the state x and the workspace's second state buffer must be "
                                                                "16-byte aligned (the node moves 16 bytes per lane)");
    if (k.z_step) {
        REQUIRE(k.step_stride >= ch.n_state() && (k.step_stride & 3) == 0, "known region (1-D): the step tape's stride is smaller than one state or no multiple of 4");
        if (recur_iters > 1) {
            REQUIRE(k.z_recur, "known region (1-D): a guided chain with relaxation iterations and a tape needs the relaxation tape too");
            REQUIRE(k.recur_stride >= (int64_t)recur_iters * ch.n_state() && (k.recur_stride & 3) == 0,
                    "known region (1-D): the relaxation tape's stride is smaller than the step's iterations x one state, or no multiple of 4");
        }
    }
    took.h->kn1 = &took.kn1;
    return 0;
}

// the known node on the buffer `x` the last launch wrote, reading the step-state slot `st` it wrote: mode 0 a step's last update,
// 1 rule 1 (the chain body's), 2 after relaxation `relax_idx`
static int known1_node(const Chain1D& ch, const StepIO& io, float* x, const int* st, int mode, int relax_idx) {
    const Known1D& k = *ch.h->kn1;
    Known1dArgs a; std::memset(&a, 0, sizeof(a));
    a.x = x; a.known = k.known; a.mask = k.mask; a.B = ch.B; a.Ltot = ch.Ltot(); a.F = ch.c->n_bodies * 4;
    a.known_per_design = k.known_per_design; a.mask_per_design = k.mask_per_design;
    a.sqrt_ac = ch.h->tab + 3 * (size_t)ch.h->T; a.sqrt_1mac = ch.h->tab + 4 * (size_t)ch.h->T;
    a.st = st; a.tnext = io.ddim_tab ? io.ddim_tnext : nullptr;
    a.mode = mode; a.init_tag = (uint32_t)ch.h->T; a.relax_idx = relax_idx;
    a.z_init = k.z_init; a.z_step = k.z_step; a.z_step_stride = k.step_stride;
    a.z_recur = (k.z_step && k.z_recur) ? k.z_recur + (size_t)relax_idx * ch.n_state() : nullptr; a.z_recur_stride = k.recur_stride;
    a.dyn = io.dyn;
    hipLaunchKernelGGL(known1d_kernel, dim3((unsigned)((ch.n_state() / 4 + 255) / 256)), dim3(256), 0, ch.stream, a);
    HIPCHK(hipGetLastError());
    return 0;
}

// One launch of the element-wise update: the instantiation of compose_update_body by the armed objective (dz_mode: 5 quadratic, 6 pair
// distance, 7 the sum, whose tables `dsum` holds; anything else the position objectives or none) and by `hist`, the multistep
// solver's history (null: the update without the multistep term).
static void launch_compose_update(const ComposeArgs& a, const DesignSum& dsum, float* hist, int64_t ne, hipStream_t stream) {
    const dim3 grid((unsigned)((ne + 255) / 256));
    const int dzm = a.dz_mode & kDzModeMask;
    if (dzm == kDesignSumMode) launch_compose_update_sum(a, dsum, hist, ne, stream);
    else if (dzm == 6) launch_compose_update_pair(a, hist, ne, stream);
    else if (dzm == 5 && hist) hipLaunchKernelGGL(compose_update_ms_quad_kernel, grid, dim3(256), 0, stream, a, hist);
    else if (dzm == 5) hipLaunchKernelGGL(compose_update_quad_kernel, grid, dim3(256), 0, stream, a);
    else if (hist) hipLaunchKernelGGL(compose_update_ms_kernel, grid, dim3(256), 0, stream, a, hist);
    else hipLaunchKernelGGL(compose_update_kernel, grid, dim3(256), 0, stream, a);
}

static int run_step(const Chain1D& ch, const StepIO& io, int32_t t, const int32_t* t_dev) {
    if (step1_refuse(ch, io.x, io.cond) != 0) return -1;
    cindm_ddpm1d* h = ch.h; cindm_unet1d* pair = ch.pair; cindm_unet1d* uncond = ch.uncond; const cindm_compose_desc* c = ch.c;
    const StepLayout& s = ch.s; const int64_t B = ch.B; const int Ltot = s.Ltot; hipStream_t stream = ch.stream;
    REQUIRE(t_dev || (t >= 0 && t < h->T), "timestep out of range");
    ComposeArgs a;
    std::memset(&a, 0, sizeof(a));
    a.mode = c->mode; a.W = (c->mode >= 1 && c->mode <= 4) ? c->n_windows : 1; a.cs = c->compose_start_step;
    a.T = s.Tw; a.nb = c->n_bodies; a.cond_steps = c->cond_steps; a.objective = c->objective; a.clip = c->clip_denoised;
    a.uncond_coef = c->uncond_coef; a.B = B; a.Ltot = Ltot; a.F = c->n_bodies * 4;
    a.x = io.x; a.cond = io.cond;
    a.pair_in = ch.pair_in();
    a.pair_eps = ch.pair_eps();
    a.single_in = ch.single_in();
    a.single_eps = ch.single_eps();
    const float* tb = h->tab; const size_t T = h->T;
    a.sqrt_ac = tb + 3 * T; a.sqrt_1mac = tb + 4 * T; a.sqrt_recip = tb + 6 * T; a.sqrt_recipm1 = tb + 7 * T;
    a.logvar = tb + 9 * T; a.coef1 = tb + 10 * T; a.coef2 = tb + 11 * T;
    a.t_ptr = t_dev; a.t_imm = t;
    const int q = io.pingpong ? (io.parity & 1) : 0;
    pair->epoch_slot = 8 * q;
    if (uncond) uncond->epoch_slot = 8 * q;
    if (io.pingpong) {
        // this step reads t at t_dev[4 q] and its epochs at epoch_dev[8 q]; its update writes the other slots for the next step
        t_dev = h->t_dev + 4 * q;
        a.t_ptr = t_dev;
        a.t_next = h->t_dev + 4 * (1 - q);
        a.ep_cur0 = pair->epoch_dev + 8 * q; a.ep_next0 = pair->epoch_dev + 8 * (1 - q);
        if (c->mode == CINDM_COMPOSE_MULTIBODY && uncond) { a.ep_cur1 = uncond->epoch_dev + 8 * q; a.ep_next1 = uncond->epoch_dev + 8 * (1 - q); }
    }
    a.mean_out = io.mean_out; a.x0_out = io.x0_out; a.eps_out = io.eps_out; a.x_out = io.x_out;
    a.noise = io.noise; a.noise_t_stride = io.noise_t_stride; a.seed = io.seed; a.sample_off = io.sample_off; a.add_noise = io.add_noise;
    a.dyn = io.dyn;
    a.inp_cond = io.inp_cond; a.inp_steps = io.inp_steps; a.inp_noise = io.inp_noise; a.inp_noise_t_stride = io.inp_noise_t_stride;
    if (io.ddim_tab) {
        a.ddim_tab = io.ddim_tab; a.ddim_tnext = io.ddim_tnext; a.step_idx = h->t_dev + 2;
        if (io.pingpong) { a.step_idx = h->t_dev + 4 * q + 2; a.sidx_next = h->t_dev + 4 * (1 - q) + 2; }      // the slot's own step index
    }
    const bool guided = io.dz && io.x_out;
    DesignSum dsum; std::memset(&dsum, 0, sizeof(dsum));      // (read under dz_mode 7 only)
    if (guided) {
        a.dz_mode = io.dz->mode; a.dz_alpha = io.dz->alpha; a.dz_tc = io.dz->time_consistency_coef;
        const int kind = design_kind_of(io.dz->mode);
        if (io.dz->mode == kDesignSumMode) {     // the sum: every kind the chain took, in the update's second argument
            auto taken = [&](int k) -> const DesignTables* { return (h->dzt && h->dzt[k].taken) ? &h->dzt[k] : nullptr; };
            const DesignTables* w = taken(kWaypoint); const DesignTables* qd = taken(kQuadratic); const DesignTables* pd = taken(kPairDist);
            if (!w && !qd && !pd) return fail("design objective mode 7 outside a chain that took design tables (internal error)");
            if (w) {
                dsum.way_target = w->a; dsum.way_scale = w->b;
                dsum.flags |= kSumWay | (w->a_per_design ? kSumWayTargetPerDesign : 0) | (w->b_per_design ? kSumWayScalePerDesign : 0) |
                              (io.dz->last_n_step == 1 ? kSumWayL2 : 0);
            }
            if (qd) {
                dsum.quad_S = qd->a; dsum.quad_h = qd->b;
                dsum.flags |= kSumQuad | (qd->a_per_design ? kSumQuadSPerDesign : 0) | (qd->b_per_design ? kSumQuadHPerDesign : 0);
            }
            if (pd) {
                dsum.pair_band = pd->a; dsum.pair_weight = pd->b;
                dsum.flags |= kSumPair | (pd->a_per_design ? kSumPairBandPerDesign : 0) | (pd->b_per_design ? kSumPairWeightPerDesign : 0);
            }
        } else if (kind >= 0) {     // table objective: the addresses and the per-design flags are operands of the captured update
            const DesignKind& k = kDesignKinds[kind]; const DesignTables* t = (h->dzt && h->dzt[kind].taken) ? &h->dzt[kind] : nullptr;
            if (!t || t->kind != kind)
                return fail(std::string("design objective mode ") + k.modes + " outside a chain that took " + k.label + " (internal error)");
            a.*k.arg_a = t->a; a.*k.arg_b = t->b;
            a.dz_mode |= (t->a_per_design ? kDzTargetPerDesign : 0) | (t->b_per_design ? kDzScalePerDesign : 0);
        } else {
            a.dz_last_n = io.dz->last_n_step; a.dz_coef = io.dz->coef; a.dz_tx = io.dz->pos_target[0]; a.dz_ty = io.dz->pos_target[1];
        }
        a.relax = io.relax; a.recur_noise = io.recur_noise; a.recur_t_stride = io.recur_t_stride; a.recur_tag = io.recur_tag;
        a.iso = io.iso; a.iso_steps = io.iso_steps;
        a.betas = tb; a.ac = tb + 1 * T; a.acp = tb + 2 * T;
        a.x_out = io.state_pp ? io.x_out : ch.stage();
    }

    const float* unet_in = io.x;
    // Time composition of two-body states (config 3: W windows of one pair): the gathered batch is a row-wise COPY of the state --
    // row (window kk, design b) = state[b, kk * cs .. + Tw) -- so the first kernel of the forward reads the state in place and
    // compose_gather_kernel is not launched (option fuse_gather; level0_down_kernel must be the kernel that consumes the input)
    const bool gather_fused = !s.direct && c->mode >= 1 && c->mode <= 4 && c->n_bodies == 2 && c->cond_steps == 0 && !s.single_rows &&
                              pair->O("fuse_gather") && level0_serves_input(pair) && pair->d.horizon == s.Tw && pair->d.transition_dim == 8;
    pair->gatherB = 0;
    if (gather_fused) { pair->gatherB = (int)B; pair->gather_cs = c->compose_start_step; pair->gather_Ltot = Ltot; }
    else if (!s.direct) {
        const int64_t n = (c->mode == CINDM_COMPOSE_PLAIN) ? B * (int64_t)s.Lfull * a.F
                          : s.pair_rows * s.Tw * 8 + s.single_rows * s.Tw * 4;
        hipLaunchKernelGGL(compose_gather_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, a);
        unet_in = a.pair_in;
    }
    // A plain single-model step (configs 1 and 2: the U-Net reads the state, its output row IS the row's prediction, the
    // update is element-wise and in place): ups_last_kernel runs the update on the rows it has just predicted, so the step
    // has no compose_update_kernel launch.  Everything else (composition over windows / pairs, a second U-Net, guidance,
    // callers that want mean / x0 / eps back) keeps the separate kernel.  Round 4: the DDIM loop fuses too (objective pred_noise).
    // sample() reaches this path as COMPOSE_MEAN_OUTSIDE with one window and one pair (p_sample_loop -> outside=True): for
    // s.direct every mode 0..4 aggregates exactly one prediction with weight 1 -- (0 + e) / 1 -- so the element-wise result is
    // the plain one (the bitwise identities outside(mean) == inside == plain are GPU tests) and all of them fuse.
    const bool can_fuse = c->mode >= CINDM_COMPOSE_PLAIN && c->mode <= 4 && s.direct && !s.single_rows && !guided && (!io.ddim_tab || c->objective == 0) &&
                          io.x_out == io.x && !io.mean_out && !io.x0_out && !io.eps_out && !io.inp_cond && pair->O("fuse_update") &&
                          (a.F & 3) == 0 && !io.ms_hist;
    pair->fused_done = false;
    pair->fuse_upd = can_fuse ? &a : nullptr;
    const int frc = cindm_unet1d_forward(pair, unet_in, t, t_dev, ch.pair_eps(), s.pair_rows, ch.ws_pair(), ch.ws_pair_bytes(), stream);
    pair->fuse_upd = nullptr;
    pair->gatherB = 0;
    if (frc != 0) return -1;
    if (s.single_rows &&
        cindm_unet1d_forward(uncond, a.single_in, t, t_dev, ch.single_eps(), s.single_rows, ch.ws_single(), ch.ws_single_bytes(), stream) != 0) return -1;
    const int64_t ne = s.n_state;
    h->last_step_launches = ((s.direct || gather_fused) ? 0 : 1) + pair->issued + (s.single_rows ? uncond->issued : 0) + (pair->fused_done ? 0 : 1) +
                            ((io.dec_t && !io.pingpong) ? 1 : 0);
    h->last_step_fused = pair->fused_done ? 1 : 0;
    if (io.ula_tab) {
        // Langevin iteration: the update moves every row of the (full) state by the composed score; io.noise is the iteration tape
        UlaArgs u;
        u.c = a; u.tab = io.ula_tab; u.L = io.ula_L; u.t_hi = io.ula_t_hi; u.noise_it_stride = io.noise_t_stride;
        hipLaunchKernelGGL(ula_update_kernel, dim3((unsigned)((ne / 4 + 255) / 256)), dim3(256), 0, stream, u);
    } else if (io.tc) {
        // parallel time composition: the DDIM update keyed per segment, with the hand-over of every segment's tail to the next one's condition
        TimeComposeArgs u = *io.tc;
        u.c = a;
        hipLaunchKernelGGL(timecompose_update_kernel, dim3((unsigned)((ne / 4 + 255) / 256)), dim3(256), 0, stream, u);
    } else if (io.ddim_tab && !guided && a.objective != 0 && a.clip) {
        // the unguided DDIM update under pred_x0 / pred_v with the clamp on: pred_noise re-derived from the clamped x_start, as
        // model_predictions(clip_x_start = True) does (never fused: the fused update serves pred_noise only)
        launch_compose_update_clamped(a, io.ms_hist, ne, stream);
    } else if (!pair->fused_done) {
        // (a guided step and a multistep chain are never fused.)  The multistep solver's history goes to a step's update only: a
        // relaxation iteration is not an update and leaves it alone
        launch_compose_update(a, dsum, (io.ms_hist && io.ddim_tab && !(guided && io.relax)) ? io.ms_hist : nullptr, ne, stream);
    }
    pair->epoch_slot = 0;
    if (uncond) uncond->epoch_slot = 0;
    if (io.pingpong) {                       // the update has advanced t and the epochs for the next step
        pair->epoch_prebumped = true;
        if (s.single_rows && uncond) uncond->epoch_prebumped = true;
    } else if (io.dec_t) {
        // the counter kernel also advances the U-Nets' exchange epochs for the step that follows
        if (io.ula_tab) hipLaunchKernelGGL(ula_counter_kernel, dim3(1), dim3(64), 0, stream, h->t_dev, io.ula_L, pair->epoch_dev,
                                           (s.single_rows && uncond) ? uncond->epoch_dev : (int*)nullptr);
        else
        hipLaunchKernelGGL(step_counter_kernel, dim3(1), dim3(64), 0, stream, h->t_dev, io.ddim_tab ? io.ddim_tnext : (const int*)nullptr,
                           pair->epoch_dev, (s.single_rows && uncond) ? uncond->epoch_dev : (int*)nullptr);
        pair->epoch_prebumped = true;
        if (s.single_rows && uncond) uncond->epoch_prebumped = true;
    }
    HIPCHK(hipGetLastError());
    if (guided && !io.state_pp) HIPCHK(hipMemcpyAsync(io.x_out, a.x_out, (size_t)ne * sizeof(float), hipMemcpyDeviceToDevice, stream));
    if (io.kn && h->kn1) {
        // after the update in whichever form, the counter and the staging copy: the node writes the buffer the update wrote and reads
        // the slot it advanced (a relaxation iteration of the guided DDPM step launches no counter: the word is still t)
        if (known1_node(ch, io, io.x_out, io.pingpong ? h->t_dev + 4 * (1 - q) : h->t_dev, (guided && io.relax) ? 2 : 0, io.relax_idx) != 0) return -1;
        h->last_step_launches += 1;
    }
    if (io.rec && h->rec) {
        // after the step's last writer of the state and of the step state: a ping-pong step has just advanced the OTHER slot
        if (rec_node(h, io.x_out, io.pingpong ? 1 - q : 0, stream) != 0) return -1;
        h->last_step_launches += 1;
    }
    return 0;
}

extern "C" int cindm_ddpm1d_predict(cindm_ddpm1d* h, cindm_unet1d* pair, cindm_unet1d* uncond, const cindm_compose_desc* c,
                                    const float* x, const float* cond, int32_t t, const int32_t* t_dev, int64_t B,
                                    float* mean_out, float* x0_out, float* eps_out, void* ws, size_t ws_bytes, void* stream) {
    StepIO io{};
    io.x = x; io.cond = cond; io.mean_out = mean_out; io.x0_out = x0_out; io.eps_out = eps_out;
    return run_step(Chain1D(h, pair, uncond, c, B, ws, ws_bytes, (hipStream_t)stream, 0), io, t, t_dev);
}

extern "C" int cindm_ddpm1d_step(cindm_ddpm1d* h, cindm_unet1d* pair, cindm_unet1d* uncond, const cindm_compose_desc* c,
                                 float* x, const float* cond, const float* noise, uint64_t seed, int64_t sample_offset,
                                 const float* inpaint_cond, int32_t inpaint_steps, const float* inpaint_noise,
                                 int32_t t, const int32_t* t_dev, int64_t B, float* x0_out,
                                 void* ws, size_t ws_bytes, void* stream) {
    StepIO io{};
    io.x = x; io.cond = cond; io.x_out = x; io.x0_out = x0_out;
    io.noise = noise; io.noise_t_stride = 0; io.seed = seed; io.sample_off = sample_offset; io.add_noise = 1;
    io.inp_cond = inpaint_cond; io.inp_steps = inpaint_steps; io.inp_noise = inpaint_noise; io.inp_noise_t_stride = 0;
    return run_step(Chain1D(h, pair, uncond, c, B, ws, ws_bytes, (hipStream_t)stream, 0), io, t, t_dev);
}

// ---- the chains --------------------------------------------------------------------------------------------------------------------------
// What a DDIM entry is handed on top of a DDPM one.
struct Ddim1Call { int32_t n_steps; const int32_t* times; const float* coefs; };

// What every chain entry refuses before it touches the device: step1_refuse and the DDPM range t_start .. t_end or, for a DDIM chain
// (dd), its schedule pointers and the bound of the workspace's table slice, which holds 5 words per U-Net timestep (n_steps < 1 and
// the schedule itself are refused by upload_ddim_tables, before anything is copied).
static int chain1_refuse(const Chain1D& ch, const float* x, const float* cond, const Ddim1Call* dd, int t_start = 0, int t_end = 0) {
    if (dd) REQUIRE(dd->times && dd->coefs, "null argument");
    if (step1_refuse(ch, x, cond) != 0) return -1;
    if (dd) REQUIRE(dd->n_steps <= ch.pair->d.timesteps, "more DDIM steps than the U-Net's timesteps");
    else REQUIRE(t_start < ch.h->T && t_end >= 0 && t_end <= t_start, "bad timestep range");
    return 0;
}

// What a guided entry refuses on top of chain1_refuse (after it): the objective, its tables (design_begin hands them to the handle
// for the call; x: the state the quadratic update reads 16 bytes at a time) and the rows it overwrites.
// min_recurrence: 0 for the DDPM chain (no recurrence: one plain guided iteration), 1 for the DDIM chain.
static int guided_refuse(const Chain1D& ch, ChainArmed& took, const cindm_design_desc* dz, const float* x, int min_recurrence,
                         const float* initial_state_overwrite, int overwrite_steps) {
    REQUIRE(dz, "null argument");
    REQUIRE(dz->mode >= 1 && dz->mode <= 7, "design objective mode must be 1 (L2), 2 (L2square), 3 (table L2), 4 (table L2square), 5 (quadratic tables), 6 (pair-distance tables) or 7 (the sum of the tables armed)");
    if (min_recurrence == 0) REQUIRE(dz->recurrence >= 0 && dz->recurrence <= 64, "recurrence count out of range");
    else REQUIRE(dz->recurrence >= 1 && dz->recurrence <= 64,
                 "guided DDIM needs a recurrence count in 1 .. 64 (without recurrence the reference returns no noise prediction)");
    if (design_begin(took, dz, ch.Ltot(), ch.c->n_bodies, ch.B, x, ch.stage()) != 0) return -1;
    REQUIRE(dz->mode >= 3 || (dz->last_n_step >= 1 && dz->last_n_step <= ch.Ltot()), "last_n_step out of range");
    REQUIRE(!initial_state_overwrite || (overwrite_steps >= 1 && overwrite_steps <= ch.Ltot()), "bad overwrite_steps");
    return 0;
}

// t_dev block: [0] t, [1] unused, [2] DDIM step index; bytes 64..79: (seed, sample_off) read by the update kernel of a loop
__global__ void set_counter_kernel(int* p, int v, unsigned long long seed, long long sample_off) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        p[0] = v; p[1] = 0; p[2] = 0;
        unsigned long long* dyn = reinterpret_cast<unsigned long long*>(p + 16);
        dyn[0] = seed; dyn[1] = (unsigned long long)sample_off;
    }
}
// the sample loops end with a handle whose epoch has been advanced for a step that never runs: harmless (the next
// forward simply uses that epoch), but the flag must describe the stream-ordered truth, so loops clear nothing.

// start of a sample loop: set the device step counter and advance the U-Nets' exchange epochs once, eagerly, so that the
// captured step carries no epoch launch (its counter kernel advances them for the following step)
static void start_loop(const Chain1D& ch, int t0, uint64_t seed, int64_t sample_off) {
    cindm_unet1d* pair = ch.pair; cindm_unet1d* uncond = ch.uncond;
    hipLaunchKernelGGL(set_counter_kernel, dim3(1), dim3(64), 0, ch.stream, ch.h->t_dev, t0, (unsigned long long)seed, (long long)sample_off);
    if (pair->epoch_dev) { hipLaunchKernelGGL(dconv_epoch_kernel, dim3(1), dim3(64), 0, ch.stream, pair->epoch_dev); pair->epoch_prebumped = true; }
    if (ch.un() && uncond->epoch_dev) {
        hipLaunchKernelGGL(dconv_epoch_kernel, dim3(1), dim3(64), 0, ch.stream, uncond->epoch_dev); uncond->epoch_prebumped = true;
    }
}

// run one captured step n times (graph) or launch it n times (stream): the 1-D loops' replay, on the chain driver's stream_steps /
// graph_capture / graph_run (chain_host.inc).  The instantiated graph is kept in the handle and reused while `key` (everything the
// captured launches embed) is unchanged.
template <typename StepFn>
static int replay_steps(const Chain1D& ch, const std::vector<unsigned char>& key, int nsteps, StepFn step, bool pingpong = false) {
    cindm_ddpm1d* h = ch.h; cindm_unet1d* pair = ch.pair; cindm_unet1d* uncond = ch.un(); hipStream_t stream = ch.stream;
    // a chain is only handed back after the exchange flags of its U-Nets have been read: a timed-out partner (not
    // co-resident under foreign load) would otherwise return designs computed from garbage statistics.  Returns 1 for a
    // time-out (run_chain_with_recovery re-runs the chain on the exchange-free kernels), -1 for an error.
    auto finish = [&]() -> int {
        if (pingpong) {          // the slot an eager forward reads may hold an older epoch than the loop's last step used: bump next time
            pair->epoch_prebumped = false;
            if (uncond) uncond->epoch_prebumped = false;
        }
        const int r0 = unet1d_poll_flag(pair, stream);
        const int r1 = uncond ? unet1d_poll_flag(uncond, stream) : 0;
        if (r0 < 0 || r1 < 0) return -1;
        return (r0 == 1 || r1 == 1) ? 1 : 0;
    };
    if (!ch.use_graph) return stream_steps(nsteps, step) != 0 ? -1 : finish();
    // ping-pong loops (the step state alternates between two slots, the step's own update advances it): the graph holds TWO
    // steps (parity 0 then 1); an odd count ends with a one-step graph of parity 0 -- after an even number of steps the
    // current state is in slot 0 again
    const int per = pingpong ? 2 : 1;
    if (!(h->gexec && h->gkey == key)) {
        h->drop_graph();
        hipGraph_t graph = nullptr; hipGraphExec_t exec = nullptr;
        if (graph_capture(stream, per, step, &graph, &exec) != 0) return -1;
        h->graph = graph; h->gexec = exec; h->gkey = key;
    }
    const bool odd = pingpong && (nsteps & 1);
    if (odd && !h->gexec1) {
        hipGraph_t graph = nullptr; hipGraphExec_t exec = nullptr;
        if (graph_capture(stream, 1, step, &graph, &exec) != 0) return -1;
        h->graph1 = graph; h->gexec1 = exec;
    }
    if (graph_run(stream, h->gexec, nsteps / per, odd ? h->gexec1 : nullptr) != 0) { h->drop_graph(); return -1; }
    return finish();
}

// A chain (one sample-loop call) with its recovery: `body` runs the loop and returns replay_steps' code.  When an in-kernel
// exchange between workgroups timed out (1) -- foreign load on the device kept a partner workgroup from becoming resident
// within the spin bound; the chain's state is garbage from that step on -- the state is restored to the chain's x_T (kept in its
// slice of the caller's workspace) and the chain is re-run ONCE with both U-Nets in exchange-free mode (per-layer kernels, nothing
// to time out); the handles go back to the fast kernels afterwards.  The counter-based noise is a function of (seed, sample, step),
// tapes are read-only: the re-run draws what the first run drew.
// One sampling chain per device at a time is the rule of the exchange kernels (their workgroups wait for partners that must be
// co-resident: a second chain on another stream keeps them off the chip, DESIGN 4.12).  The registry counts the chains in flight
// per device IN THIS PROCESS: a chain that starts while another is running takes the exchange-free plan up front -- correct, about
// 10 % slower, no time-out, no re-run -- and the Python face warns once.  (Other processes on the device cannot be seen from here;
// against them the bounded spin + recovery below remains.)  Concurrent chains need their own U-Net handles.
static std::atomic<int> g_chains_in_flight[64];
struct ChainInFlight {
    std::atomic<int>* c = nullptr; int prev = 0;
    ChainInFlight() { int dev = 0; if (hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < 64) { c = &g_chains_in_flight[dev]; prev = c->fetch_add(1); } }
    ~ChainInFlight() { if (c) c->fetch_sub(1); }
};

template <typename Body>
static int run_chain_with_recovery(const Chain1D& ch, float* x, Body body) {
    cindm_ddpm1d* h = ch.h; cindm_unet1d* pair = ch.pair; cindm_unet1d* uncond = ch.un(); hipStream_t stream = ch.stream;
    const size_t bytes = (size_t)ch.n_state() * sizeof(float);
    // one chain at a time per U-Net handle: the recovery and the up-front demotion below flip the handle's plan switches (no_xchg_force, the
    // cached graph) without a lock -- concurrent chains need their own handles, and a second one on the same handle is an error, not a race
    struct Busy {
        cindm_unet1d* a; cindm_unet1d* b; bool ok;
        Busy(cindm_unet1d* a_, cindm_unet1d* b_) : a(a_), b(b_ && b_ != a_ ? b_ : nullptr), ok(true) {
            if (a->in_chain.exchange(1)) { ok = false; a = nullptr; b = nullptr; return; }
            if (b && b->in_chain.exchange(1)) { ok = false; a->in_chain.store(0); a = nullptr; b = nullptr; }
        }
        ~Busy() { if (a) a->in_chain.store(0); if (b) b->in_chain.store(0); }
    } busy(pair, uncond);
    if (!busy.ok) return fail("this U-Net handle is already inside a sampling chain on another thread: concurrent chains need their own handles "
                              "(cindm_unet1d_create per chain; the weights can be shared by loading the same state dict)");
    ChainInFlight inflight;
    h->last_chain_recovered = 0; h->last_chain_crowded = 0; h->last_chain_in_flight = inflight.prev + 1;
    h->last_chain_range = std::max(pair->O("range_fallback"), uncond ? uncond->O("range_fallback") : 0);
    // (already exchange-free: nothing can time out, nothing to keep -- BOTH models of a multibody step count)
    const bool guard = !pair->NX() || (uncond && !uncond->NX());
    if (guard && inflight.prev > 0) {
        h->last_chain_crowded = 1;
        const int f0 = pair->no_xchg_force, f1 = uncond ? uncond->no_xchg_force : 0;
        pair->no_xchg_force = 1; if (uncond) uncond->no_xchg_force = 1;
        h->drop_graph();
        const int rc = body();
        pair->no_xchg_force = f0; if (uncond) uncond->no_xchg_force = f1;
        h->drop_graph();
        if (rc == 1) return fail("an in-kernel exchange timed out in exchange-free mode (internal error)");
        return rc;
    }
    if (guard) HIPCHK(hipMemcpyAsync(ch.xT(), x, bytes, hipMemcpyDeviceToDevice, stream));
    int rc = body();
    if (rc != 1) return rc;
    if (!guard) return fail("an in-kernel exchange timed out in exchange-free mode (internal error)");
    if (!pair->O("recover") || (uncond && !uncond->O("recover")))
        return fail("an in-kernel exchange between workgroups timed out (foreign load on the device kept a partner workgroup from becoming "
                    "resident); option recover = 0: the chain is not re-run");
    if (h->ms && h->ms->kappa[0] != 0.f)
        return fail("an in-kernel exchange between workgroups timed out, and the chain's first step reads a multistep history that the run "
                    "has overwritten: restore the history and call again");
    HIPCHK(hipMemcpyAsync(x, ch.xT(), bytes, hipMemcpyDeviceToDevice, stream));
    pair->no_xchg_force = 1; ++pair->recovered;
    if (uncond) { uncond->no_xchg_force = 1; ++uncond->recovered; }
    h->last_chain_recovered = 1;
    h->drop_graph();
    rc = body();
    pair->no_xchg_force = 0;
    if (uncond) uncond->no_xchg_force = 0;
    h->drop_graph();
    if (rc == 1) return fail("an in-kernel exchange timed out again during the exchange-free re-run (internal error)");
    return rc;
}

// what the last chain of this handle did: info[0] = 1 when it was re-run on the exchange-free plan after a time-out, info[1] = 1 when
// it ran on the exchange-free plan from the start because another chain was in flight on the device, info[2] = chains in flight on
// the device when it started (itself included), info[3] = the models' "range_fallback" when it ran (0 = the split-fp16 kernels; 1 / 2 / 3 =
// the exact fp32-MFMA kernels because a weight / the calibration batch / the caller's own batch left the split-fp16 window)
extern "C" int cindm_ddpm1d_last_chain_info(const cindm_ddpm1d* h, int32_t info[4]) {
    REQUIRE(h && info, "null argument");
    info[0] = h->last_chain_recovered; info[1] = h->last_chain_crowded; info[2] = h->last_chain_in_flight; info[3] = h->last_chain_range;
    return 0;
}

static void key_common(KeyBuilder& K, int kind, const Chain1D& ch, const StepIO& io) {
    const cindm_unet1d* pair = ch.pair; const cindm_unet1d* uncond = ch.uncond;
    K(kind)(pair)(pair->generation)(uncond)(uncond ? uncond->generation : 0)(*ch.c)(ch.B)(ch.ws)(ch.ws_bytes)(pair->NX())(uncond ? uncond->NX() : false);
    K(io.x)(io.cond)(io.x_out)(io.noise)(io.noise_t_stride)(io.add_noise)(io.inp_cond)(io.inp_steps)(io.inp_noise)(io.inp_noise_t_stride);
    K(io.ddim_tab)(io.ddim_tnext)(io.iso)(io.iso_steps)(io.recur_t_stride);
    K(io.rec)(io.x0_out);      // recorder on, which streams; the x0 stream's staging record is an operand of the captured update
    if (io.tc) K(io.tc->cond_buf)(io.tc->seeds)(io.tc->Bseg)(io.tc->n_seg);      // (nothing set: the key is what it was)
    if (io.kn && ch.h->kn1) {  // known region: everything the captured node embeds (nothing armed: the key is what it was)
        const Known1D& k = *ch.h->kn1;
        K(io.kn)(k.known)(k.mask)(k.known_per_design)(k.mask_per_design)(k.z_step)(k.step_stride)(k.z_recur)(k.recur_stride);
    }
    if (io.ms_hist) ms_key(K, ch.h);      // multistep solver: the history is an operand of the captured update
}

// the StepIO fields every sample loop sets the same way: in-place state, per-step tapes (or the counter noise keyed in device
// memory), inpainting.  What a loop adds -- DDIM tables, the design objective -- it sets itself; loop_steps sets dec_t and pingpong.
static StepIO chain_io(const Chain1D& ch, float* x, const float* cond, const float* noise_steps, uint64_t seed, int64_t sample_offset,
                       const float* inpaint_cond, int32_t inpaint_steps, const float* inpaint_noise_steps) {
    StepIO io{};
    io.x = x; io.cond = cond; io.x_out = x;
    io.noise = noise_steps; io.noise_t_stride = ch.n_state(); io.seed = seed; io.sample_off = sample_offset; io.add_noise = 1;
    io.inp_cond = inpaint_cond; io.inp_steps = inpaint_steps; io.inp_noise = inpaint_noise_steps;
    io.inp_noise_t_stride = ch.B * inpaint_steps * ch.c->n_bodies * 4;
    io.dyn = reinterpret_cast<const unsigned long long*>(ch.h->t_dev + 16);
    if (ch.h->rec) { io.rec = ch.h->rec->streams; io.x0_out = ch.h->rec->x0_stage; }      // (x0_out set: the update is not fused)
    io.kn = ch.h->kn1 ? 1 : 0;
    return io;
}

// The DDIM preamble: the per-step tables go to their slice of the caller's workspace (step_layout's off_ddim holds 5 words per U-Net
// timestep: chain1_refuse has bounded n_steps by that) and io reads them from there.
static int ddim_tables1(const Chain1D& ch, const Ddim1Call& dd, StepIO& io) {
    int* tn_dev = nullptr;
    // (a chain that took the multistep solver: kappa rides in the rows' fourth word, which is free in 1-D)
    const Multistep* ms = ch.h->ms;
    if (upload_ddim_tables(ch.h->T, dd.n_steps, dd.times, dd.coefs, ch.ddim_tab(), ch.stream, &tn_dev, ms ? ms->kappa.data() : nullptr) != 0) return -1;
    io.ddim_tab = ch.ddim_tab(); io.ddim_tnext = tn_dev; io.ms_hist = ms ? ms->hist : nullptr;
    return 0;
}

// One unguided loop inside a chain body: start at t0 with (seed, sample_offset) in the device counter, then replay the step
// nsteps times.  The step decrements the counter; with option "pingpong" the step state lives in two slots and the step's own
// update advances it (no step_counter_kernel launch, and a plain single-model step runs its update inside the last U-Net kernel).
// kind: 0 DDPM, 1 DDIM and the rollout's segments (whose keys are equal, so that one graph serves them all), 3 Langevin (2: the guided loop,
// 4: the guided DDIM loop).
static int loop_steps(const Chain1D& ch, StepIO io, int kind, int t0, int nsteps, uint64_t seed, int64_t sample_offset) {
    const bool pp = ch.pair->O("pingpong") != 0;
    io.dec_t = 1; io.pingpong = pp ? 1 : 0;
    start_loop(ch, t0, seed, sample_offset);
    rec_arm(ch.h, io.ddim_tab ? -1 : t0, io.ddim_tab ? 2 : 0, pp ? 4 : 0, ch.stream);
    // (rule 1 of a known region, at the level set_counter_kernel has just written to slot 0; a recovery re-run starts from it again)
    if (io.kn && ch.h->kn1 && ch.h->kn1->apply_init && known1_node(ch, io, io.x_out, ch.h->t_dev, 1, 0) != 0) return -1;
    KeyBuilder K;
    key_common(K, kind, ch, io);
    K(pp)(io.ula_tab)(io.ula_L)(io.ula_t_hi);
    return replay_steps(ch, K.k, nsteps, [&](int q) { StepIO it = io; it.parity = q; return run_step(ch, it, 0, ch.h->t_dev); }, pp);
}

// the chain that is one such loop (DDPM, DDIM, Langevin) from the (seed, sample_off) of its io: what a recovery re-run repeats
static int loop_chain(ChainArmed& took, const Chain1D& ch, const StepIO& io, int kind, int t0, int nsteps) {
    return rec_done(took, run_chain_with_recovery(ch, io.x_out, [&]() -> int {
        if (prepare_step_ws(ch) != 0) return -1;
        return loop_steps(ch, io, kind, t0, nsteps, io.seed, io.sample_off);
    }));
}

// One guided step: `iters` iterations of run_step, [p_mean_variance, mean - grad, overwrite, relaxation] (:1286-1370).  All but the
// last relax (x <- a_t (mean - g | overwrite) + b_t z', drawn from the recurrence tape or under the iteration's tag) and are not
// steps: they do not record.  The last iteration's relaxation is never used by the reference; its result is the step's.
// buf null (guided DDPM): in-place state through the staging slice, the last iteration decrements the device counter.
// buf (guided DDIM): iteration k of the CHAIN reads buf[k & 1] and writes the other, and the step state alternates between its two
// slots with it; q is the step's parity inside the captured pair -- after two steps (2 iters iterations) both parities are 0 again.
static int guided_step(const Chain1D& ch, const StepIO& io, int iters, const float* recur_noise_steps, float* const* buf, int q) {
    for (int r = 0; r < iters; ++r) {
        StepIO it = io;
        it.relax = (r < iters - 1) ? 1 : 0;
        if (it.relax) it.rec = 0;
        it.recur_noise = recur_noise_steps ? recur_noise_steps + (size_t)r * ch.n_state() : nullptr;
        it.recur_tag = 0x10000u * (uint32_t)(r + 1);
        it.relax_idx = r;
        if (buf) { const int p = (q * iters + r) & 1; it.parity = p; it.x = buf[p]; it.x_out = buf[1 - p]; }
        else it.dec_t = it.relax ? 0 : 1;
        if (run_step(ch, it, 0, ch.h->t_dev) != 0) return -1;
    }
    return 0;
}

// The tail of the two guided entries, on the io they have completed: kind 2 (DDPM: max(R, 1) iterations per step, from timestep t0)
// or 4 (DDIM: R iterations per step, ping-pong between the caller's x and x2, the workspace's second state buffer; the record word
// is the step index).  The key carries the objective, its tables and the recurrence tape; after() runs behind a chain that ended well.
template <typename After>
static int guided_chain(ChainArmed& took, const Chain1D& ch, StepIO io, int kind, const float* recur_noise_steps, int t0, int nsteps, float* x2, After after) {
    const bool pp = x2 != nullptr;
    const int R = io.dz->recurrence, iters = pp ? R : std::max(R, 1);
    float* const buf[2] = {io.x_out, x2};
    io.recur_t_stride = (int64_t)iters * ch.n_state();
    io.pingpong = pp ? 1 : 0; io.state_pp = pp ? 1 : 0;
    auto step = [&](int q) -> int { return guided_step(ch, io, iters, recur_noise_steps, pp ? buf : nullptr, q); };
    return rec_done(took, run_chain_with_recovery(ch, io.x_out, [&]() -> int {
        if (prepare_step_ws(ch) != 0) return -1;
        start_loop(ch, t0, io.seed, io.sample_off);
        rec_arm(ch.h, pp ? -1 : t0, pp ? 2 : 0, pp ? 4 : 0, ch.stream);
        if (io.kn && ch.h->kn1 && ch.h->kn1->apply_init && known1_node(ch, io, io.x_out, ch.h->t_dev, 1, 0) != 0) return -1;      // (rule 1)
        KeyBuilder K;
        key_common(K, kind, ch, io);
        K(*io.dz)(recur_noise_steps)(R);
        design_key(K, ch.h);
        const int rc = replay_steps(ch, K.k, nsteps, step, pp);
        return rc == 0 ? after() : rc;
    }));
}

// the objective and the overwritten rows of a guided chain's io
static void guided_io(StepIO& io, const cindm_design_desc* dz, const float* initial_state_overwrite, int overwrite_steps) {
    io.dz = dz; io.iso = initial_state_overwrite; io.iso_steps = initial_state_overwrite ? overwrite_steps : 0;
}

extern "C" int cindm_ddpm1d_sample(cindm_ddpm1d* h, cindm_unet1d* pair, cindm_unet1d* uncond, const cindm_compose_desc* c,
                                   float* x, const float* cond, const float* noise_steps, uint64_t seed, int64_t sample_offset,
                                   const float* inpaint_cond, int32_t inpaint_steps, const float* inpaint_noise_steps,
                                   int32_t t_start, int32_t t_end, int64_t B, void* ws, size_t ws_bytes, void* stream_,
                                   int32_t use_graph) {
    ChainArmed took(h);
    Chain1D ch(h, pair, uncond, c, B, ws, ws_bytes, nullptr, use_graph);
    const int nsteps = t_start - t_end + 1;
    if (took.refuse_all_but(kServesKnown1) != 0 || chain1_refuse(ch, x, cond, nullptr, t_start, t_end) != 0) return -1;
    if (rec_begin(took, x, nsteps, ch.n_state()) != 0 || known1_begin(took, ch, x, 0) != 0) return -1;
    if (chain_stream(h, stream_, use_graph, &ch.stream) != 0) return -1;
    const StepIO io = chain_io(ch, x, cond, noise_steps, seed, sample_offset, inpaint_cond, inpaint_steps, inpaint_noise_steps);
    return loop_chain(took, ch, io, 0, (int)t_start, nsteps);
}

extern "C" int cindm_ddpm1d_sample_ddim(cindm_ddpm1d* h, cindm_unet1d* pair, cindm_unet1d* uncond, const cindm_compose_desc* c,
                                        float* x, const float* cond, int32_t n_steps, const int32_t* times,
                                        const float* coefs, const float* noise_steps, uint64_t seed, int64_t sample_offset,
                                        const float* inpaint_cond, int32_t inpaint_steps, const float* inpaint_noise_steps,
                                        int64_t B, void* ws, size_t ws_bytes, void* stream_, int32_t use_graph) {
    ChainArmed took(h);
    Chain1D ch(h, pair, uncond, c, B, ws, ws_bytes, nullptr, use_graph);
    const Ddim1Call dd{n_steps, times, coefs};
    if (took.refuse_all_but(kServesKnown1 | kServesMultistep) != 0 || chain1_refuse(ch, x, cond, &dd) != 0) return -1;
    if (took.rec.on()) REQUIRE(n_steps >= 1, "n_steps must be >= 1");
    if (rec_begin(took, x, n_steps, ch.n_state()) != 0 || known1_begin(took, ch, x, 0) != 0 || ms_begin(took, n_steps, coefs, ch.n_state(), x) != 0) return -1;
    if (chain_stream(h, stream_, use_graph, &ch.stream) != 0) return -1;
    StepIO io = chain_io(ch, x, cond, noise_steps, seed, sample_offset, inpaint_cond, inpaint_steps, inpaint_noise_steps);
    if (ddim_tables1(ch, dd, io) != 0) return -1;
    return loop_chain(took, ch, io, 1, (int)times[0], n_steps);
}

// Autoregressive time composition (autoregress_time_compose_sample, model/diffusion_1d.py:2240-2327): n_seg unguided DDIM chains, each
// from a fresh x_T and conditioned on the last Lc rows of the previous one.  The whole rollout is ONE chain for the recovery and the
// in-flight registry: its body draws segment 0's x_T and copies the caller's cond into cond_buf itself, so it is a pure function of
// its inputs and a time-out re-runs all of it once on the exchange-free kernels.  Per segment: loop_steps with that segment's seed
// (io.cond = cond_buf: a fixed address, and the seed lives in the device counter -- one captured graph serves every segment), then
// autoregress_handover_kernel (out slice, next cond, next x_T).
extern "C" int cindm_ddpm1d_sample_autoregress(cindm_ddpm1d* h, cindm_unet1d* pair, cindm_unet1d* uncond, const cindm_compose_desc* c,
                                               float* x, const float* cond, float* cond_buf, float* out, int32_t n_seg,
                                               int32_t n_steps, const int32_t* times, const float* coefs, const uint64_t* seeds,
                                               const float* init_tape, const float* noise_steps, int64_t sample_offset, int64_t B,
                                               void* ws, size_t ws_bytes, void* stream_, int32_t use_graph) {
    ChainArmed took(h);
    Chain1D ch(h, pair, uncond, c, B, ws, ws_bytes, nullptr, use_graph);
    const Ddim1Call dd{n_steps, times, coefs};
    if (took.refuse_all_but(0, "the autoregressive rollout draws a fresh state per segment and hands rows over between segments: a region of "
                               "one [B, rows, F] state does not name a place in it") != 0) return -1;
    REQUIRE(!took.rec.on(), "recorder: the autoregressive rollout is not recorded (its step index is (segment, step)); the recorder was dropped");
    REQUIRE(h && pair && c && x && cond && cond_buf && out && times && coefs && seeds, "null argument");
    REQUIRE(c->mode == CINDM_COMPOSE_PLAIN || c->mode == CINDM_COMPOSE_MULTIBODY, "the rollout runs the plain (or multibody) prediction");
    REQUIRE(c->cond_steps >= 1, "conditioned_steps == 0: the reference's img[:, -0:] hands over the whole state and its slice assignment fails");
    REQUIRE(n_seg >= 1, "n_seg must be >= 1");
    const int R = state_len(pair, c), Lc = c->cond_steps, F = c->n_bodies * 4;
    REQUIRE(R >= Lc, "rollout_steps < conditioned_steps: the next segment's condition would be shorter than the model's horizon needs");
    for (const void* p : {(const void*)x, (const void*)cond_buf, (const void*)out, (const void*)init_tape})
        REQUIRE(((uintptr_t)p & 15) == 0, "x, cond_buf, out and init_tape must be 16-byte aligned");
    if (chain1_refuse(ch, x, cond_buf, &dd) != 0) return -1;
    if (chain_stream(h, stream_, use_graph, &ch.stream) != 0) return -1;
    const int64_t n_state = ch.n_state();
    // (the seed differs per segment and goes to the device counter; the tape per segment below; no inpainting)
    StepIO io = chain_io(ch, x, cond_buf, nullptr, 0, 0, nullptr, 0, nullptr);
    if (ddim_tables1(ch, dd, io) != 0) return -1;
    const unsigned hblocks = (unsigned)((n_state / 4 + 255) / 256);
    hipStream_t stream = ch.stream;
    return run_chain_with_recovery(ch, x, [&]() -> int {
        if (prepare_step_ws(ch) != 0) return -1;
        if (init_tape) HIPCHK(hipMemcpyAsync(x, init_tape, (size_t)n_state * sizeof(float), hipMemcpyDeviceToDevice, stream));
        else hipLaunchKernelGGL(fill_normal_kernel, dim3((unsigned)((n_state + 255) / 256)), dim3(256), 0, stream,
                                x, B, (int64_t)R * F, seeds[0], sample_offset, (uint32_t)h->T);
        HIPCHK(hipMemcpyAsync(cond_buf, cond, (size_t)B * Lc * F * sizeof(float), hipMemcpyDeviceToDevice, stream));
        for (int k = 0; k < n_seg; ++k) {
            StepIO seg = io;
            seg.noise = noise_steps ? noise_steps + (size_t)k * n_steps * n_state : nullptr;      // (a tape re-captures per segment)
            const int rc = loop_steps(ch, seg, 1, (int)times[0], n_steps, seeds[k], sample_offset);
            if (rc != 0) return rc;
            const int has_next = k + 1 < n_seg;
            hipLaunchKernelGGL(autoregress_handover_kernel, dim3(hblocks), dim3(256), 0, stream, x, out, cond_buf,
                               (has_next && init_tape) ? init_tape + (size_t)(k + 1) * n_state : (const float*)nullptr,
                               B, R, F, Lc, k, (int)n_seg, has_next, has_next ? seeds[k + 1] : (uint64_t)0, sample_offset, (uint32_t)h->T);
            HIPCHK(hipGetLastError());
        }
        return 0;
    });
}

// Langevin (ULA) phase of sample_compose_multibodies (model/diffusion_1d.py:2002-2022, sample_step_ULA :2048-2073): for
// t = t_start .. t_end, L iterations of x <- x + (-scalar_t eps(x, t)) ss_t + std_t z on the WHOLE state (c->cond_steps == 0: the
// conditioning rows are rows of x and move with it).  One iteration = one step of the chain driver (gather, both U-Nets,
// ula_update_kernel); the step state (t, inner index) advances on the device, the timestep once per L iterations, so the
// captured iteration is replayed (t_start - t_end + 1) * L times with no host code in between.
extern "C" int cindm_ddpm1d_sample_ula(cindm_ddpm1d* h, cindm_unet1d* pair, cindm_unet1d* uncond, const cindm_compose_desc* c,
                                       float* x, int32_t t_start, int32_t t_end, int32_t L, const float* scalar,
                                       const float* step_size, const float* noise_std, void* tab, size_t tab_bytes,
                                       const float* noise_tape, uint64_t seed, int64_t sample_offset, int64_t B,
                                       void* ws, size_t ws_bytes, void* stream_, int32_t use_graph) {
    ChainArmed took(h);
    Chain1D ch(h, pair, uncond, c, B, ws, ws_bytes, nullptr, use_graph);
    if (took.refuse_all_but(0, "the Langevin chain moves the whole state, conditioning rows included, at one noise level per timestep without a "
                               "reverse update: the region's forward-diffusion trajectory is not defined for it") != 0) return -1;
    REQUIRE(!took.rec.on(), "recorder: the Langevin chain is not recorded (its step index is (timestep, inner iteration)); the recorder was dropped");
    REQUIRE(h && pair && c && x && scalar && step_size && noise_std && tab, "null argument");
    REQUIRE(c->mode == CINDM_COMPOSE_MULTIBODY && uncond, "the Langevin phase runs the multibody composition (pair + unconditioned model)");
    REQUIRE(c->cond_steps == 0, "the Langevin phase moves the whole state: pass cat(cond, x) as x with cond_steps = 0");
    REQUIRE(c->objective == CINDM_OBJ_PRED_NOISE, "the Langevin score is the composed noise prediction (objective pred_noise)");
    // (the range ahead of chain1_refuse's: the table's size is stated in it, and a call with L == 0 is refused or returns before the step's checks)
    REQUIRE(t_start < h->T && t_end >= 0 && t_end <= t_start, "bad timestep range");
    REQUIRE(L >= 0 && L <= 32767 && h->T <= 65536, "L must be in 0 .. 32767 (and timesteps <= 65536): the noise key packs (l, t) into one word");
    const int n_t = t_start - t_end + 1;
    REQUIRE(tab_bytes >= (size_t)n_t * 4 * sizeof(float), "tab too small: (t_start - t_end + 1) * 16 bytes");
    for (const void* p : {(const void*)x, (const void*)tab, (const void*)noise_tape})
        REQUIRE(((uintptr_t)p & 15) == 0, "x, tab and noise_tape must be 16-byte aligned");
    if (L == 0) return 0;
    if (chain1_refuse(ch, x, nullptr, nullptr, t_start, t_end) != 0) return -1;
    if (chain_stream(h, stream_, use_graph, &ch.stream) != 0) return -1;
    {
        std::vector<float> tabv((size_t)n_t * 4, 0.f);
        for (int j = 0; j < n_t; ++j) { tabv[4 * j] = scalar[j]; tabv[4 * j + 1] = step_size[j]; tabv[4 * j + 2] = noise_std[j]; }
        HIPCHK(hipMemcpyAsync(tab, tabv.data(), tabv.size() * sizeof(float), hipMemcpyHostToDevice, ch.stream));
        HIPCHK(hipStreamSynchronize(ch.stream));            // the host vector goes out of scope
    }
    StepIO io = chain_io(ch, x, nullptr, noise_tape, seed, sample_offset, nullptr, 0, nullptr);
    io.ula_tab = reinterpret_cast<const float*>(tab); io.ula_L = L; io.ula_t_hi = t_start;
    return loop_chain(took, ch, io, 3, (int)t_start, n_t * L);
}

extern "C" int cindm_ddpm1d_sample_guided(cindm_ddpm1d* h, cindm_unet1d* pair, cindm_unet1d* uncond, const cindm_compose_desc* c,
                                          const cindm_design_desc* dz, float* x, const float* cond, const float* noise_steps,
                                          const float* recur_noise_steps, uint64_t seed, int64_t sample_offset,
                                          const float* inpaint_cond, int32_t inpaint_steps, const float* inpaint_noise_steps,
                                          const float* initial_state_overwrite, int32_t overwrite_steps,
                                          int32_t t_start, int32_t t_end, int64_t B, void* ws, size_t ws_bytes, void* stream_,
                                          int32_t use_graph) {
    ChainArmed took(h);
    Chain1D ch(h, pair, uncond, c, B, ws, ws_bytes, nullptr, use_graph);
    const int nsteps = t_start - t_end + 1;
    if (took.refuse_all_but(kServesTables | kServesKnown1) != 0 || chain1_refuse(ch, x, cond, nullptr, t_start, t_end) != 0 ||
        guided_refuse(ch, took, dz, x, 0, initial_state_overwrite, overwrite_steps) != 0) return -1;
    if (rec_begin(took, x, nsteps, ch.n_state()) != 0 || known1_begin(took, ch, x, std::max(dz->recurrence, 1)) != 0) return -1;
    if (chain_stream(h, stream_, use_graph, &ch.stream) != 0) return -1;
    StepIO io = chain_io(ch, x, cond, noise_steps, seed, sample_offset, inpaint_cond, inpaint_steps, inpaint_noise_steps);
    guided_io(io, dz, initial_state_overwrite, overwrite_steps);
    return guided_chain(took, ch, io, 2, recur_noise_steps, (int)t_start, nsteps, nullptr, []() -> int { return 0; });
}

// Guided DDIM (ddim_sample :1724-1804 with design_fn = the built-in objective and "-recurrence-N" guidance, i.e. through the DDIM
// return of p_sample_compose_inside :1284-1376).  One DDIM step = R iterations of [U-Net(s), one compose_update_kernel launch]:
// iterations 0 .. R-2 relax (x <- a_t (mean - g | overwrite) + b_t z'), iteration R-1 is the DDIM update on (eps + g, x_start).
// The gradient reads neighbours of its input, so the state alternates between the caller's x and one workspace slice (the guided
// DDPM step's staging slice, unused here): iteration k of the chain reads buffer k & 1 and writes the other -- no staging copy.
// The step state (t, step index, exchange epochs) alternates between its two slots per ITERATION as well, written by the update
// itself (compose_advance: a relaxation iteration hands t and the step index on unchanged), so there is no counter launch either.
// A graph holds two steps (2 R iterations: both parities return to 0); when n_steps * R is odd the result is copied to x once, after the chain.
extern "C" int cindm_ddpm1d_sample_ddim_guided(cindm_ddpm1d* h, cindm_unet1d* pair, cindm_unet1d* uncond, const cindm_compose_desc* c,
                                               const cindm_design_desc* dz, float* x, const float* cond, int32_t n_steps,
                                               const int32_t* times, const float* coefs, const float* noise_steps,
                                               const float* recur_noise_steps, uint64_t seed, int64_t sample_offset,
                                               const float* inpaint_cond, int32_t inpaint_steps, const float* inpaint_noise_steps,
                                               const float* initial_state_overwrite, int32_t overwrite_steps, int64_t B,
                                               void* ws, size_t ws_bytes, void* stream_, int32_t use_graph) {
    ChainArmed took(h);
    Chain1D ch(h, pair, uncond, c, B, ws, ws_bytes, nullptr, use_graph);
    const Ddim1Call dd{n_steps, times, coefs};
    if (took.refuse_all_but(kServesTables | kServesKnown1 | kServesMultistep) != 0 || chain1_refuse(ch, x, cond, &dd) != 0 ||
        guided_refuse(ch, took, dz, x, 1, initial_state_overwrite, overwrite_steps) != 0) return -1;
    REQUIRE(!inpaint_cond || (inpaint_steps >= 1 && inpaint_steps <= ch.Ltot()), "bad inpaint_steps");
    if (took.rec.on()) REQUIRE(n_steps >= 1, "n_steps must be >= 1");
    if (rec_begin(took, x, n_steps, ch.n_state()) != 0 || known1_begin(took, ch, x, dz->recurrence) != 0 ||
        ms_begin(took, n_steps, coefs, ch.n_state(), x, ch.stage()) != 0) return -1;
    if (chain_stream(h, stream_, use_graph, &ch.stream) != 0) return -1;
    StepIO io = chain_io(ch, x, cond, noise_steps, seed, sample_offset, inpaint_cond, inpaint_steps, inpaint_noise_steps);
    if (ddim_tables1(ch, dd, io) != 0) return -1;
    guided_io(io, dz, initial_state_overwrite, overwrite_steps);
    float* x2 = ch.stage();
    return guided_chain(took, ch, io, 4, recur_noise_steps, (int)times[0], n_steps, x2, [&]() -> int {
        if (((int64_t)n_steps * dz->recurrence) & 1) {        // the last iteration wrote the workspace buffer
            HIPCHK(hipMemcpyAsync(x, x2, (size_t)ch.n_state() * sizeof(float), hipMemcpyDeviceToDevice, ch.stream));
            if (use_graph) HIPCHK(hipStreamSynchronize(ch.stream));
        }
        return 0;
    });
}

extern "C" int cindm_fill_normal(float* out, int64_t B, int64_t per_sample, uint64_t seed, int64_t sample_offset,
                                 int32_t step_tag, void* stream) {
    REQUIRE(out && B > 0 && per_sample > 0, "bad argument");
    const int64_t n = B * per_sample;
    hipLaunchKernelGGL(fill_normal_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       out, B, per_sample, seed, sample_offset, (uint32_t)step_tag);
    HIPCHK(hipGetLastError());
    return 0;
}
