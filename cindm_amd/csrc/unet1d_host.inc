// Host side of TemporalUnet1D (included by cindm_hip.hip): the handle, its manifest and options, the weight packers, the launch
// emitter and the forward it emits (model/diffusion_1d.py:610-646 of the reference) out of the kernels in kernels.h and
// kernels_dconv.h, the plan, finalize, the workspace size, and the forward / profile / tap entry points.

struct Packed { size_t off = 0; size_t sz = 0; int T = 0, CinP = 0, Npad = 0, N = 0, KC = 32; size_t bias_off = 0; bool has_bias = false; bool h3 = false; };

struct RtbDesc { std::string p; int cin, cout; int tb_off; };

// One sample-local level kernel (level0_down, level1_down, ups_last, ups_tail128) as data: the "#lvl" fragments it consists of, in
// the order pack_level0 packs them (the blob layout) and each with the role that names its member of the kernel's argument
// struct; its attention site; the ResidualTemporalBlocks whose ttable columns it reads.  level_specs() states the four kernels
// (the ups.* prefixes depend on n_mults) and pack_level0 resolves them once per pack: the packer, the L2 warm-up registration
// (Emitter::pf_level) and the argument fill (level_args) read this one description, and an emission looks up no key.
enum FragRole { FRAG_CONV, FRAG_RES, FRAG_RESAMPLE, FRAG_HEAD };     // Wc[] in order; Wr | Wr0, Wr1; Wd | Wu; Wf
struct LevelFrag {
    FragRole role; std::string p; int want_co; int kind;      // module prefix; pack_level_frag's want_co; 0 Conv1d, 1 ConvTranspose1d
    const Packed* w = nullptr; const Packed* b = nullptr;     // resolved: p + "#lvl" (the fragments), p (its bias)
    size_t gam = 0, bet = 0;                                   // FRAG_CONV: the Conv1dBlock's GroupNorm vectors (vec_off)
};
struct LevelSpec {
    std::string label;                     // the launch's name for the phase clocks
    bool fits = false;                     // the level has the widths the kernel is written for (decided before anything is packed)
    bool allowed = false;                  // ... and nothing the kernel leaves out (an identity second block, F within its tile)
    std::vector<LevelFrag> frags;
    std::string attn;                      // attention site, e.g. "downs.0.2"
    std::vector<std::string> rtb;          // the blocks whose time-bias columns the kernel reads (tb0, tb1 | tb)
    bool ok = false;                       // every fragment packed, the site exists: the kernel's operands are in the blob
    const Packed *qkv = nullptr, *wo = nullptr, *bo = nullptr;      // resolved: to_qkv#site, to_out#site (nullptr: no fused site), to_out
    size_t ln_g = 0; int tb[2] = {0, 0};
    Packed span;                           // resolved: the blob range of the fragments (off, sz)
    // the i-th fragment of a role (level_specs gives every kernel the roles its emitter asks for)
    const LevelFrag& frag(FragRole r, int i = 0) const { size_t k = 0; while (frags[k].role != r || i-- > 0) ++k; return frags[k]; }
};
enum { LV_LEVEL0, LV_LEVEL1, LV_UPS_LAST, LV_UPS_TAIL, LV_COUNT };      // (pack order)

struct cindm_unet1d : ModelCore {
    const cindm::ComposeArgs* fuse_upd = nullptr;   // set by run_step around one forward: ups_last_kernel also runs this update
    bool fused_done = false;                          // ... and reports here that it did
    int issued = 0;                                   // kernels the last cindm_unet1d_forward actually launched (the plan's `launches` counts the epoch
                                                      // launch of a bare forward, which a sample loop's step does not issue: its predecessor advanced the epoch)
    int gatherB = 0, gather_cs = 0, gather_Ltot = 0;  // set by run_step around one forward: x is the sampler's state, level0_down_kernel reads its windows in place
    cindm_unet1d_desc d;
    std::vector<int> dims;                 // [F, dim*m0, ...]
    int n_plain = 1;                       // number of trailing levels without down-sampling (:550-555)
    // device
    float* blob = nullptr;                 // packed weights / biases / norm vectors
    size_t blob_floats = 0;
    std::unordered_map<std::string, Packed> packed;     // conv / linear weights by module prefix
    std::unordered_map<std::string, size_t> vec_off;    // norm vectors by full key
    float* ttable = nullptr;               // [T, tb_ld] per-timestep, per-RTB bias (Mish->Linear of temb)
    int tb_ld = 0;
    std::unordered_map<std::string, int> tb_off;        // RTB prefix -> column offset
    bool use_h3 = true;                    // k=5 convolutions on the fp16 matrix cores (3-term split); CINDM_MFMA=f32 disables
    LevelSpec lvl[LV_COUNT];               // the level kernels; lvl[k].ok: operands packed (level0: dim 64, F <= 32, attention, down-sampling;
                                           // level1: 64 -> 128; ups_last: the finest up level + head; ups_tail: the second half of the level above it)
    int launches = 0;
    struct WReg { size_t off[PF_REGIONS]; unsigned bytes[PF_REGIONS]; unsigned stride[PF_REGIONS]; };      // byte offsets into blob
    std::vector<WReg> pf_table;            // per launch of one forward: the weights it streams (L2 warm-up of its predecessor)
    int* epoch_dev = nullptr;              // [0] per-forward epoch (tag of the pair exchanges), [1] error flag, [2] prefetch sink, [8] second epoch slot
    int epoch_slot = 0;                    // which epoch slot (0 / 8) the forward being emitted reads (ping-pong sample loop)
    const int* ep() const { return epoch_dev + epoch_slot; }
    const void* seen_ws = nullptr; int64_t seen_rows = 0;   // workspace whose exchange regions have been cleared
    int generation = 0;                    // bumped by every (re)pack: captured graphs that embed this handle's pointers check it
    std::atomic<int> in_chain{0};          // 1 while a sampling chain runs on this handle (run_chain_with_recovery mutates its plan switches: one chain at a time)
    bool force_f32 = false;                // calibration forward overflowed on the split-fp16 kernels: fp32 MFMA kernels in use
    int force_reason = 0;                  // what "range_fallback" reads then: 2 = the synthetic calibration batch, 3 = the caller's own batch (cindm_unet1d_range_escalate)
    bool epoch_prebumped = false;          // the sample loop's counter kernel has already advanced the epoch for the next forward
    // Exchange-free mode (run-time option "no_exchange", or forced for the re-run of a chain whose exchange timed out): the
    // kernels that hand data between WORKGROUPS inside a launch (dconv / dconv2 at C = 512 and the y0 all-gather, attn1d_head)
    // are not emitted; their per-layer / one-workgroup counterparts run instead.  Nothing in that mode can time out.
    int no_xchg_force = 0;
    int recovered = 0;                     // chains / forwards re-run in exchange-free mode after a time-out (cindm_unet1d_recovered)
    bool NX() const { return no_xchg_force || O("no_exchange"); }
    // cindm_unet1d_workspace_bytes' cache (one entry: a sampling loop asks for the same row count over and over)
    mutable std::mutex wsb_mu; int wsb_gen = -1, wsb_nx = -1; int64_t wsb_rows = -1; size_t wsb_val = 0;
    int plan_nx = -1;                      // the mode h->launches / pf_table were planned for
    // phase clocks (profiling builds): [slot][PH_MAXWG][PH_MAXWAVE][PH_NST] uint64, armed by cindm_unet1d_phase_prof_enable
    unsigned long long* ph_buf = nullptr; int ph_on = 0;
    std::vector<std::string> ph_names;     // kernel of each launch slot of the last emitted forward
    // taps of the last forward
    struct Tap { size_t off; int L, C, ld; };
    std::unordered_map<std::string, Tap> taps;
    int64_t taps_rows = 0;
};

// State-dict manifest in the reference's registration order (time_mlp, downs, ups, mid_*, final_conv).
static int build_manifest(cindm_unet1d* h) {
    const auto& d = h->d;
    const int dim = d.dim;
    h->dims.clear();
    h->dims.push_back(d.transition_dim);
    for (int i = 0; i < d.n_mults; ++i) h->dims.push_back(dim * d.dim_mults[i]);
    const int nres = d.n_mults;
    if (d.horizon % 8 == 0) h->n_plain = 1;
    else if (d.horizon % 4 == 0) h->n_plain = 2;
    else if (d.horizon % 2 == 0) h->n_plain = 3;
    else return fail("horizon must be even (model/diffusion_1d.py:550-555)");
    auto lin = [&](const std::string& p, int i, int o) { h->add_param(p + ".weight", {o, i}); h->add_param(p + ".bias", {o}); };
    auto conv = [&](const std::string& p, int i, int o, int k) { h->add_param(p + ".weight", {o, i, k}); h->add_param(p + ".bias", {o}); };
    auto cblock = [&](const std::string& p, int i, int o) {
        conv(p + ".block.0", i, o, 5);
        h->add_param(p + ".block.2.weight", {o}); h->add_param(p + ".block.2.bias", {o});
    };
    auto rtb = [&](const std::string& p, int i, int o) {
        cblock(p + ".blocks.0", i, o); cblock(p + ".blocks.1", o, o);
        lin(p + ".time_mlp.1", dim, o);
        if (i != o) conv(p + ".residual_conv", i, o, 1);
    };
    auto attn = [&](const std::string& p, int c) {
        h->add_param(p + ".fn.fn.to_qkv.weight", {384, c, 1});
        conv(p + ".fn.fn.to_out", 128, c, 1);
        h->add_param(p + ".fn.norm.g", {1, c, 1});
    };
    lin("time_mlp.1", dim, dim * 4);
    lin("time_mlp.3", dim * 4, dim);
    for (int ind = 0; ind < nres; ++ind) {
        const int ci = h->dims[ind], co = h->dims[ind + 1];
        const bool is_last = ind >= nres - h->n_plain;
        const std::string p = "downs." + std::to_string(ind);
        rtb(p + ".0", ci, co); rtb(p + ".1", co, co);
        if (d.attention) attn(p + ".2", co);
        if (!is_last) conv(p + ".3.conv", co, co, 3);
    }
    for (int ind = 0; ind < nres - 1; ++ind) {
        const int ci = h->dims[nres - 1 - ind], co = h->dims[nres - ind];   // reversed(in_out[1:])
        const std::string p = "ups." + std::to_string(ind);
        rtb(p + ".0", co * 2, co); rtb(p + ".1", co, ci);
        if (d.attention) attn(p + ".2", ci);
        if (ind >= h->n_plain - 1) { h->add_param(p + ".3.conv.weight", {ci, ci, 4}); h->add_param(p + ".3.conv.bias", {ci}); }
    }
    const int mid = h->dims[nres];
    rtb("mid_block1", mid, mid);
    if (d.attention) attn("mid_attn", mid);
    rtb("mid_block2", mid, mid);
    cblock("final_conv.0", dim, dim);
    conv("final_conv.1", dim, d.transition_dim, 1);
    return 0;
}

// Option keys, defaults, the environment variables that override the defaults at create (ablation scripts) and kinds
// (handle_core.inc): every alternative kernel path is selectable per handle so the parity suite can run each of them in one process.
static const OptDef kUnet1dOpts[] = {
    {"mfma_f32", 0, nullptr, OPT_PACK},          // 1: every product on the exact fp32 MFMA kernels (CINDM_MFMA=f32)
    {"local_gn", 1, "CINDM_LOCAL_GN", OPT_PACK}, // producer-side GroupNorm + Mish, block tails folded into launch B
    {"attn_site", 1, "CINDM_ATTN_SITE", OPT_PACK},   // one launch per attention site
    {"level0", 1, "CINDM_LEVEL0", OPT_PACK},     // level kernels (master switch)
    {"level1", 1, "CINDM_LEVEL1", OPT_PACK},     // level1_down_kernel: samples per workgroup (0 = off, 1, 2)
    {"ups_last", 1, "CINDM_UPS_LAST", OPT_PACK},
    {"ups_tail", 1, "CINDM_UPS_TAIL", OPT_PACK},
    {"level_pairs", 1, "CINDM_LEVEL_PAIRS", OPT_PACK},   // up to 320 rows: level0_down + level1_down and ups_tail128 + ups_last as one launch each (level01_down_kernel, ups_tail_last_kernel)
    {"attn_head", 1, "CINDM_ATTN_HEAD", OPT_PACK},   // deep attention sites with the heads split over workgroups (attn1d_head_kernel)
    {"dconv", 1, "CINDM_DCONV", OPT_PACK},       // deep-level k=5 convolutions on dconv_kernel (LDS-resident activation planes)
    {"ws_alias", 1, "CINDM_WS_ALIAS", OPT_PACK}, // sampling path (taps = 0): dead intermediates' workspace blocks are recycled: 0 never, 1 above 320 rows, 2 always
    {"pingpong", 1, "CINDM_PINGPONG", OPT_PACK}, // plain sample loops: step counter / epochs in two slots advanced by the step's update (no step_counter_kernel launch)
    {"dresample", 2, "CINDM_DRESAMPLE", OPT_PACK},   // the resampling convolutions between the deep levels on dresample_kernel: 2 = 16 columns per workgroup, 1 = 32 (0: conv_gemm_h3_kernel<3 | 4>)
    {"dconv2", 1, "CINDM_DCONV2", OPT_PACK},     // a whole deep-level ResidualTemporalBlock per launch (dconv2_kernel: in-launch all-gather between its convolutions)
    {"l2_prefetch", 1, "CINDM_L2_PREFETCH", OPT_PACK},   // launches touch the next launch's weights (L2 warm-up)
    {"fuse_gather", 1, nullptr, OPT_PACK},       // time composition of two-body states: level0_down_kernel reads the state's windows in place (no compose_gather_kernel launch)
    {"fuse_update", 1, "CINDM_FUSE_UPDATE", OPT_PACK},   // plain single-model steps: the reverse-step update inside ups_last_kernel (no update launch)
    {"taps", 0, "CINDM_TAPS", OPT_PACK},         // 1: the level kernels also store the block outputs that only cindm_unet1d_tap reads
    {"recover", 1, nullptr, OPT_RUNTIME},                   // 0 = a chain whose exchange timed out is an error instead of an exchange-free re-run
    {"no_exchange", 0, "CINDM_NO_EXCHANGE", OPT_RUNTIME},   // 1: only kernels without an in-launch exchange between workgroups
    {"tune", 0, "CINDM_TUNE", OPT_RUNTIME},         // same-box A/B switches (0 = the shipped choices): bit 0 = round 5's L2 warm-up placement, regions and issuers, bit 1 = round 5's plain output stores, bits 2 + i = launch i of the forward issues no warm-up (tools/pf_mask_scan.py)
    {"stress", 0, "CINDM_STRESS", OPT_PACK},     // > 0 (a seed): pseudo-random pauses before the in-kernel hand-overs (dconv pair exchange, attention heads)
    {"auto_range", 1, "CINDM_AUTO_RANGE", OPT_PACK}, // per-layer fall-back to the fp32 MFMA kernels when weights leave the fp16-safe window
    {"range_fallback", 0, nullptr, OPT_READONLY},    // 1 after finalize when a weight left the split-fp16 window: fp32 kernels in use
    {"dbg", 0, "CINDM_DBG", OPT_PACK},           // timing ablations / forced time-outs (wrong results)
};

static void unet1d_plan(cindm_unet1d* h);
extern "C" int cindm_unet1d_set_option(cindm_unet1d* h, const char* key, int32_t value) {
    const int rc = core_set_option(h, key, value);
    if (rc == 1) {
        h->generation = ++g_generation;         // (captured steps embed the run-time switches: never replay an older capture)
        if (std::string(key) == "tune" && h->finalized) unet1d_plan(h);      // (a tune bit may change what a launch registers for the warm-up)
    }
    return rc < 0 ? -1 : 0;
}

extern "C" int cindm_unet1d_get_option(const cindm_unet1d* h, const char* key, int32_t* value) { return core_get_option(h, key, value); }

extern "C" int cindm_unet1d_create(const cindm_unet1d_desc* desc, cindm_unet1d** out) {
    REQUIRE(desc && out, "null argument");
    REQUIRE(desc->n_mults >= 1 && desc->n_mults <= 8, "n_mults out of range");
    // 96: GroupNorm groups of 3 * 2^k channels, served by the generic tier (kernels.h, g3_group); every accepted width makes
    // every level's group width dim * m / 8 a multiple of 4
    REQUIRE(desc->dim == 96 || (desc->dim >= 32 && (desc->dim & (desc->dim - 1)) == 0), "dim must be a power of two >= 32 or 96");
    for (int i = 0; i < desc->n_mults; ++i)
        REQUIRE(desc->dim_mults[i] >= 1 && (desc->dim_mults[i] & (desc->dim_mults[i] - 1)) == 0, "dim_mults must be powers of two");
    REQUIRE(desc->transition_dim % 4 == 0 && desc->transition_dim >= 4 && desc->transition_dim <= 32,
            "transition_dim must be a multiple of 4 in [4, 32]");
    REQUIRE(desc->horizon >= 2 && desc->horizon <= TM, "horizon must be in [2, 48]");
    REQUIRE(desc->timesteps >= 1, "timesteps must be >= 1");
    auto* h = new cindm_unet1d();
    h->d = *desc;
    h->init_options(kUnet1dOpts);
    if (build_manifest(h) != 0) { delete h; return -1; }
    // every internal length must stay integral
    int L = desc->horizon;
    for (int ind = 0; ind < desc->n_mults - h->n_plain; ++ind) {
        if (L % 2) { delete h; return fail("horizon not divisible for the down-sampling levels"); }
        L /= 2;
    }
    *out = h;
    return 0;
}

extern "C" void cindm_unet1d_destroy(cindm_unet1d* h) {
    if (!h) return;
    if (h->blob) (void)hipFree(h->blob);
    if (h->ttable) (void)hipFree(h->ttable);
    if (h->epoch_dev) (void)hipFree(h->epoch_dev);
    if (h->ph_buf) (void)hipFree(h->ph_buf);
    delete h;
}

extern "C" int cindm_unet1d_num_params(const cindm_unet1d* h) { return core_num_params(h); }
extern "C" int cindm_unet1d_param_info(const cindm_unet1d* h, int idx, char* name, int cap, int64_t shape[4], int* ndim) {
    return core_param_info(h, idx, name, cap, shape, ndim);
}
extern "C" int cindm_unet1d_set_param(cindm_unet1d* h, const char* key, const float* src, int64_t numel, int on_device) {
    return core_set_param(h, key, src, numel, on_device);
}
extern "C" int cindm_unet1d_set_sinusoid_table(cindm_unet1d* h, const float* t, int64_t numel) {
    return core_set_sinusoid(h, t, numel, h ? (int64_t)h->d.timesteps * h->d.dim : 0);
}

// ---- weight packing ([tap][CinP][Npad], zero padded) -------------------------------------------
struct BlobBuilder {
    std::vector<float> data;
    size_t alloc(size_t n) { size_t o = data.size(); data.resize(o + ceil_to((int)n, 64), 0.f); return o; }
};

static const Param& P(const cindm_unet1d* h, const std::string& k) { return h->params[h->index.at(k)]; }
static uint16_t f16_bits(float v) { _Float16 hv = (_Float16)v; uint16_t u; std::memcpy(&u, &hv, 2); return u; }

// kind 0: conv weight [Co][Ci][k]; kind 1: conv-transpose weight [Ci][Co][k]; kind 2: linear [Co][Ci]
// split: channel count of the first concatenated source (0 = single source)
static void pack_bias(cindm_unet1d* h, BlobBuilder& bb, const std::string& prefix, Packed& pk, int Co) {
    auto bi = h->index.find(prefix + ".bias");
    if (bi != h->index.end()) {
        pk.has_bias = true;
        pk.bias_off = bb.alloc(pk.Npad);
        const Param& b = h->params[bi->second];
        for (int n = 0; n < Co; ++n) bb.data[pk.bias_off + n] = b.host[n];
    }
}

// Split-fp16 packing for conv_gemm_h3_kernel: w = wh + 2^-11 * wl', wh = fp16(w), wl' = fp16((w - wh) * 2^11);
// layout [n-tile][stage of 128 channels][q = (tap*2 + nb)*2 + plane][thread = wave*64 + lane][8 halfs], where the
// 8 halfs are B[k = (lane>>4)*8 + e][j = lane&15] of v_mfma_f32_16x16x32_f16 for the wave's 32-channel k-group.
static void pack_weight_h3(cindm_unet1d* h, BlobBuilder& bb, const std::string& prefix, int split, int kind = 0) {
    const Param& w = P(h, prefix + ".weight");
    // kind 0: Conv1d weight [Co][Ci][K]; kind 1: ConvTranspose1d weight [Ci][Co][K]
    const int Co = (int)w.shape[kind == 1 ? 1 : 0], Ci = (int)w.shape[kind == 1 ? 0 : 1], K = (int)w.shape[2];
    const int KC = 128;
    const int C0 = split ? split : Ci, C1 = Ci - C0;
    const int C0p = ceil_to(C0, KC), C1p = C1 ? ceil_to(C1, KC) : 0;
    Packed pk; pk.T = K; pk.CinP = C0p + C1p; pk.Npad = ceil_to(Co, TN); pk.N = Co; pk.KC = KC; pk.h3 = true;
    const int nch = pk.CinP / KC;
    const size_t halfs = (size_t)(pk.Npad / TN) * nch * (K * 4) * 256 * 8;
    pk.sz = halfs / 2; pk.off = bb.alloc(pk.sz);
    uint16_t* base = reinterpret_cast<uint16_t*>(bb.data.data() + pk.off);
    for (int nt = 0; nt < pk.Npad / TN; ++nt)
        for (int ch = 0; ch < nch; ++ch)
            for (int tap = 0; tap < K; ++tap)
                for (int nb = 0; nb < 2; ++nb)
                    for (int tid = 0; tid < 256; ++tid) {
                        const int wv = tid >> 6, lane = tid & 63;
                        const int n = nt * TN + nb * 16 + (lane & 15);
                        for (int e = 0; e < 8; ++e) {
                            const int cp = ch * KC + wv * 32 + (lane >> 4) * 8 + e;
                            int c = -1;
                            if (cp < C0) c = cp;
                            else if (cp >= C0p && cp - C0p < C1) c = C0 + (cp - C0p);
                            float v = 0.f;
                            if (c >= 0 && n < Co) v = (kind == 1) ? w.host[((size_t)c * Co + n) * K + tap] : w.host[((size_t)n * Ci + c) * K + tap];
                            const _Float16 hv = (_Float16)v;
                            const float lo = (v - (float)hv) * 2048.0f;
                            const size_t q0 = ((size_t)(nt * nch + ch) * (K * 4) + (tap * 2 + nb) * 2) * 256;
                            base[((q0 + tid) * 8) + e] = f16_bits((float)hv);
                            base[((q0 + 256 + tid) * 8) + e] = f16_bits(lo);
                        }
                    }
    pack_bias(h, bb, prefix, pk, Co);
    h->packed[prefix] = pk;
}

// to_qkv (1x1, no bias) of the shallow levels (C = 64 / 128) in conv1x1_wide_kernel's fragment layout:
// [n-tile of 64][q = k-step / 4][thread = wave*64 + lane][4 k-steps], W[n = tile*64 + wave*16 + (lane & 15)][k = 4*(4q+j) + (lane >> 4)]
static void pack_weight_wide(cindm_unet1d* h, BlobBuilder& bb, const std::string& prefix) {
    const Param& w = P(h, prefix + ".weight");
    const int Co = (int)w.shape[0], Ci = (int)w.shape[1];
    if (Ci != 64 && Ci != 128) return;
    Packed pk; pk.T = 1; pk.CinP = Ci; pk.Npad = ceil_to(Co, 64); pk.N = Co; pk.KC = Ci;
    const int NQ = Ci / 16;
    pk.sz = (size_t)(pk.Npad / 64) * NQ * 256 * 4; pk.off = bb.alloc(pk.sz);
    float* base = bb.data.data() + pk.off;
    for (int it = 0; it < pk.Npad / 64; ++it)
        for (int q = 0; q < NQ; ++q)
            for (int tid = 0; tid < 256; ++tid)
                for (int j = 0; j < 4; ++j) {
                    const int wv = tid >> 6, lane = tid & 63;
                    const int n = it * 64 + wv * 16 + (lane & 15), k = 4 * (4 * q + j) + (lane >> 4);
                    base[(((size_t)it * NQ + q) * 256 + tid) * 4 + j] = (n < Co) ? w.host[(size_t)n * Ci + k] : 0.f;
                }
    h->packed[prefix + "#wide"] = pk;
}

// attn1d_site_kernel operands: to_qkv as 24 tiles of 16 channels, to_out as C/16 tiles over the 128 head channels;
// fragment [tile][k16][lane][j] = W[tile*16 + lane%16][k16*16 + (lane/16)*4 + j]
static void pack_attn_site(cindm_unet1d* h, BlobBuilder& bb, const std::string& attn_prefix) {
    const Param& wq = P(h, attn_prefix + ".to_qkv.weight");
    const Param& wo = P(h, attn_prefix + ".to_out.weight");
    const int C = (int)wq.shape[1];
    if ((int)wq.shape[0] != 384 || (int)wo.shape[1] != 128 || (int)wo.shape[0] != C) return;
    if (C != 64 && C != 128 && C != 256 && C != 512) return;
    auto frag = [&](const Param& w, int Co, int Ci, const std::string& name) {
        Packed pk; pk.T = 1; pk.CinP = Ci; pk.Npad = Co; pk.N = Co; pk.KC = Ci;
        const int K16 = Ci / 16;
        pk.sz = (size_t)(Co / 16) * K16 * 256; pk.off = bb.alloc(pk.sz);
        float* base = bb.data.data() + pk.off;
        for (int t = 0; t < Co / 16; ++t)
            for (int k = 0; k < K16; ++k)
                for (int lane = 0; lane < 64; ++lane)
                    for (int j = 0; j < 4; ++j)
                        base[(((size_t)t * K16 + k) * 64 + lane) * 4 + j] =
                            w.host[(size_t)(t * 16 + (lane & 15)) * Ci + k * 16 + (lane >> 4) * 4 + j];
        h->packed[name] = pk;
    };
    // split-fp16 fragments: [tile][k32][plane hi / scaled lo][lane][e] = W[tile*16 + lane%16][k32*32 + (lane/16)*8 + e]
    auto frag_h3 = [&](const Param& w, int Co, int Ci, const std::string& name) {
        Packed pk; pk.T = 1; pk.CinP = Ci; pk.Npad = Co; pk.N = Co; pk.KC = Ci; pk.h3 = true;
        const int K32 = Ci / 32;
        pk.sz = (size_t)(Co / 16) * K32 * 2 * 64 * 4; pk.off = bb.alloc(pk.sz);
        uint16_t* base = reinterpret_cast<uint16_t*>(bb.data.data() + pk.off);
        for (int t = 0; t < Co / 16; ++t)
            for (int k = 0; k < K32; ++k)
                for (int lane = 0; lane < 64; ++lane)
                    for (int e = 0; e < 8; ++e) {
                        const float v = w.host[(size_t)(t * 16 + (lane & 15)) * Ci + k * 32 + (lane >> 4) * 8 + e];
                        const _Float16 hv = (_Float16)v;
                        const float lo = (v - (float)hv) * 2048.0f;
                        const size_t q0 = ((size_t)t * K32 + k) * 2;
                        base[((q0 + 0) * 64 + lane) * 8 + e] = f16_bits((float)hv);
                        base[((q0 + 1) * 64 + lane) * 8 + e] = f16_bits(lo);
                    }
        h->packed[name] = pk;
    };
    if (h->use_h3) {
        frag_h3(wq, 384, C, attn_prefix + ".to_qkv#site");
        frag_h3(wo, C, 128, attn_prefix + ".to_out#site");
    } else {
        frag(wq, 384, C, attn_prefix + ".to_qkv#site");
        frag(wo, C, 128, attn_prefix + ".to_out#site");
    }
}

// level0_down_kernel operands: every convolution of downs.0 as split-fp16 fragments
// [tile of 16 output channels][tap][k32][plane hi / scaled lo][lane][e] = W[tile*16 + lane%16][k32*32 + (lane/16)*8 + e][tap]
// (input channels zero-padded to a multiple of 32)
static bool pack_level_frag(cindm_unet1d* h, BlobBuilder& bb, const std::string& prefix, int want_co, int kind = 0) {
    // kind 0: Conv1d weight [Co][Ci][K]; kind 1: ConvTranspose1d weight [Ci][Co][K]; want_co < 0: any Co <= 16, padded to one tile
    auto it = h->index.find(prefix + ".weight");
    if (it == h->index.end()) {
        if (getenv("CINDM_VERBOSE")) fprintf(stderr, "[cindm] level frag %s: no such parameter\n", prefix.c_str());
        return false;
    }
    const Param& w = h->params[it->second];
    const int Co_ = (int)w.shape[kind == 1 ? 1 : 0], Ci = (int)w.shape[kind == 1 ? 0 : 1], K = (int)w.shape[2];
    if ((want_co >= 0 && Co_ != want_co) || (want_co < 0 && Co_ > 16) || (Ci > 32 && Ci % 32 != 0)) {
        if (getenv("CINDM_VERBOSE")) fprintf(stderr, "[cindm] level frag %s rejected: Co %d Ci %d K %d\n", prefix.c_str(), Co_, Ci, K);
        return false;
    }
    const int Co = want_co < 0 ? 16 : Co_;
    const int KS = (Ci + 31) / 32;
    Packed pk; pk.T = K; pk.CinP = KS * 32; pk.Npad = Co; pk.N = Co_; pk.KC = 32; pk.h3 = true;
    pk.sz = (size_t)(Co / 16) * K * KS * 2 * 64 * 4; pk.off = bb.alloc(pk.sz);
    uint16_t* base = reinterpret_cast<uint16_t*>(bb.data.data() + pk.off);
    for (int t = 0; t < Co / 16; ++t)
        for (int tap = 0; tap < K; ++tap)
            for (int k = 0; k < KS; ++k)
                for (int lane = 0; lane < 64; ++lane)
                    for (int e = 0; e < 8; ++e) {
                        const int co = t * 16 + (lane & 15), ci = k * 32 + (lane >> 4) * 8 + e;
                        float v = 0.f;
                        if (ci < Ci && co < Co_) v = (kind == 1) ? w.host[((size_t)ci * Co_ + co) * K + tap] : w.host[((size_t)co * Ci + ci) * K + tap];
                        const _Float16 hv = (_Float16)v;
                        const float lo = (v - (float)hv) * 2048.0f;
                        const size_t q0 = (((size_t)t * K + tap) * KS + k) * 2;
                        base[((q0 + 0) * 64 + lane) * 8 + e] = f16_bits((float)hv);
                        base[((q0 + 1) * 64 + lane) * 8 + e] = f16_bits(lo);
                    }
    h->packed[prefix + "#lvl"] = pk;
    return true;
}

// The four level kernels of this handle (LevelSpec); nothing is packed or resolved here.
static void level_specs(cindm_unet1d* h) {
    const int nres = h->d.n_mults, F = h->d.transition_dim;
    auto spec = [&](int k, const std::string& label, const std::string& level, bool fits) -> LevelSpec& {
        LevelSpec& s = h->lvl[k] = LevelSpec{};
        s.label = label + level; s.attn = level + ".2"; s.fits = fits; s.allowed = true;
        return s;
    };
    auto frag = [](LevelSpec& s, FragRole role, const std::string& p, int co, int kind = 0) { s.frags.push_back({role, p, co, kind}); };
    auto block = [&](LevelSpec& s, const std::string& rtb, int co) {      // a ResidualTemporalBlock's two convolutions and its time bias
        frag(s, FRAG_CONV, rtb + ".blocks.0.block.0", co); frag(s, FRAG_CONV, rtb + ".blocks.1.block.0", co);
        s.rtb.push_back(rtb);
    };
    // level0_down_kernel (F -> 64) / level1_down_kernel (64 -> 128): RTB, RTB with an identity residual, attention, Downsample1d
    auto down = [&](LevelSpec& s, const std::string& p, int co) {
        block(s, p + ".0", co); block(s, p + ".1", co); frag(s, FRAG_RES, p + ".0.residual_conv", co); frag(s, FRAG_RESAMPLE, p + ".3.conv", co);
        s.allowed = !h->index.count(p + ".1.residual_conv.weight");
    };
    LevelSpec& l0 = spec(LV_LEVEL0, "level0_down ", "downs.0", true);
    down(l0, "downs.0", 64);
    l0.allowed = l0.allowed && F <= 32;
    down(spec(LV_LEVEL1, "level1_down ", "downs.1", h->dims.size() > 2 && h->dims[1] == 64 && h->dims[2] == 128), "downs.1", 128);
    // ups_last_kernel: the finest up level (RTB(256 -> 128), RTB(128 -> 64), attention(64), Upsample1d) + the output head
    const std::string u = "ups." + std::to_string(nres - 2), v = "ups." + std::to_string(nres - 3);
    LevelSpec& ul = spec(LV_UPS_LAST, "ups_last ", u, nres >= 3 && F <= 16 && F % 4 == 0);
    ul.label += " + final_conv";
    block(ul, u + ".0", 128); frag(ul, FRAG_RES, u + ".0.residual_conv", 128);
    block(ul, u + ".1", 64); frag(ul, FRAG_RES, u + ".1.residual_conv", 64);
    frag(ul, FRAG_CONV, "final_conv.0.block.0", 64); frag(ul, FRAG_RESAMPLE, u + ".3.conv", 64, 1); frag(ul, FRAG_HEAD, "final_conv.1", -1);
    // ups_tail128_kernel: the second half of the level above it (RTB(256 -> 128), attention(128), Upsample1d(128))
    LevelSpec& ut = spec(LV_UPS_TAIL, "ups_tail128 ", v, nres >= 4 && h->dims[3] == 256);
    block(ut, v + ".1", 128); frag(ut, FRAG_RES, v + ".1.residual_conv", 128); frag(ut, FRAG_RESAMPLE, v + ".3.conv", 128, 1);
}

// Packs the level kernels' fragments in the order of the specs and resolves the specs whose kernel can run.  A kernel of the up
// path is packed only when level 1's fragments were (the same widths on the way down).
static void pack_level0(cindm_unet1d* h, BlobBuilder& bb) {
    level_specs(h);
    bool level1_packed = false;
    for (int k = 0; k < LV_COUNT; ++k) {
        LevelSpec& s = h->lvl[k];
        bool ok = s.fits && (k <= LV_LEVEL1 || level1_packed);
        if (ok) for (const LevelFrag& f : s.frags) ok = pack_level_frag(h, bb, f.p, f.want_co, f.kind) && ok;
        if (k == LV_LEVEL1) level1_packed = ok;
        s.ok = ok && s.allowed && h->index.count(s.attn + ".fn.fn.to_qkv.weight");
    }
    // (after the last insertion into h->packed: its elements stay where they are until the next pack clears it)
    for (LevelSpec& s : h->lvl) {
        if (!s.ok) continue;
        size_t lo = ~(size_t)0, hi = 0;
        for (LevelFrag& f : s.frags) {
            f.w = &h->packed.at(f.p + "#lvl"); f.b = &h->packed.at(f.p);
            lo = std::min(lo, f.w->off); hi = std::max(hi, f.w->off + f.w->sz);
            if (f.role != FRAG_CONV) continue;
            const std::string gn = f.p.substr(0, f.p.size() - 1) + "2";          // "<block>.block.0" -> "<block>.block.2"
            f.gam = h->vec_off.at(gn + ".weight"); f.bet = h->vec_off.at(gn + ".bias");
        }
        s.span.off = lo; s.span.sz = hi - lo;
        auto site = h->packed.find(s.attn + ".fn.fn.to_qkv#site");
        if (site != h->packed.end()) { s.qkv = &site->second; s.wo = &h->packed.at(s.attn + ".fn.fn.to_out#site"); }
        s.bo = &h->packed.at(s.attn + ".fn.fn.to_out");
        s.ln_g = h->vec_off.at(s.attn + ".fn.norm.g");
        for (size_t i = 0; i < s.rtb.size(); ++i) s.tb[i] = h->tb_off.at(s.rtb[i]);
    }
}

// residual_conv (1x1) in the split-fp16 layout of conv_gemm_h3_kernel's second GEMM: [n-tile][stage of 128 channels]
// [q = nb*2 + plane][thread][8 halfs], channel mapping identical to the k=5 convolution that shares its staged rows
static void pack_weight_h3_res(cindm_unet1d* h, BlobBuilder& bb, const std::string& prefix, int split) {
    const Param& w = P(h, prefix + ".weight");
    const int Co = (int)w.shape[0], Ci = (int)w.shape[1];
    const int KC = 128;
    const int C0 = split ? split : Ci, C1 = Ci - C0;
    const int C0p = ceil_to(C0, KC), C1p = C1 ? ceil_to(C1, KC) : 0;
    Packed pk; pk.T = 1; pk.CinP = C0p + C1p; pk.Npad = ceil_to(Co, TN); pk.N = Co; pk.KC = KC; pk.h3 = true;
    const int nch = pk.CinP / KC;
    const size_t halfs = (size_t)(pk.Npad / TN) * nch * 4 * 256 * 8;
    pk.sz = halfs / 2; pk.off = bb.alloc(pk.sz);
    uint16_t* base = reinterpret_cast<uint16_t*>(bb.data.data() + pk.off);
    for (int nt = 0; nt < pk.Npad / TN; ++nt)
        for (int ch = 0; ch < nch; ++ch)
            for (int nb = 0; nb < 2; ++nb)
                for (int tid = 0; tid < 256; ++tid) {
                    const int wv = tid >> 6, lane = tid & 63;
                    const int n = nt * TN + nb * 16 + (lane & 15);
                    for (int e = 0; e < 8; ++e) {
                        const int cp = ch * KC + wv * 32 + (lane >> 4) * 8 + e;
                        int c = -1;
                        if (cp < C0) c = cp;
                        else if (cp >= C0p && cp - C0p < C1) c = C0 + (cp - C0p);
                        const float v = (c >= 0 && n < Co) ? w.host[(size_t)n * Ci + c] : 0.f;
                        const _Float16 hv = (_Float16)v;
                        const float lo = (v - (float)hv) * 2048.0f;
                        const size_t q0 = ((size_t)(nt * nch + ch) * 4 + nb * 2) * 256;
                        base[((q0 + tid) * 8) + e] = f16_bits((float)hv);
                        base[((q0 + 256 + tid) * 8) + e] = f16_bits(lo);
                    }
                }
    pack_bias(h, bb, prefix, pk, Co);
    h->packed[prefix + "#h3"] = pk;
}

static void pack_weight(cindm_unet1d* h, BlobBuilder& bb, const std::string& prefix, int kind, int split) {
    const Param& w = P(h, prefix + ".weight");
    int Co, Ci, K;
    if (kind == 0) { Co = (int)w.shape[0]; Ci = (int)w.shape[1]; K = (int)w.shape[2]; }
    else if (kind == 1) { Ci = (int)w.shape[0]; Co = (int)w.shape[1]; K = (int)w.shape[2]; }
    else { Co = (int)w.shape[0]; Ci = (int)w.shape[1]; K = 1; }
    if (kind == 0 && K == 5 && h->use_h3) { pack_weight_h3(h, bb, prefix, split); return; }
    if (h->use_h3 && ((kind == 0 && K == 3) || (kind == 1 && K == 4))) { pack_weight_h3(h, bb, prefix, split, kind); return; }
    const int C0 = split ? split : Ci, C1 = Ci - C0;
    // stage width: tap-ful convolutions stage 32 channels x T taps; 1x1 layers stage 64 or 128 channels
    const int KC = (K > 1) ? 32 : ((C0 % 128 == 0 && C1 % 128 == 0) ? 128 : 64);
    int C0p = ceil_to(C0, KC), C1p = C1 ? ceil_to(C1, KC) : 0;
    // the kernel's two-set register pipeline wants an even number of stages (or exactly one): pad with a zero stage
    if (((C0p + C1p) / KC) > 1 && ((C0p + C1p) / KC) % 2) { if (C1) C1p += KC; else C0p += KC; }
    Packed pk; pk.T = K; pk.CinP = C0p + C1p; pk.Npad = ceil_to(Co, TN); pk.N = Co; pk.KC = KC;
    // MFMA-fragment order: [n-tile][stage][q][thread = wave*64 + lane][4], flat j = 4q + e = (tap*CS + cs)*2 + nb: the
    // value a lane feeds to v_mfma_f32_16x16x4_f32 as B[k = lane>>4][j = lane&15] of k-step (tap, cs), column block
    // nb.  Every float4 load of a wave is 1 KiB contiguous.
    const int nch = pk.CinP / KC, CPW = KC / 4, CS = CPW / 4, KS = K * CS;
    pk.sz = (size_t)K * pk.CinP * pk.Npad; pk.off = bb.alloc(pk.sz);
    float* base = bb.data.data() + pk.off;
    for (int nt = 0; nt < pk.Npad / TN; ++nt)
        for (int ch = 0; ch < nch; ++ch)
            for (int tid = 0; tid < 256; ++tid) {
                const int wv = tid >> 6, lane = tid & 63;
                float* dst = base + ((size_t)nt * nch + ch) * 256 * (2 * KS);      // + ((j/4)*256 + tid)*4 + j%4
                for (int tap = 0; tap < K; ++tap)
                    for (int cs = 0; cs < CS; ++cs)
                        for (int nb = 0; nb < 2; ++nb) {
                            const int cp = ch * KC + wv * CPW + cs * 4 + (lane >> 4);     // padded channel index
                            const int n = nt * TN + nb * 16 + (lane & 15);
                            int c = -1;
                            if (cp < C0) c = cp;
                            else if (cp >= C0p && cp - C0p < C1) c = C0 + (cp - C0p);
                            float v = 0.f;
                            if (c >= 0 && n < Co) {
                                if (kind == 0) v = w.host[((size_t)n * Ci + c) * K + tap];
                                else if (kind == 1) v = w.host[((size_t)c * Co + n) * K + tap];
                                else v = w.host[(size_t)n * Ci + c];
                            }
                            const int j = (tap * CS + cs) * 2 + nb;
                            dst[((size_t)(j / 4) * 256 + tid) * 4 + (j % 4)] = v;
                        }
            }
    pack_bias(h, bb, prefix, pk, Co);
    h->packed[prefix] = pk;
}

static void pack_vec(cindm_unet1d* h, BlobBuilder& bb, const std::string& key) {
    const Param& v = P(h, key);
    size_t o = bb.alloc(v.numel);
    std::memcpy(bb.data.data() + o, v.host.data(), v.numel * sizeof(float));
    h->vec_off[key] = o;
}

// launch through the emitter: plain, or with per-dispatch timestamps in profile mode
#define KLAUNCH(E_, kernel, grid, block, shm, ...) \
    do { \
        if ((E_).prof_cur) hipExtLaunchKernelGGL(kernel, grid, block, shm, (E_).stream, (E_).prof_cur->e0, (E_).prof_cur->e1, 0, __VA_ARGS__); \
        else hipLaunchKernelGGL(kernel, grid, block, shm, (E_).stream, __VA_ARGS__); \
    } while (0)

// ---- launch helpers ---------------------------------------------------------------------------
struct Ten { float* p = nullptr; int L = 0, C = 0, ld = 0; uint4* pl = nullptr; size_t pst = 0;   // pl: tiled split-fp16 planes (dconv_kernel)
             size_t off_p = ~(size_t)0, sz_p = 0, off_pl = ~(size_t)0, sz_pl = 0; };      // workspace blocks behind p / pl (none: caller's memory)

struct Emitter {
    cindm_unet1d* h;
    hipStream_t stream;
    bool dry;                 // dry run: only count workspace + launches
    char* ws; size_t ws_off = 0;
    int64_t rows;
    const int* t_ptr; int t_imm;
    int launches = 0;
    hipError_t err = hipSuccess;
    // a dry run counts launches, workspace and warm-up regions of `rows` rows; a live one launches on `stream` out of `ws`
    static Emitter dry_run(cindm_unet1d* h, int64_t rows) { return Emitter{h, nullptr, true, nullptr, 0, rows, nullptr, 0}; }
    static Emitter live(cindm_unet1d* h, hipStream_t stream, void* ws, int64_t rows, const int* t_ptr, int t_imm) {
        return Emitter{h, stream, false, (char*)ws, 0, rows, t_ptr, t_imm};
    }
    struct ProfRec { int kind; hipEvent_t e0, e1; double flops; int gx, gy, nstage; };
    std::vector<ProfRec>* prof = nullptr;     // when set, every launch records its own begin / end timestamps
    ProfRec* prof_cur = nullptr;              // the record of the launch being emitted (profile mode)
    static constexpr int prof_reps = 1;       // one pass in forward order: caches as cold as in the real step
    // L2 warm-up (kernels.h, Pf): every launch registers the blob ranges it streams; the table of a dry run at finalize
    // (h->pf_table, one entry per launch in order) tells launch i what launch i + 1 will stream
    int pf_idx = 0;
    std::vector<cindm_unet1d::WReg>* pf_out = nullptr;
    // `issue` false: this launch streams what it registers but touches nothing for its successor.  Round 6 measured every launch of the
    // headline step with its touches off (tools/pf_mask_scan.py, one process): the three attn1d_head launches pay 1.2 - 1.5 us for them
    // (they end on a spin + a short projection: nothing hides the touches) and their successors gain nothing -- a C = 512 dconv2
    // launch streams at the L2-hot rate either way, its 16 workgroups per n-tile warm each other --: -0.9 / -1.0 / -0.9 us per step
    // without; downs.3.1 (in front of the first of them): -0.5 us.  Every other launch's touches are worth 0 ... +1.0 us per step.
    bool pf_issue = true;
    void pf_step(Pf& pf, const cindm_unet1d::WReg& mine) {
        std::memset(&pf, 0, sizeof(pf));
        if (pf_out) pf_out->push_back(mine);
        const auto& tab = h->pf_table;
        // (experiment: bits 2.. of `tune` = launches of the forward that issue NO touches, bit 2 + i = launch i)
        if (!dry && !pf_out && h->O("l2_prefetch") && !tab.empty() && (pf_issue || (h->O("tune") & 1)) && !(((h->O("tune") >> 2) >> (pf_idx % 24)) & 1)) {
            const cindm_unet1d::WReg& nx = tab[(size_t)(pf_idx + 1) % tab.size()];
            for (int k = 0; k < PF_REGIONS; ++k) {
                pf.base[k] = reinterpret_cast<const char*>(h->blob) + nx.off[k];
                pf.bytes[k] = nx.bytes[k]; pf.stride[k] = nx.stride[k];
            }
            pf.sink = h->epoch_dev + 2;
            pf.late = (h->O("tune") & 1) ? 0 : 1;      // round 6: touches a few microseconds before the launch ends (tune bit 0: round 5's, at its head)
        }
        if (!dry && !pf_out) pf.wt = (h->O("tune") & 2) ? 0 : 1;        // round 6: the launch's outputs are written through (kernels.h st_out; tune bit 1: round 5's plain stores)
        ++pf_idx;
    }
    // weights tiled by 32-column n-tile (conv_gemm_h3_kernel / dconv_kernel packings): tile nt is streamed by the
    // workgroups with blockIdx.x = nt, i.e. on XCD nt % 8 when the grid's x extent is a multiple of 8
    void pf_tiled(Pf& pf, const Packed& pk, int ntiles) {
        cindm_unet1d::WReg r{};
        const size_t tile = pk.sz * 4 / (size_t)(ntiles > 0 ? ntiles : 1);
        if (ntiles % 8 == 0 && ntiles > 0) {
            r.off[0] = pk.off * 4; r.bytes[0] = (unsigned)tile; r.stride[0] = (unsigned)tile;
            if (ntiles >= 16) { r.off[1] = pk.off * 4 + 8 * tile; r.bytes[1] = (unsigned)tile; r.stride[1] = (unsigned)tile; }
        } else {
            r.off[0] = pk.off * 4; r.bytes[0] = (unsigned)std::min(pk.sz * 4, (size_t)2 << 20); r.stride[0] = 0;
        }
        pf_step(pf, r);
    }
    // weights every workgroup streams: the blob range [lo, hi) of the packed tensors `a` (region 0) and `b` (region 1)
    void pf_all(Pf& pf, std::initializer_list<const Packed*> a0, std::initializer_list<const Packed*> b0) {
        cindm_unet1d::WReg r{};
        int k = 0;
        for (const auto& lst : {a0, b0}) {
            size_t lo = ~(size_t)0, hi = 0;
            for (const Packed* q : lst) if (q) { lo = std::min(lo, q->off); hi = std::max(hi, q->off + q->sz); }
            if (hi > lo) { r.off[k] = lo * 4; r.bytes[k] = (unsigned)std::min((hi - lo) * 4, (size_t)2 << 20); r.stride[k] = 0; }
            ++k;
        }
        pf_step(pf, r);
    }
    // a level kernel: region 0 = its "#lvl" fragments, region 1 = its attention site's pair
    Pf pf_level(const LevelSpec& lv) { Pf pf; pf_all(pf, {&lv.span}, {lv.qkv, lv.wo}); return pf; }
    // phase clocks (profiling builds): the record slot of the launch being emitted
    int ph_slot = 0;
    PhaseBuf ph_next(const std::string& name) {
        PhaseBuf b{nullptr, 0};
        if (dry || !h || !h->ph_on || !h->ph_buf || ph_slot >= 32) return b;
        b.buf = h->ph_buf; b.slot = ph_slot++;
        if ((int)h->ph_names.size() <= b.slot) h->ph_names.resize(b.slot + 1);
        h->ph_names[b.slot] = name;
        return b;
    }
    bool epoch_bumped = false;                // dconv pair exchanges: the per-forward epoch has been advanced
    std::vector<std::pair<size_t, size_t>>* xregions = nullptr;      // dry run: (offset, bytes) of the exchange regions

    // tiled planes of an [rows, L, C] tensor (kernels_dconv.h): two planes of tiles * (C / 32) * 192 uint4
    void planes(Ten& t) {
        const int S = 48 / t.L;
        const size_t tiles = (size_t)((rows + S - 1) / S);
        t.pst = tiles * (size_t)(t.C / 32) * 192;
        t.pl = reinterpret_cast<uint4*>(alloc(t.pst * 2 * 4));
        t.off_pl = last_off; t.sz_pl = last_bytes;
    }
    // the in-kernel exchanges of one forward are tagged with its epoch: advance it once, before the first of them
    void need_epoch() {
        if (epoch_bumped) return;
        epoch_bumped = true;
        if (!dry && h->epoch_prebumped) { h->epoch_prebumped = false; return; }    // done by the previous step's counter kernel
        ++launches;
        if (!dry) hipLaunchKernelGGL(dconv_epoch_kernel, dim3(1), dim3(64), 0, stream, h->epoch_dev);
    }
    unsigned long long* xchg(size_t granules) {
        float* p = alloc(granules * 2, false);
        if (xregions) xregions->push_back({last_off, granules * 8});
        return reinterpret_cast<unsigned long long*>(p);
    }

    // Profile mode: the launch goes through hipExtLaunchKernelGGL, whose start / stop events carry the dispatch's own
    // begin / end timestamps (what rocprofv3 --kernel-trace reports), not the cost of an event bracket around it.
    void prof_begin(int kind, double flops) {
        if (!prof || dry) return;
        ProfRec r; r.kind = kind; r.flops = flops; r.gx = r.gy = r.nstage = 0;
        (void)hipEventCreate(&r.e0); (void)hipEventCreate(&r.e1);
        prof->push_back(r);
        prof_cur = &prof->back();
    }
    void prof_end() { prof_cur = nullptr; }
    void note_error() { hipError_t e = hipGetLastError(); if (e != hipSuccess && err == hipSuccess) err = e; }      // the first launch error of the emission
    // `go` issues one launch through KLAUNCH: under the profile bracket, prof_reps times in profile mode
    template <typename Go> void profiled(int kind, double flops, Go go) {
        prof_begin(kind, flops);
        for (int rep = 0; rep < (prof ? prof_reps : 1); ++rep) go();
        prof_end();
    }

    // Workspace blocks.  On the sampling path (option "taps" = 0, "ws_alias" = 1) a block goes back to a free list when the
    // last launch that reads it has been emitted (drop): launches execute in stream order, so a later launch can only
    // overwrite what every earlier launch has finished with.  Every activation of this U-Net has C * L = 1536 floats per row,
    // so exact-size reuse finds a block almost always: the live set is the current tensor, the skips and a block's
    // temporaries -- 157 MB -> ~20 MB at 256 rows, which keeps weights + activations of the 768 / 1280-row configurations inside
    // the 256 MiB Infinity Cache.  With "taps" = 1 every intermediate keeps its own block (the tap API reads them afterwards).
    // Exchange regions (xchg) are never recycled: their words are tags.
    std::multimap<size_t, size_t> free_blocks;       // bytes -> offset
    bool reuse = false;
    size_t last_off = 0, last_bytes = 0;
    float* alloc(size_t nfloats, bool recyclable = true) {
        const size_t bytes = ((nfloats * sizeof(float) + 255) / 256) * 256;
        size_t o;
        auto it = (reuse && recyclable) ? free_blocks.find(bytes) : free_blocks.end();
        if (it != free_blocks.end()) { o = it->second; free_blocks.erase(it); }
        else { o = ws_off; ws_off += bytes; }
        last_off = o; last_bytes = bytes;
        return dry ? nullptr : reinterpret_cast<float*>(ws + o);
    }
    void drop_block(size_t off, size_t bytes) { if (reuse && off != ~(size_t)0 && bytes) free_blocks.insert({bytes, off}); }
    void drop(Ten& t) { drop_block(t.off_p, t.sz_p); drop_block(t.off_pl, t.sz_pl); t.off_p = t.off_pl = ~(size_t)0; }
    struct Tmp { size_t off, bytes; };
    float* tmp(size_t nfloats, Tmp& k) { float* p = alloc(nfloats); k = {last_off, last_bytes}; return p; }
    void drop(const Tmp& k) { drop_block(k.off, k.bytes); }
    Ten ten(int L, int C) { Ten t; t.L = L; t.C = C; t.ld = C; t.p = alloc((size_t)rows * L * C); t.off_p = last_off; t.sz_p = last_bytes; return t; }
    const float* W(const Packed& pk) const { return h->blob + pk.off; }
    const float* B(const Packed& pk) const { return pk.has_bias ? h->blob + pk.bias_off : nullptr; }
    const float* V(const std::string& k) const { return h->blob + h->vec_off.at(k); }

    void base(GemmArgs& a, const Packed& pk, int Bp, int Lin, int Lout) {
        std::memset(&a, 0, sizeof(a));
        a.W = W(pk); a.bias = B(pk); a.CinP = pk.CinP; a.Npad = pk.Npad; a.N = pk.N; a.KC = pk.KC; a.h3 = pk.h3 ? 1 : 0;
        a.Bp = Bp; a.Lin = Lin; a.Lout = Lout; a.stride = 1; a.pad = pk.T / 2; a.transposed = 0;
        a.spt = TM / (Lout > 0 ? Lout : 1);
        if (a.spt * Lin > MAXR) a.spt = MAXR / Lin;
        if (a.spt < 1) a.spt = 1;
        a.t_ptr = t_ptr; a.t_imm = t_imm;
        a.nsrc = 1;
        a.lout_magic = (65536 + Lout - 1) / Lout;
        a.lin_magic = (65536 + Lin - 1) / Lin;
    }
    static void plain(Src& s, const Ten& t) { s.p = t.p; s.ld = t.ld; s.C = t.C; s.mode = SRC_PLAIN; s.P = 1; s.gw = 1; s.cnt = 1.f; }

    void launch(int T, const GemmArgs& a) {
        ++launches;
        if (h) {                                  // register this launch's weights, learn the next launch's (L2 warm-up)
            cindm_unet1d::WReg r{};
            const int ntiles = a.Npad / TN;
            if (T > 0 && a.W && ntiles > 0) {
                const size_t off = (size_t)(reinterpret_cast<const char*>(a.W) - reinterpret_cast<const char*>(h->blob));
                const size_t tile = a.h3 ? (size_t)(a.CinP / 128) * T * 16384 : (size_t)T * a.CinP * TN * 4;
                if (ntiles % 8 == 0) {
                    r.off[0] = off; r.bytes[0] = (unsigned)tile; r.stride[0] = (unsigned)tile;
                    if (ntiles >= 16) { r.off[1] = off + 8 * tile; r.bytes[1] = (unsigned)tile; r.stride[1] = (unsigned)tile; }
                } else {
                    r.off[0] = off; r.bytes[0] = (unsigned)std::min(tile * ntiles, (size_t)2 << 20);
                }
            }
            pf_step(const_cast<GemmArgs&>(a).pf, r);
        } else {
            std::memset(&const_cast<GemmArgs&>(a).pf, 0, sizeof(Pf));
        }
        if (dry) return;
        dim3 grid(a.Npad / TN, (unsigned)((a.Bp + a.spt - 1) / a.spt));
        {
            const double cin = (double)a.src[0].C + (a.nsrc > 1 ? (double)a.src[1].C : 0.0);
            const double taps = a.transposed ? T * 0.5 : (double)T;          // algorithmic: 2 of 4 taps hit per output
            // (+ the residual_conv that rides on the centre tap of a k=5 launch: one more tap's worth of products)
            prof_begin(T == 0 ? 0 : T == 1 ? 1 : T == 3 ? 2 : T == 4 ? 3 : 4, 2.0 * a.Bp * a.Lout * a.N * cin * (taps + (a.W2 ? 1.0 : 0.0)));
            if (prof && !dry) { prof->back().gx = grid.x; prof->back().gy = grid.y; prof->back().nstage = T ? a.CinP / a.KC : 0; }
        }
        const int mode = a.src[0].mode;
        // a GroupNorm width of 3 * 2^k (dim = 96) in what this launch produces, normalises on load or adds in its epilogue: the G3
        // instantiations (kernels.h, g3_group).  Producer-side activation needs whole groups in a tile: never at these widths.
        auto g3w = [](int gw) { return gw > 0 && (gw & (gw - 1)) != 0; };
        const bool g3 = (a.stats_out && g3w(a.so_gw)) || (mode == SRC_GN_MISH && g3w(a.src[0].gw)) || (a.e_y && g3w(a.e_gw));
#define CINDM_LAUNCH(T_, KC_, ROWS_, MODE_) KLAUNCH((*this), (conv_gemm_kernel<T_, KC_, ROWS_, MODE_>), grid, dim3(256), 0, a)
#define CINDM_LAUNCH_G3(T_, KC_, ROWS_, MODE_) KLAUNCH((*this), (conv_gemm_kernel<T_, KC_, ROWS_, MODE_, 0, true>), grid, dim3(256), 0, a)
#define CINDM_LAUNCH_H3_G3(MODE_, RES_) KLAUNCH((*this), (conv_gemm_h3_kernel<5, 48, MODE_, RES_, 0, true>), grid, dim3(256), 0, a)
        bool ok = true;
        // profile mode: the (idempotent) launch is repeated inside one event bracket so that the ~6 us cost of the
        // bracket itself is amortised; the reported time is bracket / prof_reps
        for (int rep = 0; rep < (prof ? prof_reps : 1); ++rep) {
        const int dbg_h3 = h ? h->O("dbg") : 0;
        const_cast<GemmArgs&>(a).dbg = a.h3 ? dbg_h3 : 0;
        if (g3) {
            // the launches of emit_rtb's three-launch form and of emit_head, on the split-fp16 and on the fp32-MFMA path
            if (a.act_gamma) ok = false;
            else if (a.h3 && T == 5 && mode == SRC_PLAIN && a.W2) CINDM_LAUNCH_H3_G3(SRC_PLAIN, true);
            else if (a.h3 && T == 5 && mode == SRC_PLAIN) CINDM_LAUNCH_H3_G3(SRC_PLAIN, false);
            else if (a.h3 && T == 5 && mode == SRC_GN_MISH) CINDM_LAUNCH_H3_G3(SRC_GN_MISH, false);
            else if (a.h3) ok = false;
            else if (T == 0) CINDM_LAUNCH_G3(0, 32, 48, SRC_PLAIN);
            else if (T == 5 && mode == SRC_PLAIN) CINDM_LAUNCH_G3(5, 32, 48, SRC_PLAIN);
            else if (T == 5 && mode == SRC_GN_MISH) CINDM_LAUNCH_G3(5, 32, 48, SRC_GN_MISH);
            else if (T == 1 && a.KC == 128 && mode == SRC_PLAIN) CINDM_LAUNCH_G3(1, 128, 48, SRC_PLAIN);
            else if (T == 1 && a.KC == 64 && mode == SRC_PLAIN) CINDM_LAUNCH_G3(1, 64, 48, SRC_PLAIN);
            else if (T == 1 && a.KC == 64 && mode == SRC_GN_MISH) CINDM_LAUNCH_G3(1, 64, 48, SRC_GN_MISH);
            else ok = false;
        }
        else if (a.h3 && T == 5 && mode == SRC_PLAIN && a.W2) KLAUNCH((*this), (conv_gemm_h3_kernel<5, 48, SRC_PLAIN, true>), grid, dim3(256), 0, a);
        else if (a.h3 && T == 5 && mode == SRC_PLAIN && dbg_h3 >= 21 && dbg_h3 <= 25) {
            if (dbg_h3 == 21) KLAUNCH((*this), (conv_gemm_h3_kernel<5, 48, SRC_PLAIN, false, 1>), grid, dim3(256), 0, a);
            else if (dbg_h3 == 22) KLAUNCH((*this), (conv_gemm_h3_kernel<5, 48, SRC_PLAIN, false, 2>), grid, dim3(256), 0, a);
            else if (dbg_h3 == 23) KLAUNCH((*this), (conv_gemm_h3_kernel<5, 48, SRC_PLAIN, false, 3>), grid, dim3(256), 0, a);
            else if (dbg_h3 == 24) KLAUNCH((*this), (conv_gemm_h3_kernel<5, 48, SRC_PLAIN, false, 4>), grid, dim3(256), 0, a);
            else KLAUNCH((*this), (conv_gemm_h3_kernel<5, 48, SRC_PLAIN, false, 5>), grid, dim3(256), 0, a);
        }
        else if (a.h3 && T == 5 && mode == SRC_PLAIN) KLAUNCH((*this), (conv_gemm_h3_kernel<5, 48, SRC_PLAIN>), grid, dim3(256), 0, a);
        else if (a.h3 && T == 5 && mode == SRC_GN_MISH) KLAUNCH((*this), (conv_gemm_h3_kernel<5, 48, SRC_GN_MISH>), grid, dim3(256), 0, a);
        else if (a.h3 && T == 3 && mode == SRC_PLAIN) KLAUNCH((*this), (conv_gemm_h3_kernel<3, 96, SRC_PLAIN>), grid, dim3(256), 0, a);
        else if (a.h3 && T == 4 && mode == SRC_PLAIN) KLAUNCH((*this), (conv_gemm_h3_kernel<4, 48, SRC_PLAIN>), grid, dim3(256), 0, a);
        else if (a.h3) ok = false;
        else if (T == 0) CINDM_LAUNCH(0, 32, 48, SRC_PLAIN);
        else if (T == 5 && mode == SRC_PLAIN) {
            const int dbg = h ? h->O("dbg") : 0;   // timing ablations (wrong results)
            if (dbg == 1) KLAUNCH((*this), (conv_gemm_kernel<5, 32, 48, SRC_PLAIN, 1>), grid, dim3(256), 0, a);
            else if (dbg == 2) KLAUNCH((*this), (conv_gemm_kernel<5, 32, 48, SRC_PLAIN, 2>), grid, dim3(256), 0, a);
            else if (dbg == 3) KLAUNCH((*this), (conv_gemm_kernel<5, 32, 48, SRC_PLAIN, 3>), grid, dim3(256), 0, a);
            else if (dbg == 4) KLAUNCH((*this), (conv_gemm_kernel<5, 32, 48, SRC_PLAIN, 4>), grid, dim3(256), 0, a);
            else if (dbg == 5) KLAUNCH((*this), (conv_gemm_kernel<5, 32, 48, SRC_PLAIN, 5>), grid, dim3(256), 0, a);
            else if (dbg == 6) KLAUNCH((*this), (conv_gemm_kernel<5, 32, 48, SRC_PLAIN, 6>), grid, dim3(256), 0, a);
            else if (dbg == 7) KLAUNCH((*this), (conv_gemm_kernel<5, 32, 48, SRC_PLAIN, 7>), grid, dim3(256), 0, a);
            else if (dbg == 8) KLAUNCH((*this), (conv_gemm_kernel<5, 32, 48, SRC_PLAIN, 8>), grid, dim3(256), 0, a);
            else CINDM_LAUNCH(5, 32, 48, SRC_PLAIN);
        }
        else if (T == 5 && mode == SRC_GN_MISH) CINDM_LAUNCH(5, 32, 48, SRC_GN_MISH);
        else if (T == 3 && mode == SRC_PLAIN) CINDM_LAUNCH(3, 32, 96, SRC_PLAIN);
        else if (T == 4 && mode == SRC_PLAIN) CINDM_LAUNCH(4, 32, 48, SRC_PLAIN);
        else if (T == 1 && a.KC == 128) {
            if (mode == SRC_PLAIN) CINDM_LAUNCH(1, 128, 48, SRC_PLAIN);
            else if (mode == SRC_LN) CINDM_LAUNCH(1, 128, 48, SRC_LN);
            else if (mode == SRC_MISH) CINDM_LAUNCH(1, 128, 48, SRC_MISH);
            else if (mode == SRC_GELU) CINDM_LAUNCH(1, 128, 48, SRC_GELU);
            else if (mode == SRC_SILU) CINDM_LAUNCH(1, 128, 48, SRC_SILU);
            else ok = false;
        } else if (T == 1 && a.KC == 64) {
            if (mode == SRC_PLAIN) CINDM_LAUNCH(1, 64, 48, SRC_PLAIN);
            else if (mode == SRC_LN) CINDM_LAUNCH(1, 64, 48, SRC_LN);
            else if (mode == SRC_MISH) CINDM_LAUNCH(1, 64, 48, SRC_MISH);
            else if (mode == SRC_GN_MISH) CINDM_LAUNCH(1, 64, 48, SRC_GN_MISH);
            else ok = false;
        } else ok = false;
        }
#undef CINDM_LAUNCH
#undef CINDM_LAUNCH_G3
#undef CINDM_LAUNCH_H3_G3
        if (!ok) err = hipErrorInvalidValue;
        prof_end();
        note_error();
    }
    void tap(const std::string& name, const Ten& t) {
        if (dry || reuse) return;            // (recycled workspace: an intermediate may be overwritten before the forward ends)
        h->taps[name] = {(size_t)(reinterpret_cast<char*>(t.p) - ws), t.L, t.C, t.ld};
    }
};

// ---- deep levels: ResidualTemporalBlock as TWO dconv_kernel launches (kernels_dconv.h) --------------------------
//   A: y0 = Mish(GN(conv5(x) + b0)) + tbias_t  -> planes only;   r = Wr . x + br rides on A's centre tap
//   B: out = Mish(GN(conv5(y0) + b1)) + (x | r) -> fp32 (taps, attention, identity residuals) + planes (next conv)
static bool dconv_instantiated(int L, int k0, int k1, bool res) {
    if (L == 6) return (k0 == 1 && k1 == 0 && res) || (k0 == 2 && k1 == 0 && !res) || (k0 == 2 && k1 == 2 && res);
    if (L == 3) return (k0 == 2 && k1 == 0) || (k0 == 4 && k1 == 0) || (k0 == 4 && k1 == 4 && res);
    return false;
}

static void dconv_launch(Emitter& E, int L, int k0, int k1, bool res, const DconvArgs& d, double flops) {
    ++E.launches;
    if (E.dry) return;
    const int S = 48 / L;
    const dim3 grid((unsigned)d.NT, (unsigned)((d.Bp + S - 1) / S));
    const_cast<DconvArgs&>(d).dbg = E.h->O("dbg") >= 30 ? E.h->O("dbg") - 30 : 0;      // dbg 31..35: dconv phase ablations
    const_cast<DconvArgs&>(d).stress = E.h->O("stress");
    E.prof_begin(4, flops);
    if (E.prof) { E.prof->back().gx = grid.x; E.prof->back().gy = grid.y; E.prof->back().nstage = d.nch; }
    for (int rep = 0; rep < (E.prof ? Emitter::prof_reps : 1); ++rep) {
#define DC(L_, K0_, K1_, R_) KLAUNCH(E, (dconv_kernel<L_, K0_, K1_, R_>), grid, dim3(256), 0, d)
        if (L == 6) {
            if (k0 == 1) DC(6, 1, 0, true);
            else if (k1 == 2) DC(6, 2, 2, true);
            else DC(6, 2, 0, false);
        } else {
            if (k0 == 2 && res) DC(3, 2, 0, true);
            else if (k0 == 2) DC(3, 2, 0, false);
            else if (k1 == 4) DC(3, 4, 4, true);
            else if (res) DC(3, 4, 0, true);
            else DC(3, 4, 0, false);
        }
#undef DC
    }
    E.prof_end();
    E.note_error();
}

static void dsrc(DSrc& s, const Ten& t) { s.f32 = t.pl ? nullptr : t.p; s.planes = t.pl; s.pstride = t.pst; s.C = t.C; s.ld = t.ld; }

static bool dconv_applicable(cindm_unet1d* h, const std::string& p, const Ten& x0, const Ten* x1, int cout) {
    if (!h->O("dconv") || !h->use_h3 || !h->O("local_gn")) return false;
    const int L = x0.L, gw = cout / 8;
    if ((L != 3 && L != 6) || cout % 32 || (gw != 16 && gw != 32 && gw != 64)) return false;
    if (gw == 64 && ((cout / 32) % 2 || h->NX())) return false;
    if (x0.C % 128 || (x1 && (x1->C % 128 || x1->L != L))) return false;
    if (x0.ld != x0.C || (x1 && x1->ld != x1->C)) return false;      // (every tensor that reaches a block has an fp32 copy)
    auto w0 = h->packed.find(p + ".blocks.0.block.0"), w1 = h->packed.find(p + ".blocks.1.block.0");
    if (w0 == h->packed.end() || w1 == h->packed.end() || !w0->second.h3 || !w1->second.h3) return false;
    const bool identity = !h->packed.count(p + ".residual_conv");
    if (!identity && !h->packed.count(p + ".residual_conv#h3")) return false;
    const int k0 = x0.C / 128, k1 = x1 ? x1->C / 128 : 0;
    if (w0->second.CinP != (k0 + k1) * 128 || w1->second.CinP != cout || cout % 128) return false;
    return dconv_instantiated(L, k0, k1, !identity) && dconv_instantiated(L, cout / 128, 0, false);
}

// ---- deep levels: the whole ResidualTemporalBlock as ONE dconv2_kernel launch (kernels_dconv.h; option "dconv2") --------
static bool dconv2_instantiated(int L, int k0, int k1, bool res, int kb) {
    if (L == 6) return kb == 2 && ((k0 == 1 && k1 == 0 && res) || (k0 == 2 && k1 == 0 && !res) || (k0 == 2 && k1 == 2 && res));
    if (L == 3) return (kb == 4 && ((k0 == 2 && k1 == 0 && res) || (k0 == 4 && k1 == 0 && !res) || (k0 == 4 && k1 == 4 && res))) ||
                       (kb == 2 && k0 == 4 && k1 == 0 && res);
    return false;
}

static Ten emit_rtb_dconv2(Emitter& E, const std::string& p, const Ten& x0, const Ten* x1, int cout) {
    cindm_unet1d* h = E.h;
    const int Bp = (int)E.rows, L = x0.L, S = 48 / L, gw = cout / 8, NT = cout / 32;
    const int tiles = (Bp + S - 1) / S;
    const Packed& w0 = h->packed.at(p + ".blocks.0.block.0");
    const Packed& w1 = h->packed.at(p + ".blocks.1.block.0");
    const bool identity = !h->packed.count(p + ".residual_conv");
    const int k0 = x0.C / 128, k1 = x1 ? x1->C / 128 : 0, kb = cout / 128;
    Ten y0; y0.L = L; y0.C = cout; y0.ld = cout; E.planes(y0);
    Ten out = E.ten(L, cout); E.planes(out);
    unsigned long long* fl = E.xchg((size_t)tiles * NT);
    unsigned long long* xa = gw == 64 ? E.xchg((size_t)tiles * NT * 32) : nullptr;
    unsigned long long* xb = gw == 64 ? E.xchg((size_t)tiles * NT * 32) : nullptr;
    E.need_epoch();
    ++E.launches;
    {   // L2 warm-up registration: both convolutions' weights, tiled by n-tile
        cindm_unet1d::WReg r{};
        const size_t t0 = w0.sz * 4 / (size_t)NT, t1 = w1.sz * 4 / (size_t)NT;
        // dconv2_kernel's workgroup mapping: a column of NT workgroups spreads over XS XCDs, 4 workgroups on each (NT = 16: XS = 4, NT = 8:
        // XS = 2 -- scanned, same process: config 2 316.6 us per step with the identity mapping, 309.4 with XS = 4 / 4, 307.3 with 4 / 2, 307.7
        // with 2 / 2, 312.6 with 4 / 8; config 3 799.8 / 779.6 / 774.9); a coarser spread where the number of m-tiles does not divide
        int XS = NT / 4;
        while (XS >= 1 && XS < 8 && tiles % (8 / XS) != 0) XS *= 2;
        const bool remap = (XS == 2 || XS == 4) && NT % XS == 0 && tiles % (8 / XS) == 0;
        if (NT % 8 == 0 && !(h->O("tune") & 1)) {
            // round 6: conv A's fragments only, n-tiles x AND x + 8 of XCD x (through round 5: tile x of conv A and of conv B -- half of a
            // 512-channel layer's tiles were never warmed, and conv B's lines were touched a whole launch phase before their use).  Under the
            // workgroup mapping above XCD x streams the tiles (x % XS) + XS k: x and x + 8 are two of its four.  All four as pieces of one
            // region -- built, alternating processes against this: 304.7 -> 307.5 us per step: the touches cost their issuer more than the
            // other two tiles bring -- so two it stays.
            r.off[0] = w0.off * 4; r.bytes[0] = (unsigned)t0; r.stride[0] = (unsigned)t0;
            if (NT >= 16) { r.off[1] = w0.off * 4 + 8 * t0; r.bytes[1] = (unsigned)t0; r.stride[1] = (unsigned)t0; }
        }
        else if (NT % 8 == 0) { r.off[0] = w0.off * 4; r.bytes[0] = (unsigned)t0; r.stride[0] = (unsigned)t0;
                           r.off[1] = w1.off * 4; r.bytes[1] = (unsigned)t1; r.stride[1] = (unsigned)t1;
                         }
        else { r.off[0] = w0.off * 4; r.bytes[0] = (unsigned)std::min(w0.sz * 4, (size_t)2 << 20); }
        E.pf_issue = p != "downs.3.1";              // (see Emitter::pf_issue)
        Pf pf; E.pf_step(pf, r);
        E.pf_issue = true;
        if (E.dry) { E.drop(y0); return out; }
        Dconv2Args d;
        std::memset(&d, 0, sizeof(d));
        d.pf = pf;
        dsrc(d.src[0], x0); if (x1) dsrc(d.src[1], *x1);
        d.Wa = reinterpret_cast<const uint4*>(E.W(w0)); d.bias_a = E.B(w0); d.ncha = w0.CinP / 128;
        d.Wb = reinterpret_cast<const uint4*>(E.W(w1)); d.bias_b = E.B(w1);
        if (!identity) {
            const Packed& rc = h->packed.at(p + ".residual_conv#h3");
            d.W2 = reinterpret_cast<const uint4*>(E.W(rc)); d.bias2 = E.B(rc);
        } else { d.res = x0.p; d.ldres = x0.ld; }
        d.Bp = Bp; d.N = cout; d.NT = NT; d.gw = gw;
        d.gamma_a = E.V(p + ".blocks.0.block.2.weight"); d.beta_a = E.V(p + ".blocks.0.block.2.bias");
        d.gamma_b = E.V(p + ".blocks.1.block.2.weight"); d.beta_b = E.V(p + ".blocks.1.block.2.bias");
        d.tb = h->ttable + h->tb_off.at(p); d.tb_ld = h->tb_ld; d.t_ptr = E.t_ptr; d.t_imm = E.t_imm;
        d.y0 = y0.pl; d.y0_pstride = y0.pst; d.flags = reinterpret_cast<unsigned*>(fl);
        d.out_f32 = out.p; d.ldo = out.ld; d.out_planes = out.pl; d.out_pstride = out.pst;
        d.xchg_a = xa; d.xchg_b = xb; d.epoch = h->ep(); d.err_flag = h->epoch_dev + 1;
        d.stress = h->O("stress"); d.dbg = h->O("dbg") >= 30 ? h->O("dbg") - 30 : 0;
        d.tune = h->O("tune");
        d.xs = remap ? XS : 0;
        d.ph = E.ph_next("dconv2<" + std::to_string(L) + "," + std::to_string(k0) + "," + std::to_string(k1) + "," + (identity ? "false" : "true") + "," +
                         std::to_string(kb) + "> " + p);
        const dim3 grid((unsigned)NT, (unsigned)tiles);
        const double cin = (double)x0.C + (x1 ? (double)x1->C : 0.0);
        E.prof_begin(4, 2.0 * Bp * L * cout * cin * (5.0 + (identity ? 0.0 : 1.0)) + 2.0 * Bp * L * cout * (double)cout * 5.0);
        if (E.prof) { E.prof->back().gx = grid.x; E.prof->back().gy = grid.y; E.prof->back().nstage = d.ncha + kb; }
#define DC2(L_, K0_, K1_, R_, KB_) KLAUNCH(E, (dconv2_kernel<L_, K0_, K1_, R_, KB_>), grid, dim3(256), 0, d)
        if (L == 6) {
            if (k0 == 1) DC2(6, 1, 0, true, 2);
            else if (k1 == 2) DC2(6, 2, 2, true, 2);
            else DC2(6, 2, 0, false, 2);
        } else {
            if (k0 == 2) DC2(3, 2, 0, true, 4);
            else if (k1 == 4) DC2(3, 4, 4, true, 4);
            else if (kb == 2) DC2(3, 4, 0, true, 2);
            else DC2(3, 4, 0, false, 4);
        }
#undef DC2
        E.prof_end();
        E.note_error();
    }
    E.drop(y0);
    E.tap(p, out);
    return out;
}

static Ten emit_rtb_dconv(Emitter& E, const std::string& p, const Ten& x0, const Ten* x1, int cout) {
    cindm_unet1d* h = E.h;
    const int Bp = (int)E.rows, L = x0.L, S = 48 / L, gw = cout / 8, NT = cout / 32;
    const int tiles = (Bp + S - 1) / S;
    const Packed& w0 = h->packed.at(p + ".blocks.0.block.0");
    const Packed& w1 = h->packed.at(p + ".blocks.1.block.0");
    const bool identity = !h->packed.count(p + ".residual_conv");
    if (h->O("dconv2") && !h->NX() && dconv2_instantiated(L, x0.C / 128, x1 ? x1->C / 128 : 0, !identity, cout / 128) &&
        w0.CinP / 128 == x0.C / 128 + (x1 ? x1->C / 128 : 0))
        return emit_rtb_dconv2(E, p, x0, x1, cout);
    Ten y0; y0.L = L; y0.C = cout; y0.ld = cout; E.planes(y0);
    Ten out = E.ten(L, cout); E.planes(out);
    Ten r; if (!identity) r = E.ten(L, cout);
    auto pair_setup = [&](DconvArgs& d) {
        if (gw != 64) return;
        d.xchg = E.xchg((size_t)tiles * NT * 32);
        d.epoch = h->ep(); d.err_flag = h->epoch_dev + 1;
        E.need_epoch();
    };
    const double cin = (double)x0.C + (x1 ? (double)x1->C : 0.0);
    DconvArgs d;
    // A
    std::memset(&d, 0, sizeof(d));
    dsrc(d.src[0], x0); if (x1) dsrc(d.src[1], *x1);
    d.W = reinterpret_cast<const uint4*>(E.W(w0)); d.bias = E.B(w0); d.nch = w0.CinP / 128;
    d.Bp = Bp; d.N = cout; d.NT = NT; d.gw = gw;
    d.gamma = E.V(p + ".blocks.0.block.2.weight"); d.beta = E.V(p + ".blocks.0.block.2.bias");
    d.tb = h->ttable + h->tb_off.at(p); d.tb_ld = h->tb_ld; d.t_ptr = E.t_ptr; d.t_imm = E.t_imm;
    d.out_planes = y0.pl; d.out_pstride = y0.pst;
    if (!identity) {
        const Packed& rc = h->packed.at(p + ".residual_conv#h3");
        d.W2 = reinterpret_cast<const uint4*>(E.W(rc)); d.bias2 = E.B(rc); d.out2 = r.p; d.ldo2 = r.ld;
    }
    pair_setup(d);
    E.pf_tiled(d.pf, w0, NT);
    dconv_launch(E, L, x0.C / 128, x1 ? x1->C / 128 : 0, !identity, d, 2.0 * Bp * L * cout * cin * (5.0 + (identity ? 0.0 : 1.0)));
    // B
    std::memset(&d, 0, sizeof(d));
    dsrc(d.src[0], y0);
    d.W = reinterpret_cast<const uint4*>(E.W(w1)); d.bias = E.B(w1); d.nch = w1.CinP / 128;
    d.Bp = Bp; d.N = cout; d.NT = NT; d.gw = gw;
    d.gamma = E.V(p + ".blocks.1.block.2.weight"); d.beta = E.V(p + ".blocks.1.block.2.bias");
    d.t_ptr = E.t_ptr; d.t_imm = E.t_imm;
    if (identity) { d.res = x0.p; d.ldres = x0.ld; } else { d.res = r.p; d.ldres = r.ld; }
    d.out_f32 = out.p; d.ldo = out.ld; d.out_planes = out.pl; d.out_pstride = out.pst;
    pair_setup(d);
    E.pf_tiled(d.pf, w1, NT);
    dconv_launch(E, L, cout / 128, 0, false, d, 2.0 * Bp * L * cout * (double)cout * 5.0);
    E.drop(y0);
    if (!identity) E.drop(r);
    E.tap(p, out);
    return out;
}

// GroupNorm(8, C) partial statistics of an [*, L, C] tensor as the GEMM kernels write and merge them (kernels.h): one (mean, M2)
// partial per (sample, group, segment of seg = gcd(gw, 32) channels) -- the whole group up to gw = 32, its 32-column tiles at the wider
// powers of two, and at gw = 3 * 2^k (dim = 96: 12, 24, 48, 96) three segments of 4, 8, 16, 32 channels that straddle neither a tile
// nor a group.  tile_local: whole groups inside a 32-column tile, which is what producer-side activation ("local_gn") needs.
struct GnPart { int gw, P; float cnt; bool tile_local; };
static GnPart gn_part(int C, int L) {
    const int gw = C / 8;
    int seg = gw & -gw;
    if (seg > TN) seg = TN;
    return {gw, gw / seg, (float)(L * seg), gw == seg};
}

// ResidualTemporalBlock (model/diffusion_1d.py:483-511) as three launches:
//   A: y0 = conv5(x) + b0                      (+ GroupNorm partial stats of y0)
//   B: y1 = conv5(Mish(GN(y0)) + tbias_t) + b1 (normalise-on-load; + stats of y1)
//   C: out = Mish(GN(y1)) + (Wr x + br | x)    (1x1 GEMM or epilogue-only; + LayerNorm row partials)
static Ten emit_rtb(Emitter& E, const std::string& p, const Ten& x0, const Ten* x1, int cout, bool want_ln, float** ln_out) {
    cindm_unet1d* h = E.h;
    if (!want_ln && dconv_applicable(h, p, x0, x1, cout)) return emit_rtb_dconv(E, p, x0, x1, cout);
    const int Bp = (int)E.rows, L = x0.L;
    const GnPart gp = gn_part(cout, L);
    const int gw = gp.gw, Pn = gp.P;
    const float cnt = gp.cnt;
    if (gw % 4 && E.err == hipSuccess) E.err = hipErrorInvalidValue;      // the loaders' float4 of four adjacent channels lies in one group
    const Packed& w0 = h->packed.at(p + ".blocks.0.block.0");
    const Packed& w1 = h->packed.at(p + ".blocks.1.block.0");
    Ten out = E.ten(L, cout), y0 = E.ten(L, cout), y1 = E.ten(L, cout);
    Emitter::Tmp k0, k1;
    float* st0 = E.tmp((size_t)Bp * 8 * Pn * 2, k0);
    float* st1 = E.tmp((size_t)Bp * 8 * Pn * 2, k1);
    GemmArgs a;
    // GroupNorm groups inside one 32-column tile (cout <= 256): the producers normalise + activate their own output
    const bool local_gn = gp.tile_local && h->O("local_gn");
    auto rc = h->packed.find(p + ".residual_conv");
    const bool identity = rc == h->packed.end();
    // the 1x1 residual_conv rides on launch A's centre tap (split-fp16 kernel only): r = Wr . x + br
    auto rc3 = h->packed.find(p + ".residual_conv#h3");
    const bool fused_res = !identity && rc3 != h->packed.end() && w0.h3;
    Ten r;
    if (fused_res) r = E.ten(L, cout);
    // A
    E.base(a, w0, Bp, L, L);
    Emitter::plain(a.src[0], x0);
    if (x1) { Emitter::plain(a.src[1], *x1); a.nsrc = 2; }
    a.out = y0.p; a.ldo = y0.ld; a.so_gw = gw;
    if (fused_res) {
        a.W2 = E.W(rc3->second); a.bias2 = E.B(rc3->second); a.out2 = r.p; a.ldo2 = r.ld;
    }
    if (local_gn) {          // y0 <- Mish(GN(conv(x))) + tbias_t
        a.act_gamma = E.V(p + ".blocks.0.block.2.weight"); a.act_beta = E.V(p + ".blocks.0.block.2.bias");
        a.act_tb = h->ttable + h->tb_off.at(p); a.act_tb_ld = h->tb_ld;
    } else {
        a.stats_out = st0;
    }
    E.launch(5, a);
    // B
    E.base(a, w1, Bp, L, L);
    Src& s = a.src[0];
    if (local_gn) {
        Emitter::plain(s, y0);
    } else {
        s.p = y0.p; s.ld = y0.ld; s.C = cout; s.mode = SRC_GN_MISH; s.stats = st0; s.P = Pn; s.gw = gw; s.cnt = cnt;
        s.gamma = E.V(p + ".blocks.0.block.2.weight"); s.beta = E.V(p + ".blocks.0.block.2.bias");
        s.tb = h->ttable + h->tb_off.at(p); s.tb_ld = h->tb_ld;
    }
    a.so_gw = gw;
    if (local_gn && (identity || fused_res)) {
        // out <- Mish(GN(conv(h))) + (x | r): the whole tail of the block in B's epilogue, no third launch
        a.act_gamma = E.V(p + ".blocks.1.block.2.weight"); a.act_beta = E.V(p + ".blocks.1.block.2.bias");
        if (identity) { a.res = x0.p; a.ldres = x0.ld; } else { a.res = r.p; a.ldres = r.ld; }
        a.out = out.p; a.ldo = out.ld;
        if (want_ln) { *ln_out = E.alloc((size_t)Bp * L * (ceil_to(cout, TN) / TN) * 2); a.ln_out = *ln_out; }
        E.launch(5, a);
        E.drop(y0); E.drop(y1); E.drop(k0); E.drop(k1);
        if (fused_res) E.drop(r);
        E.tap(p, out);
        return out;
    }
    a.out = y1.p; a.ldo = y1.ld; a.stats_out = st1;
    E.launch(5, a);
    // C
    if (!identity && !fused_res) {
        E.base(a, rc->second, Bp, L, L);
        Emitter::plain(a.src[0], x0);
        if (x1) { Emitter::plain(a.src[1], *x1); a.nsrc = 2; }
    } else {
        Packed none; none.T = 0; none.CinP = 0; none.Npad = ceil_to(cout, TN); none.N = cout; none.KC = 32;
        E.base(a, none, Bp, L, L);
        a.W = nullptr; a.bias = nullptr; a.pad = 0;
        Emitter::plain(a.src[0], x0);
        if (identity) { a.res = x0.p; a.ldres = x0.ld; } else { a.res = r.p; a.ldres = r.ld; }
    }
    a.e_y = y1.p; a.e_ld = y1.ld; a.e_stats = st1; a.e_P = Pn; a.e_gw = gw; a.e_cnt = cnt;
    a.e_gamma = E.V(p + ".blocks.1.block.2.weight"); a.e_beta = E.V(p + ".blocks.1.block.2.bias");
    a.out = out.p; a.ldo = out.ld;
    if (want_ln) { *ln_out = E.alloc((size_t)Bp * L * (ceil_to(cout, TN) / TN) * 2); a.ln_out = *ln_out; }
    E.launch((identity || fused_res) ? 0 : 1, a);
    E.drop(y0); E.drop(y1); E.drop(k0); E.drop(k1);
    if (fused_res) E.drop(r);
    E.tap(p, out);
    return out;
}

// Residual(PreNorm(LinearAttentionTemporal)) (model/diffusion_1d.py:75-81, :123-142, :272-291):
//   qkv = Wqkv (LN(x) * g)  [LayerNorm applied on load from the producer's row partials]
//   per (sample, head) softmax / context / out (linattn_core_kernel)
//   out = Wo att + bo + x
static Ten emit_attn(Emitter& E, const std::string& p, const Ten& x, const float* lnp) {
    cindm_unet1d* h = E.h;
    const int Bp = (int)E.rows, L = x.L, C = x.C;
    const Packed& wq = h->packed.at(p + ".fn.fn.to_qkv");
    const Packed& wo = h->packed.at(p + ".fn.fn.to_out");
    GemmArgs a;
    auto site = h->packed.find(p + ".fn.fn.to_qkv#site");
    if (site != h->packed.end() && site->second.h3 && h->O("attn_head") && !h->NX() && (C == 512 || (C == 256 && (L <= 4 || h->O("attn_head") > 1))) && L <= 16 && x.ld == C) {
        // (at C = 256 with two samples per group the site kernel is faster: 10.6 vs 12.2 us, measured; attn_head = 2 forces this path)
        // heads split over workgroups (attn1d_head_kernel): grid (4 heads, sample groups)
        Ten out = E.ten(L, C);
        const int slot = ceil_to(L, 4), S = 16 / slot, groups = (Bp + S - 1) / S;
        unsigned long long* xg = E.xchg((size_t)groups * 2048);
        E.need_epoch();
        ++E.launches;
        Pf pfs;
        E.pf_issue = false;                        // (see Emitter::pf_issue)
        E.pf_all(pfs, {&site->second, &h->packed.at(p + ".fn.fn.to_out#site")}, {});
        E.pf_issue = true;
        if (!E.dry) {
            AttnHeadArgs s;
            std::memset(&s, 0, sizeof(s));
            s.pf = pfs;
            s.x = x.p; s.ldx = x.ld; s.out = out.p; s.ldo = out.ld; s.g = E.V(p + ".fn.norm.g");
            s.Wqkv = E.W(site->second); s.Wo = E.W(h->packed.at(p + ".fn.fn.to_out#site")); s.bo = E.B(h->packed.at(p + ".fn.fn.to_out"));
            s.L = L; s.S = S; s.slot = slot; s.Bp = Bp;
            s.xchg = xg; s.epoch = h->ep(); s.err_flag = h->epoch_dev + 1;
            s.stress = h->O("stress");
            s.ph = E.ph_next("attn1d_head<" + std::to_string(C) + "> " + p);
            const dim3 grid(4, (unsigned)groups);
            E.profiled(5, 2.0 * Bp * L * 1024.0 * C + (double)Bp * 4 * (2.0 * 32 * 32 * L * 2), [&] {
                if (C == 256) KLAUNCH(E, attn1d_head_kernel<256>, grid, dim3(256), 0, s);
                else KLAUNCH(E, attn1d_head_kernel<512>, grid, dim3(256), 0, s);
            });
            E.note_error();
        }
        E.tap(p, out);
        return out;
    }
    if (site != h->packed.end() && L <= 32) {
        // the whole site in one launch: one sample per workgroup (attn1d_site_kernel)
        Ten out = E.ten(L, C);
        ++E.launches;
        Pf pfs;
        E.pf_all(pfs, {&site->second, &h->packed.at(p + ".fn.fn.to_out#site")}, {});
        if (!E.dry) {
            AttnSiteArgs s;
            s.pf = pfs;
            s.x = x.p; s.ldx = x.ld; s.out = out.p; s.ldo = out.ld; s.g = E.V(p + ".fn.norm.g");
            s.Wqkv = E.W(site->second); s.Wo = E.W(h->packed.at(p + ".fn.fn.to_out#site")); s.bo = E.B(h->packed.at(p + ".fn.fn.to_out"));
            s.L = L; s.Bp = Bp;
            s.dbg = 0;
            s.ph = site->second.h3 ? E.ph_next("attn1d_site<" + std::to_string(C) + "> " + p) : PhaseBuf{nullptr, 0};
            // samples per workgroup: as many 4-aligned slots as fit one 16-position tile (weights are streamed once
            // per workgroup); CINDM_SITE_PACK=0 keeps one sample per workgroup
            const int pack = 1;
            const int NTsel = (L > 16) ? 2 : 1;
            s.slot = (L > 16) ? 32 : ceil_to(L, 4);
            s.S = (L > 16 || !pack) ? 1 : 16 / s.slot;
            const dim3 grid((unsigned)((Bp + s.S - 1) / s.S));
            E.profiled(5, 2.0 * Bp * L * 1024.0 * C + (double)Bp * 4 * (2.0 * 32 * 32 * L * 2), [&] {
#define SITE_LAUNCH(C_, NT_, PF_) KLAUNCH(E, (attn1d_site_kernel<C_, NT_, PF_>), grid, dim3(256), 0, s)
#define SITE_LAUNCH_H3(C_, NT_, PF_) KLAUNCH(E, (attn1d_site_h3_kernel<C_, NT_, PF_>), grid, dim3(256), 0, s)
                if (site->second.h3) {
                    if (NTsel == 2) {
                        if (C == 64) SITE_LAUNCH_H3(64, 2, 2); else if (C == 128) SITE_LAUNCH_H3(128, 2, 3);
                        else if (C == 256) SITE_LAUNCH_H3(256, 2, 3); else SITE_LAUNCH_H3(512, 2, 3);
                    } else {
                        if (C == 64) SITE_LAUNCH_H3(64, 1, 2); else if (C == 128) SITE_LAUNCH_H3(128, 1, 3);
                        else if (C == 256) SITE_LAUNCH_H3(256, 1, 3); else SITE_LAUNCH_H3(512, 1, 3);
                    }
                } else if (NTsel == 2) {
                    if (C == 64) SITE_LAUNCH(64, 2, 4); else if (C == 128) SITE_LAUNCH(128, 2, 4);
                    else if (C == 256) SITE_LAUNCH(256, 2, 4); else SITE_LAUNCH(512, 2, 4);
                } else {
                    if (C == 64) SITE_LAUNCH(64, 1, 4); else if (C == 128) SITE_LAUNCH(128, 1, 4);
                    else if (C == 256) SITE_LAUNCH(256, 1, 4); else SITE_LAUNCH(512, 1, 4);
                }
#undef SITE_LAUNCH
#undef SITE_LAUNCH_H3
            });
        }
        E.tap(p, out);
        return out;
    }
    Ten out = E.ten(L, C), qkv = E.ten(L, 384), att = E.ten(L, 128);       // three-launch path: q|k|v and the attention output are temporaries
    auto wide = h->packed.find(p + ".fn.fn.to_qkv#wide");
    if (wide != h->packed.end()) {
        // shallow levels (C = 64 / 128): 64-row tiles, the LayerNorm-ed input tile staged once per workgroup and its
        // fragments kept in registers over a group of output tiles (the 2-D path's projection kernel on [rows, C])
        ++E.launches;
        { Pf none; E.pf_all(none, {&wide->second}, {}); }
        if (!E.dry) {
            const int64_t rows = (int64_t)Bp * L;
            Conv2dArgs c2;
            std::memset(&c2, 0, sizeof(c2));
            Src& s2 = c2.src[0];
            s2.p = x.p; s2.ld = x.ld; s2.C = C; s2.mode = SRC2_LN; s2.stats = lnp; s2.P = ceil_to(C, TN) / TN; s2.cnt = (float)TN; s2.gw = 1;
            s2.gamma = E.V(p + ".fn.norm.g");
            c2.nsrc = 1; c2.W = E.W(wide->second); c2.CinP = C; c2.Npad = wide->second.Npad; c2.N = 384;
            c2.out = qkv.p; c2.ldo = qkv.ld; c2.rows_total = rows;
            const int mt = (int)((rows + 63) / 64);
            const int ntile = c2.Npad / 64;                      // 6
            int groups = 1;
            for (int g : {1, 2, 3, 6}) { groups = g; if (mt * g >= 256) break; }       // enough workgroups to fill the chip
            c2.tiles_per_group = ntile / groups;
            const dim3 g1((unsigned)mt, (unsigned)groups);
            E.profiled(1, 2.0 * rows * 384.0 * C, [&] {
                if (C == 64) KLAUNCH(E, (conv1x1_wide_kernel<64, SRC2_LN, true, false>), g1, dim3(256), 0, c2);
                else if (c2.tiles_per_group >= 3) KLAUNCH(E, (conv1x1_wide_kernel<128, SRC2_LN, true, false>), g1, dim3(256), 0, c2);
                else KLAUNCH(E, (conv1x1_wide_kernel<128, SRC2_LN, false, false>), g1, dim3(256), 0, c2);
            });
        }
    } else {
        E.base(a, wq, Bp, L, L);
        Src& s = a.src[0];
        s.p = x.p; s.ld = x.ld; s.C = C; s.mode = SRC_LN; s.stats = lnp; s.P = ceil_to(C, TN) / TN; s.cnt = (float)TN; s.gw = 1;
        s.gamma = E.V(p + ".fn.norm.g");
        a.out = qkv.p; a.ldo = qkv.ld;
        E.launch(1, a);
    }
    ++E.launches;
    { Pf none; E.pf_all(none, {}, {}); }
    if (!E.dry) {
        const size_t shm = 4 * (size_t)(3 * L * 32 + 32 * 33) * sizeof(float);
        static bool attr_set = false;
        if (!attr_set) {       // horizons > 32 need more than the default 64 KiB of dynamic LDS
            (void)hipFuncSetAttribute(reinterpret_cast<const void*>(linattn_core_kernel),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024);
            attr_set = true;
        }
        E.profiled(5, (double)Bp * 4 * (2.0 * 32 * 32 * L * 2),        // context + out contractions
                   [&] { KLAUNCH(E, linattn_core_kernel, dim3((unsigned)Bp), dim3(256), shm, qkv.p, att.p, L); });
    }
    E.base(a, wo, Bp, L, L);
    Emitter::plain(a.src[0], att);
    a.res = x.p; a.ldres = x.ld;
    a.out = out.p; a.ldo = out.ld;
    E.launch(1, a);
    E.drop(qkv); E.drop(att);
    E.tap(p, out);
    return out;
}

static Ten emit_resample(Emitter& E, const std::string& p, const Ten& x, bool up) {
    cindm_unet1d* h = E.h;
    const Packed& w = h->packed.at(p + ".conv");
    const int Lout = up ? x.L * 2 : x.L / 2;
    Ten out = E.ten(Lout, x.C);
    if (h->O("dresample") && h->O("dconv") && w.h3 && x.C == 256 && x.ld == x.C && x.L == (up ? 3 : 6) && w.CinP == x.C && w.T == (up ? 4 : 3)) {
        // the resampling convolutions between the deep levels on dresample_kernel (LDS-resident tile, planes for the next layer)
        const int Bp = (int)E.rows, NT = x.C / 32, tiles = (Bp + 15) / 16;
        E.planes(out);
        ++E.launches;
        // workgroup mapping (kernels_dconv.h): a column's 2 NT (NT) workgroups on XS XCDs; n-tile idx % NT of XCD x: idx = x % XS (mod XS)
        // (not on the exchange-free plan -- i.e. not for a chain that shares the device with another one: with 16 columns per workgroup TWO
        // workgroups write the two 64-byte halves of every 128-byte fp32 output line, that plan reads those rows, and this is the best lead for
        // the demoted chain's last-bit differences under contention -- DESIGN 4.12; 32 columns per workgroup = whole lines per workgroup)
        const bool half = h->O("dresample") >= 2 && NT % 8 == 0 && NT * tiles < 256 && !h->NX();
        // (2 XCDs per column: 305.0 -> 303.7 us per step, config 3 768.0 -> 764.7; 4: 304.7 / 768.2)
        int XS = 2;
        while (XS >= 1 && XS < 8 && tiles % (8 / XS) != 0) XS *= 2;
        if (!(XS == 2 || XS == 4) || (half ? 2 * NT : NT) % XS != 0 || (h->O("tune") & 1)) XS = 0;
        Pf pf;
        E.pf_tiled(pf, w, NT);
        if (!E.dry) {
            DresArgs d;
            std::memset(&d, 0, sizeof(d));
            d.pf = pf;
            d.x = x.p; d.ld = x.ld; d.W = reinterpret_cast<const uint4*>(E.W(w)); d.bias = E.B(w); d.nch = w.CinP / 128;
            d.Bp = Bp; d.N = x.C; d.NT = NT; d.out_f32 = out.p; d.ldo = out.ld; d.out_planes = out.pl; d.out_pstride = out.pst;
            d.ph = E.ph_next(std::string("dresample<") + (up ? "up" : "down") + "> " + p);
            // "dresample" = 2 (default): 16 columns per workgroup where 32 would leave CUs idle (2 NT x tiles = 256 workgroups at 256 rows:
            // 320.2 -> 317.2 us per step; at 768 rows the 32-column grid is 384 workgroups already and the split costs 2 us); 1: always 32
            d.xs = XS;
            const dim3 grid((unsigned)(half ? 2 * NT : NT), (unsigned)tiles);
            E.prof_begin(up ? 3 : 2, 2.0 * Bp * Lout * x.C * (double)x.C * (up ? 2.0 : 3.0));
            if (E.prof) { E.prof->back().gx = grid.x; E.prof->back().gy = grid.y; E.prof->back().nstage = d.nch; }
            if (half) {
                if (up) KLAUNCH(E, (dresample_kernel<true, 2, 2>), grid, dim3(256), 0, d);
                else KLAUNCH(E, (dresample_kernel<false, 2, 2>), grid, dim3(256), 0, d);
            } else {
                if (up) KLAUNCH(E, (dresample_kernel<true, 2, 1>), grid, dim3(256), 0, d);
                else KLAUNCH(E, (dresample_kernel<false, 2, 1>), grid, dim3(256), 0, d);
            }
            E.prof_end();
            E.note_error();
        }
        E.tap(p, out);
        return out;
    }
    GemmArgs a;
    E.base(a, w, (int)E.rows, x.L, Lout);
    a.pad = 1;
    if (up) a.transposed = 1; else a.stride = 2;
    Emitter::plain(a.src[0], x);
    a.out = out.p; a.ldo = out.ld;
    E.launch(up ? 4 : 3, a);
    E.tap(p, out);
    return out;
}

// ---- the sample-local level kernels (kernels.h): one workgroup runs a whole level of one sample ----------------------------------
// Does the kernel serve level `ind`, whose input is `x` (ups_last: and whose skip is `*skip`; ups_tail: `x` is the output of the
// level's first block)?  One shape for the four; level0 is also asked about the forward's input before there is a tensor.
static bool level0_serves(const cindm_unet1d* h, int ind, const Ten& x, const Ten*) {
    const LevelSpec& s = h->lvl[LV_LEVEL0];
    return ind == 0 && s.ok && h->d.attention != 0 && x.L <= 32 && (x.L & 1) == 0 && s.qkv && s.qkv->h3 && x.ld == x.C;
}
static bool level1_serves(const cindm_unet1d* h, int ind, const Ten& x, const Ten*) {
    const LevelSpec& s = h->lvl[LV_LEVEL1];
    return ind == 1 && h->O("level1") && s.ok && h->d.attention != 0 && x.L <= 16 && (x.L & 1) == 0 && x.C == 64 && x.ld == 64 && s.qkv && s.qkv->h3;
}
static bool ups_last_serves(const cindm_unet1d* h, int ind, const Ten& x, const Ten* skip) {
    const LevelSpec& s = h->lvl[LV_UPS_LAST];
    return h->O("ups_last") && ind == h->d.n_mults - 2 && s.ok && h->d.attention != 0 && x.L <= 16 && x.C == 128 && x.ld == 128 &&
           skip->C == 128 && skip->ld == 128 && s.qkv && s.qkv->h3 && h->packed.count(s.frag(FRAG_RESAMPLE).p);
}
static bool ups_tail_serves(const cindm_unet1d* h, int ind, const Ten& x, const Ten*) {
    const LevelSpec& s = h->lvl[LV_UPS_TAIL];
    const int nres = h->d.n_mults;
    return h->O("ups_tail") && ind == nres - 3 && s.ok && h->d.attention != 0 && x.L <= 8 && x.C == 256 && x.ld == 256 && h->dims[nres - 1 - ind] == 128 &&
           s.qkv && s.qkv->h3 && h->packed.count(s.frag(FRAG_RESAMPLE).p);
}

// does level0_down_kernel consume the forward's INPUT tensor?  (run_step asks before it decides to let that kernel read the sampler's
// state in place instead of launching compose_gather_kernel)
static bool level0_serves_input(const cindm_unet1d* h) {
    Ten x; x.L = h->d.horizon; x.C = x.ld = h->d.transition_dim;
    return level0_serves(h, 0, x, nullptr);
}

// The members every level kernel's argument struct has: the Conv1dBlocks in the order of Wc[], the attention site, the time step,
// the level's length, the L2 warm-up and the phase-clock slot.  What only some of the kernels have stays next to their launch.
template <typename A>
static void level_args(Emitter& E, const LevelSpec& s, const Pf& pf, int L, A& l) {
    const float* blob = E.h->blob;
    std::memset(&l, 0, sizeof(l));
    l.pf = pf;
    int i = 0;
    for (const LevelFrag& f : s.frags)
        if (f.role == FRAG_CONV) { l.Wc[i] = E.W(*f.w); l.bc[i] = E.B(*f.b); l.gam[i] = blob + f.gam; l.bet[i] = blob + f.bet; ++i; }
    l.ln_g = blob + s.ln_g; l.Wqkv = E.W(*s.qkv); l.Wo = E.W(*s.wo); l.bo = E.B(*s.bo);
    l.tb_ld = E.h->tb_ld;
    l.t_ptr = E.t_ptr; l.t_imm = E.t_imm; l.L = L;
    l.ph = E.ph_next(s.label);
}
// ... and what Level0Args and Level1Args name alike: the first block's residual_conv, Downsample1d, both blocks' time bias
template <typename A>
static void level_down_args(Emitter& E, const LevelSpec& s, A& l) {
    const LevelFrag &r = s.frag(FRAG_RES), &dw = s.frag(FRAG_RESAMPLE);
    l.Wr = E.W(*r.w); l.br = E.B(*r.b); l.Wd = E.W(*dw.w); l.bd = E.B(*dw.b);
    l.tb0 = E.h->ttable + s.tb[0]; l.tb1 = E.h->ttable + s.tb[1];
}

// Level pairs (option "level_pairs"): the two launch boundaries of the step with ONE sample per workgroup on both sides -- level0_down ->
// level1_down and ups_tail128 -> ups_last -- are fused when BOTH stand-alone kernels would run and a workgroup has a CU to itself (at most
// 320 rows; above, level0 / level1 run two workgroups per CU and the pair's LDS would not allow that).  The first stage's emitter fills
// its arguments and leaves them pending here; the second stage's emitter launches the pair.  Decided in the emitters and nowhere else: the
// launch count of a forward changes by the same amount whatever the step driver does around it.
template <typename Pair>
struct PairSlot {
    bool pending = false;
    Pair args;
    // first stage: `fuse` = the pair will run; its launch is counted here either way
    void first(Emitter& E, bool fuse) { pending = fuse; ++E.launches; }
    // the tensor between the stages stays in registers inside the pair: it goes to memory only for the tap API
    float* handover(const Ten& t, bool taps) const { return (pending && !taps) ? nullptr : t.p; }
    template <typename A, typename Alone> void launch_first(Emitter& E, const A& l, Alone alone) {
        if (pending) args.l0 = l; else E.profiled(5, 0.0, alone);
    }
    // second stage: counted only when it runs alone (the pair is the launch counted by its first stage)
    void second(Emitter& E) { if (!pending) ++E.launches; }
    template <typename A, typename Both, typename Alone> void launch_second(Emitter& E, const A& l, Both both, Alone alone) {
        if (pending) args.l1 = l;
        E.profiled(5, 0.0, [&] { if (pending) both(args); else alone(); });
    }
};

// one emission of the forward: the tensor the chain has reached, the skips, and the two pair slots
struct Fwd {
    Emitter& E;
    cindm_unet1d* h;
    const bool taps;              // tap-only block outputs of the level kernels (tests); off on the sampling path
    const bool pairs;
    float* eps;
    Ten cur;
    bool cur_is_skip = false;
    std::vector<Ten> skips;
    float* lnp = nullptr;
    PairSlot<Level01Args> p01;
    PairSlot<UpsTailLastArgs> pul;
    // the chain moves on: the tensor left behind is dead unless it is a skip (or the caller's input)
    void move_to(const Ten& next, bool next_is_skip = false) { if (!cur_is_skip) E.drop(cur); cur = next; cur_is_skip = next_is_skip; }
    // LayerNorm row partials from the producer are only needed where the attention site is not one fused launch
    bool need_ln(const std::string& ap, int L) const { return h->d.attention != 0 && !(h->packed.count(ap + ".fn.fn.to_qkv#site") && L <= 32); }

    // the whole level in one launch (level0_down_kernel)
    void emit_level0() {
        const LevelSpec& s = h->lvl[LV_LEVEL0];
        const int L = cur.L;
        Ten h1, h2;
        if (taps) { h1 = E.ten(L, 64); h2 = E.ten(L, 64); }
        Ten sk = E.ten(L, 64), dn = E.ten(L / 2, 64);
        p01.first(E, pairs && h->d.n_mults > 1 && h->O("level1") == 1 && level1_serves(h, 1, dn, nullptr));
        const Pf pf = E.pf_level(s);
        if (!E.dry) {
            Level0Args l;
            level_args(E, s, pf, L, l); level_down_args(E, s, l);
            l.x = cur.p; l.F = cur.C; l.h1 = h1.p; l.h2 = h2.p; l.skip = sk.p; l.down = p01.handover(dn, taps);       // (h1, h2: null without taps)
            l.gB = h->gatherB; l.gcs = h->gather_cs; l.gLtot = h->gather_Ltot;
            const dim3 grid((unsigned)E.rows);
            p01.launch_first(E, l, [&] {
                if (L > 16 && E.rows > 320) KLAUNCH(E, (level0_down_kernel<2, 2>), grid, dim3(256), 0, l);
                else if (L > 16) KLAUNCH(E, level0_down_kernel<2>, grid, dim3(256), 0, l);
                else KLAUNCH(E, level0_down_kernel<1>, grid, dim3(256), 0, l);
            });
        }
        if (taps) { E.tap("downs.0.0", h1); E.tap("downs.0.1", h2); }
        E.tap("downs.0.2", sk); E.tap("downs.0.3", dn);
        skips.push_back(sk);
        move_to(dn);
    }

    // the second level in one launch (level1_down_kernel), or the pair level0 + level1 (level01_down_kernel)
    void emit_level1() {
        const LevelSpec& s = h->lvl[LV_LEVEL1];
        const int L = cur.L;
        Ten h1, h2;
        if (taps) { h1 = E.ten(L, 128); h2 = E.ten(L, 128); }
        Ten sk = E.ten(L, 128), dn = E.ten(L / 2, 128);
        p01.second(E);
        const Pf pf = E.pf_level(s);
        if (!E.dry) {
            Level1Args l;
            level_args(E, s, pf, L, l); level_down_args(E, s, l);
            l.x = cur.p; l.h1 = h1.p; l.h2 = h2.p; l.skip = sk.p; l.down = dn.p;
            l.Bp = (int)E.rows;
            const int S = h->O("level1") == 1 ? 1 : 2;       // samples per workgroup
            const dim3 grid((unsigned)((E.rows + S - 1) / S));
            p01.launch_second(E, l, [&](const Level01Args& a01) {
                if (a01.l0.L > 16) KLAUNCH(E, level01_down_kernel<2>, grid, dim3(256), 0, a01);
                else KLAUNCH(E, level01_down_kernel<1>, grid, dim3(256), 0, a01);
            }, [&] {
                if (S == 1 && E.rows > 320) KLAUNCH(E, (level1_down_kernel<1, 2>), grid, dim3(256), 0, l);
                else if (S == 1) KLAUNCH(E, level1_down_kernel<1>, grid, dim3(256), 0, l);
                else KLAUNCH(E, level1_down_kernel<2>, grid, dim3(256), 0, l);
            });
        }
        p01.pending = false;
        if (taps) { E.tap("downs.1.0", h1); E.tap("downs.1.1", h2); }
        E.tap("downs.1.2", sk); E.tap("downs.1.3", dn);
        skips.push_back(sk);
        move_to(dn);
    }

    // the rest of level nres - 3 behind its first block in one launch (ups_tail128_kernel)
    void emit_ups_tail(int ind) {
        const LevelSpec& s = h->lvl[LV_UPS_TAIL];
        const std::string p = "ups." + std::to_string(ind);
        const int L = cur.L;
        Ten h2, h3;
        if (taps) { h2 = E.ten(L, 128); h3 = E.ten(L, 128); }
        Ten up = E.ten(2 * L, 128);
        pul.first(E, pairs && !skips.empty() && ups_last_serves(h, ind + 1, up, &skips.back()));
        const Pf pf = E.pf_level(s);
        if (!E.dry) {
            UpsTailArgs l;
            level_args(E, s, pf, L, l);
            const LevelFrag &r = s.frag(FRAG_RES), &u = s.frag(FRAG_RESAMPLE);
            l.Wr = E.W(*r.w); l.br = E.B(*r.b); l.Wu = E.W(*u.w); l.bu = E.B(*u.b);
            l.tb = h->ttable + s.tb[0];
            l.x = cur.p; l.h2 = h2.p; l.h3 = h3.p; l.up = pul.handover(up, taps);
            pul.launch_first(E, l, [&] { KLAUNCH(E, ups_tail128_kernel, dim3((unsigned)E.rows), dim3(256), 0, l); });
        }
        if (taps) { E.tap(p + ".1", h2); E.tap(p + ".2", h3); }
        E.tap(p + ".3", up);
        move_to(up);
    }

    // the finest up level and the output head in one launch (ups_last_kernel), or the pair ups_tail128 + ups_last (ups_tail_last_kernel)
    void emit_ups_last(int ind, const Ten& skip) {
        const LevelSpec& s = h->lvl[LV_UPS_LAST];
        const int L = cur.L;
        Ten h1, h2, h3, up, ypre;
        if (taps) { h1 = E.ten(L, 128); h2 = E.ten(L, 64); h3 = E.ten(L, 64); up = E.ten(2 * L, 64); ypre = E.ten(2 * L, 64); }
        pul.second(E);
        const Pf pf = E.pf_level(s);
        if (!E.dry) {
            UpsLastArgs l;
            level_args(E, s, pf, L, l);
            const LevelFrag &r0 = s.frag(FRAG_RES, 0), &r1 = s.frag(FRAG_RES, 1), &u = s.frag(FRAG_RESAMPLE), &hd = s.frag(FRAG_HEAD);
            l.Wr0 = E.W(*r0.w); l.br0 = E.B(*r0.b); l.Wr1 = E.W(*r1.w); l.br1 = E.B(*r1.b);
            l.Wu = E.W(*u.w); l.bu = E.B(*u.b); l.Wf = E.W(*hd.w); l.bf = E.B(*hd.b);
            l.tb0 = h->ttable + s.tb[0]; l.tb1 = h->ttable + s.tb[1];
            l.x = cur.p; l.skip = skip.p; l.eps = eps; l.F = h->d.transition_dim;
            l.h1 = h1.p; l.h2 = h2.p; l.h3 = h3.p; l.up = up.p; l.ypre = ypre.p;          // tap-only outputs of the last level (null without taps)
            if (h->fuse_upd && !E.prof) { l.fuse_upd = 1; l.upd = *h->fuse_upd; h->fused_done = true; }
            const dim3 grid((unsigned)E.rows);
            pul.launch_second(E, l, [&](const UpsTailLastArgs& aul) { KLAUNCH(E, ups_tail_last_kernel, grid, dim3(256), 0, aul); },
                                [&] { KLAUNCH(E, ups_last_kernel, grid, dim3(256), 0, l); });
        }
        pul.pending = false;
        if (taps) {
            const std::string p = "ups." + std::to_string(ind);
            E.tap(p + ".0", h1); E.tap(p + ".1", h2); E.tap(p + ".2", h3); E.tap(p + ".3", up); E.tap("final_conv.0.pre", ypre);
        }
    }

    // final_conv: Conv1dBlock(dim, dim, 5) then Conv1d(dim, F, 1) (:605-608)
    void emit_head() {
        const int Bp = (int)E.rows, L = cur.L, C = h->d.dim;
        const GnPart gp = gn_part(C, L);
        const int gw = gp.gw, Pn = gp.P;
        const float cnt = gp.cnt;
        Ten y0 = E.ten(L, C);
        float* st0 = E.alloc((size_t)Bp * 8 * Pn * 2);
        GemmArgs a;
        E.base(a, h->packed.at("final_conv.0.block.0"), Bp, L, L);
        Emitter::plain(a.src[0], cur);
        a.out = y0.p; a.ldo = y0.ld; a.stats_out = st0; a.so_gw = gw;
        E.launch(5, a);
        E.tap("final_conv.0.pre", y0);
        E.base(a, h->packed.at("final_conv.1"), Bp, L, L);
        Src& s = a.src[0];
        s.p = y0.p; s.ld = y0.ld; s.C = C; s.mode = SRC_GN_MISH; s.stats = st0; s.P = Pn; s.gw = gw; s.cnt = cnt;
        s.gamma = E.V("final_conv.0.block.2.weight"); s.beta = E.V("final_conv.0.block.2.bias");
        a.out = eps; a.ldo = h->d.transition_dim;
        E.launch(1, a);
    }
};

// The forward as the network reads (:610-646): down levels, middle, up levels, head.  A level is one level kernel where that
// kernel serves it, else ResidualTemporalBlocks (emit_rtb), the attention site (emit_attn) and the resampling (emit_resample).
static int emit_forward(Emitter& E, const float* x, float* eps) {
    cindm_unet1d* h = E.h;
    const auto& d = h->d;
    const int nres = d.n_mults;
    const bool att = d.attention != 0;
    const bool taps = h->O("taps") != 0;
    Fwd f{E, h, taps, h->O("level_pairs") != 0 && E.rows <= 320, eps};
    f.cur.p = const_cast<float*>(x); f.cur.L = d.horizon; f.cur.C = d.transition_dim; f.cur.ld = d.transition_dim;
    // "ws_alias": 0 never, 2 always, 1 (default) when the un-recycled workspace would not fit the Infinity Cache next to the
    // weights (more than 320 rows: 0.6 MB per row + 83 MB against 256 MiB).  Measured same-box: 768 rows (config 3) 918 -> 910 us
    // per step, 768 + 512 rows (config 4) 647 -> 628; at 256 rows recycling COSTS 3 us per step (364.6 -> 367.5), so it stays off there.
    E.reuse = !taps && (h->O("ws_alias") == 2 || (h->O("ws_alias") == 1 && E.rows > 320));
    E.free_blocks.clear();
    for (int ind = 0; ind < nres; ++ind) {
        if (level0_serves(h, ind, f.cur, nullptr)) { f.emit_level0(); continue; }
        if (level1_serves(h, ind, f.cur, nullptr)) { f.emit_level1(); continue; }
        const int co = h->dims[ind + 1];
        const std::string p = "downs." + std::to_string(ind);
        f.move_to(emit_rtb(E, p + ".0", f.cur, nullptr, co, false, nullptr));
        f.move_to(emit_rtb(E, p + ".1", f.cur, nullptr, co, f.need_ln(p + ".2", f.cur.L), &f.lnp));
        if (att) f.move_to(emit_attn(E, p + ".2", f.cur, f.lnp));
        f.skips.push_back(f.cur);
        f.cur_is_skip = true;
        if (h->packed.count(p + ".3.conv")) f.move_to(emit_resample(E, p + ".3", f.cur, false));
    }
    // (the last down level has no resampling: its skip is also the tensor the middle blocks read, and stays a skip)
    f.move_to(emit_rtb(E, "mid_block1", f.cur, nullptr, h->dims[nres], f.need_ln("mid_attn", f.cur.L), &f.lnp));
    if (att) f.move_to(emit_attn(E, "mid_attn", f.cur, f.lnp));
    f.move_to(emit_rtb(E, "mid_block2", f.cur, nullptr, h->dims[nres], false, nullptr));
    for (int ind = 0; ind < nres - 1; ++ind) {
        const int ci = h->dims[nres - 1 - ind], co = h->dims[nres - ind];
        Ten skip = f.skips.back(); f.skips.pop_back();
        if (E.dry && getenv("CINDM_VERBOSE")) fprintf(stderr, "[cindm] ups ind %d nres %d ok %d att %d L %d C %d ld %d sC %d sld %d\n", ind, nres, (int)h->lvl[LV_UPS_LAST].ok, (int)att, f.cur.L, f.cur.C, f.cur.ld, skip.C, skip.ld);
        if (ups_last_serves(h, ind, f.cur, &skip)) { f.emit_ups_last(ind, skip); return 0; }      // (the head is inside the kernel)
        const std::string p = "ups." + std::to_string(ind);
        f.move_to(emit_rtb(E, p + ".0", f.cur, &skip, co, false, nullptr));       // torch.cat((x, h.pop()), dim=1) :637
        E.drop(skip);
        if (ups_tail_serves(h, ind, f.cur, nullptr)) { f.emit_ups_tail(ind); continue; }
        f.move_to(emit_rtb(E, p + ".1", f.cur, nullptr, ci, f.need_ln(p + ".2", f.cur.L), &f.lnp));
        if (att) f.move_to(emit_attn(E, p + ".2", f.cur, f.lnp));
        if (h->packed.count(p + ".3.conv")) f.move_to(emit_resample(E, p + ".3", f.cur, true));
    }
    f.emit_head();
    return 0;
}

// count the launches of one forward and collect what each of them streams (L2 warm-up table), for the kernel paths the
// handle's options select NOW (the exchange-free mode is a run-time switch: re-planned when it flips)
static void unet1d_plan(cindm_unet1d* h) {
    h->pf_table.clear();
    std::vector<cindm_unet1d::WReg> regs;
    Emitter D = Emitter::dry_run(h, 1);
    D.pf_out = &regs;
    emit_forward(D, nullptr, nullptr);
    h->launches = D.launches;
    h->pf_table = regs;
    h->plan_nx = h->NX() ? 1 : 0;
}

static int unet1d_finalize_pack(cindm_unet1d* h, void* stream_) {
    REQUIRE(h, "null handle");
    hipStream_t stream = (hipStream_t)stream_;
    for (auto& p : h->params) if (!p.set) return fail("missing key in state_dict: " + p.name);
    h->pf_table.clear();                   // (offsets into the blob that is rebuilt below)
    const auto& d = h->d;
    const int T = d.timesteps, dim = d.dim;
    if (h->sinus.empty()) {
        // SinusoidalPosEmb (:151-158) with libm, fp32 throughout.
        h->sinus.resize((size_t)T * dim);
        const int half = dim / 2;
        const float e = (float)(std::log(10000.0) / (half - 1));
        for (int t = 0; t < T; ++t)
            for (int i = 0; i < half; ++i) {
                const float f = expf((float)i * -e);
                const float arg = (float)t * f;
                h->sinus[(size_t)t * dim + i] = sinf(arg);
                h->sinus[(size_t)t * dim + half + i] = cosf(arg);
            }
    }
    BlobBuilder bb;
    h->use_h3 = !h->O("mfma_f32") && !h->force_f32;
    // Range rule of the split-fp16 products: a checkpoint with a conv / projection weight outside the window of
    // max_abs_in_fp16_window runs on the exact fp32 MFMA kernels instead ("range_fallback" reads 1); "auto_range" = 0
    // disables the check.  Activations need no rule: they are GroupNorm / LayerNorm outputs of O(gamma), and an input
    // beyond 65504 shows up as inf / nan in the output rather than as a silent loss.
    h->opt["range_fallback"] = h->force_f32 ? (h->force_reason ? h->force_reason : 2) : 0;
    if (h->use_h3 && h->O("auto_range")) {
        for (const auto& p : h->params) {
            if (p.shape.size() < 2 || p.name.find("time_mlp") != std::string::npos) continue;      // time path: fp32 kernels at finalize
            if (!max_abs_in_fp16_window(p.host)) { h->use_h3 = false; h->opt["range_fallback"] = 1; break; }
        }
    }
    h->packed.clear(); h->vec_off.clear(); h->tb_off.clear();
    for (LevelSpec& s : h->lvl) s = LevelSpec{};       // (they point into h->packed)
    std::vector<RtbDesc> rtbs;
    int tb_ld = 0;
    for (const auto& p : h->params) {
        const std::string& k = p.name;
        auto ends = [&](const char* s) { size_t n = std::strlen(s); return k.size() >= n && k.compare(k.size() - n, n, s) == 0; };
        if (ends(".block.0.weight")) {
            std::string pre = k.substr(0, k.size() - 7);
            int split = 0;
            if (k.rfind("ups.", 0) == 0 && k.find(".0.blocks.0.") != std::string::npos) split = (int)p.shape[1] / 2;
            pack_weight(h, bb, pre, 0, split);
        } else if (ends(".residual_conv.weight")) {
            int split = (k.rfind("ups.", 0) == 0 && k.find(".0.residual_conv") != std::string::npos) ? (int)p.shape[1] / 2 : 0;
            pack_weight(h, bb, k.substr(0, k.size() - 7), 0, split);
            if (h->use_h3 && h->O("local_gn")) pack_weight_h3_res(h, bb, k.substr(0, k.size() - 7), split);
        } else if (ends(".3.conv.weight")) {
            pack_weight(h, bb, k.substr(0, k.size() - 7), k.rfind("ups.", 0) == 0 ? 1 : 0, 0);
        } else if (ends("to_qkv.weight") || ends("to_out.weight") || k == "final_conv.1.weight") {
            pack_weight(h, bb, k.substr(0, k.size() - 7), 0, 0);
            if (ends("to_qkv.weight")) pack_weight_wide(h, bb, k.substr(0, k.size() - 7));
            if (ends("to_out.weight") && h->O("attn_site")) pack_attn_site(h, bb, k.substr(0, k.size() - std::strlen(".to_out.weight")));
        } else if (ends("time_mlp.1.weight") || k == "time_mlp.3.weight") {
            pack_weight(h, bb, k.substr(0, k.size() - 7), 2, 0);
            if (k != "time_mlp.1.weight" && k != "time_mlp.3.weight") {
                std::string rp = k.substr(0, k.size() - std::strlen(".time_mlp.1.weight"));
                h->tb_off[rp] = tb_ld;
                rtbs.push_back({rp, 0, (int)p.shape[0], tb_ld});
                tb_ld += ceil_to((int)p.shape[0], TN);
            }
        } else if (ends(".block.2.weight") || ends(".block.2.bias") || ends(".norm.g")) {
            pack_vec(h, bb, k);
        }
    }
    h->tb_ld = tb_ld;
    if (h->use_h3 && h->O("attn_site") && h->O("level0") && h->O("local_gn")) pack_level0(h, bb);
    if (getenv("CINDM_VERBOSE")) fprintf(stderr, "[cindm] fused levels: level0 %d level1 %d ups_last %d\n", (int)h->lvl[LV_LEVEL0].ok, (int)h->lvl[LV_LEVEL1].ok, (int)h->lvl[LV_UPS_LAST].ok + 2 * (int)h->lvl[LV_UPS_TAIL].ok);
    if (h->blob) { (void)hipFree(h->blob); h->blob = nullptr; }
    if (h->ttable) { (void)hipFree(h->ttable); h->ttable = nullptr; }
    h->blob_floats = bb.data.size();
    HIPCHK(hipMalloc((void**)&h->blob, bb.data.size() * sizeof(float)));
    HIPCHK(hipMemcpy(h->blob, bb.data.data(), bb.data.size() * sizeof(float), hipMemcpyHostToDevice));
    HIPCHK(hipMalloc((void**)&h->ttable, (size_t)T * tb_ld * sizeof(float)));
    if (!h->epoch_dev) { HIPCHK(hipMalloc((void**)&h->epoch_dev, 256)); HIPCHK(hipMemset(h->epoch_dev, 0, 256)); }
    h->seen_ws = nullptr; h->seen_rows = 0;
    HIPCHK(hipMemsetAsync(h->ttable, 0, (size_t)T * tb_ld * sizeof(float), stream));

    // ---- time path for every timestep with the GEMM kernel ("samples" = timesteps, L = 1) ----
    float *sin_d = nullptr, *y1 = nullptr, *temb = nullptr;
    HIPCHK(hipMalloc((void**)&sin_d, (size_t)T * dim * sizeof(float)));
    HIPCHK(hipMalloc((void**)&y1, (size_t)T * dim * 4 * sizeof(float)));
    HIPCHK(hipMalloc((void**)&temb, (size_t)T * dim * sizeof(float)));
    HIPCHK(hipMemcpyAsync(sin_d, h->sinus.data(), (size_t)T * dim * sizeof(float), hipMemcpyHostToDevice, stream));
    Emitter E = Emitter::live(h, stream, nullptr, T, nullptr, 0);
    GemmArgs a;
    Ten ts; ts.p = sin_d; ts.L = 1; ts.C = dim; ts.ld = dim;
    E.base(a, h->packed.at("time_mlp.1"), T, 1, 1);
    Emitter::plain(a.src[0], ts); a.out = y1; a.ldo = dim * 4;
    E.launch(1, a);
    E.base(a, h->packed.at("time_mlp.3"), T, 1, 1);
    a.src[0].p = y1; a.src[0].ld = dim * 4; a.src[0].C = dim * 4; a.src[0].mode = SRC_MISH; a.src[0].P = 1; a.src[0].gw = 1;
    a.out = temb; a.ldo = dim;
    E.launch(1, a);
    for (const auto& r : rtbs) {
        E.base(a, h->packed.at(r.p + ".time_mlp.1"), T, 1, 1);
        a.src[0].p = temb; a.src[0].ld = dim; a.src[0].C = dim; a.src[0].mode = SRC_MISH; a.src[0].P = 1; a.src[0].gw = 1;
        a.out = h->ttable + r.tb_off; a.ldo = tb_ld;
        E.launch(1, a);
    }
    if (E.err != hipSuccess) return fail(std::string("finalize launch: ") + hipGetErrorString(E.err));
    HIPCHK(hipStreamSynchronize(stream));
    (void)hipFree(sin_d); (void)hipFree(y1); (void)hipFree(temb);
    h->generation = ++g_generation;
    h->finalized = true;
    unet1d_plan(h);
    return 0;
}

extern "C" size_t cindm_unet1d_workspace_bytes(const cindm_unet1d* h, int64_t rows);
extern "C" int cindm_unet1d_forward(cindm_unet1d* h, const float* x, int32_t t, const int32_t* t_dev,
                                    float* eps, int64_t rows, void* ws, size_t ws_bytes, void* stream);
static int unet1d_check_flag(cindm_unet1d* h, hipStream_t stream);

// Repack + time tables (unet1d_finalize_pack), then -- on the split-fp16 kernels with "auto_range" -- ONE calibration
// forward per timestep in {0, T/2, T-1} on a fixed unit-scale batch: an activation that leaves fp16's exponent range
// (large un-normalised residual streams, huge projection weights) shows up as inf / nan in eps, and the handle is
// repacked for the exact fp32 MFMA kernels ("range_fallback" reads 2; 1 = the weight-window rule fired).
// A handle that is finalized already (nothing changed since its last finalize) returns at once.
extern "C" int cindm_unet1d_finalize(cindm_unet1d* h, void* stream_) {
    REQUIRE(h, "null handle");
    if (h->finalized) return 0;
    h->force_f32 = false; h->force_reason = 0;
    if (unet1d_finalize_pack(h, stream_) != 0) return -1;
    if (!h->use_h3 || !h->O("auto_range")) return 0;
    hipStream_t stream = (hipStream_t)stream_;
    const int64_t rows = 4;
    const int F = h->d.transition_dim;
    const size_t wsb = cindm_unet1d_workspace_bytes(h, rows);
    auto fwd = [&](int t, const float* x, float* eps, void* ws) { return cindm_unet1d_forward(h, x, t, nullptr, eps, rows, ws, wsb, stream_); };
    bool finite = true;
    if (calibrate_at_finalize((size_t)rows * h->d.horizon * F, F, F, 0x2545F491u, h->d.timesteps, wsb, stream, fwd, &finite) != 0) return -1;
    h->seen_ws = nullptr; h->seen_rows = 0; h->taps.clear();
    if (unet1d_check_flag(h, stream) != 0) return -1;      // a calibration forward whose exchange timed out proves nothing
    if (!finite) {
        h->force_f32 = true; h->force_reason = 2;
        if (unet1d_finalize_pack(h, stream_) != 0) return -1;
    }
    return 0;
}

// The range rule on the CALLER's data (round 6).  The calibration above sees one synthetic unit-scale batch; a real checkpoint's
// residual stream can still leave fp16's exponent range on real inputs, which shows as inf / nan in the result -- never as a silently
// wrong finite value.  The Python face checks the result of the FIRST forward / chain after every weight synchronisation and, when it is
// not finite, calls this with on = 1: the handle is repacked for the exact fp32-MFMA kernels ("range_fallback" reads 3) and the call is
// repeated; on = 0 undoes exactly that (the repeat was not finite either: the cause was not the range).  Synchronises the stream.
extern "C" int cindm_unet1d_range_escalate(cindm_unet1d* h, int32_t on, void* stream_) {
    REQUIRE(h && h->finalized, "model not finalized");
    if (on) {
        if (h->force_f32 || !h->use_h3) return 0;
        h->force_f32 = true; h->force_reason = 3;
    } else {
        if (!h->force_f32 || h->force_reason != 3) return 0;
        h->force_f32 = false; h->force_reason = 0;
    }
    HIPCHK(hipStreamSynchronize((hipStream_t)stream_));
    return unet1d_finalize_pack(h, stream_);
}

// (the larger of the two kernel selections: a chain whose exchange timed out is re-run in exchange-free mode on the SAME
// caller-provided workspace)
extern "C" size_t cindm_unet1d_workspace_bytes(const cindm_unet1d* h_, int64_t rows) {
    cindm_unet1d* h = const_cast<cindm_unet1d*>(h_);
    if (!h || !h->finalized || rows <= 0) return 0;
    // cached per (pack generation, rows, the run-time "no_exchange" option): the eager entry points ask on every call
    // (cindm_unet1d_forward, twice more per run_step through step_layout) and the answer is two dry emissions of the forward
    {
        std::lock_guard<std::mutex> lk(h->wsb_mu);
        if (h->wsb_gen == h->generation && h->wsb_rows == rows && h->wsb_nx == h->O("no_exchange") && h->wsb_val) return h->wsb_val;
    }
    size_t need = 0;
    const int keep = h->no_xchg_force;
    for (int nx = 0; nx < 2; ++nx) {
        h->no_xchg_force = nx;
        if (nx == 0 && h->O("no_exchange")) continue;
        Emitter D = Emitter::dry_run(h, rows);
        emit_forward(D, nullptr, nullptr);
        need = std::max(need, D.ws_off);
    }
    h->no_xchg_force = keep;
    {
        std::lock_guard<std::mutex> lk(h->wsb_mu);
        h->wsb_gen = h->generation; h->wsb_rows = rows; h->wsb_nx = h->O("no_exchange"); h->wsb_val = need + 256;
    }
    return need + 256;
}

extern "C" int cindm_unet1d_launches_per_forward(const cindm_unet1d* h) { return h ? h->launches : 0; }

// The pair-exchange regions of a workspace must not hold a stale tag equal to the current epoch: clear them the first
// time a (workspace, rows) pair is seen (caller-owned memory arrives uninitialised).  Must run outside stream capture;
// the sample loops call it before they capture their step.
static int unet1d_prepare_ws(cindm_unet1d* h, void* ws, int64_t rows, hipStream_t stream) {
    if ((h->NX() ? 1 : 0) != h->plan_nx) { unet1d_plan(h); h->seen_ws = nullptr; }     // the exchange-free switch flipped: other launches, other regions
    if (h->seen_ws == ws && h->seen_rows == rows) return 0;
    std::vector<std::pair<size_t, size_t>> regions;
    Emitter D = Emitter::dry_run(h, rows);
    D.xregions = &regions;
    emit_forward(D, nullptr, nullptr);
    for (const auto& r : regions) HIPCHK(hipMemsetAsync((char*)ws + r.first, 0, r.second, stream));
    h->seen_ws = ws; h->seen_rows = rows;
    return 0;
}

// Error flag of the in-kernel exchanges (dconv_kernel's GroupNorm pairs, attn1d_head_kernel's head tiles): a partner
// that never arrived leaves garbage statistics behind, so every entry point that hands results to the caller after a
// synchronisation reads the flag (the sample loops once per chain; cindm_unet1d_status for the asynchronous calls).
// Synchronises the stream; clears the flag when it was set.  0 healthy, 1 timed out (flag cleared), < 0 error
static int unet1d_poll_flag(cindm_unet1d* h, hipStream_t stream) {
    if (!h || !h->epoch_dev) return 0;
    int v[2] = {0, 0};
    HIPCHK(hipMemcpyAsync(v, h->epoch_dev, sizeof(v), hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    if (!v[1]) return 0;
    HIPCHK(hipMemsetAsync(h->epoch_dev + 1, 0, sizeof(int), stream));
    HIPCHK(hipStreamSynchronize(stream));
    return 1;
}

// ... with the time-out as an error
static int unet1d_check_flag(cindm_unet1d* h, hipStream_t stream) {
    const int rc = unet1d_poll_flag(h, stream);
    return rc != 1 ? rc : fail("an in-kernel exchange between workgroups timed out (GroupNorm pair / attention head exchange): "
                               "the results of that forward are invalid");
}

extern "C" int cindm_unet1d_status(cindm_unet1d* h, void* stream) {
    REQUIRE(h, "null handle");
    return unet1d_check_flag(h, (hipStream_t)stream);
}

extern "C" int cindm_unet1d_poll(cindm_unet1d* h, void* stream) {
    REQUIRE(h, "null handle");
    return unet1d_poll_flag(h, (hipStream_t)stream);
}

extern "C" int cindm_unet1d_recovered(const cindm_unet1d* h) { return h ? h->recovered : 0; }

// ---- phase clocks (profiling builds) -----------------------------------------------------------------------------------
static constexpr size_t kPhSlots = 32;
static constexpr size_t kPhWordsPerSlot = (size_t)PH_MAXWG * PH_MAXWAVE * PH_NST;
extern "C" int cindm_unet1d_phase_prof_enable(cindm_unet1d* h, int32_t on) {
    REQUIRE(h, "null handle");
#ifndef CINDM_PHASE_PROF
    (void)on;
    return fail("not a profiling build: the phase clocks exist only in libcindm_hip_prof.so (python -m cindm_amd.build --prof)");
#else
    if (on && !h->ph_buf) HIPCHK(hipMalloc((void**)&h->ph_buf, kPhSlots * kPhWordsPerSlot * sizeof(unsigned long long)));
    if (on) HIPCHK(hipMemset(h->ph_buf, 0, kPhSlots * kPhWordsPerSlot * sizeof(unsigned long long)));
    h->ph_on = on ? 1 : 0;
    h->ph_names.clear();
    h->generation = ++g_generation;          // captured steps embed the record pointers: never replay an older capture
    return 0;
#endif
}
extern "C" int cindm_unet1d_phase_prof_read(cindm_unet1d* h, unsigned long long* dst, int64_t dst_cap, void* stream) {
    REQUIRE(h && dst, "null argument");
    REQUIRE(h->ph_buf, "phase clocks are not enabled");
    const size_t n = h->ph_names.size() * kPhWordsPerSlot;
    REQUIRE((int64_t)n <= dst_cap, "phase clocks: destination too small");
    HIPCHK(hipStreamSynchronize((hipStream_t)stream));
    HIPCHK(hipMemcpy(dst, h->ph_buf, n * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return (int)h->ph_names.size();
}
extern "C" const char* cindm_unet1d_phase_prof_name(const cindm_unet1d* h, int32_t slot) {
    return (h && slot >= 0 && slot < (int)h->ph_names.size()) ? h->ph_names[slot].c_str() : "";
}

extern "C" int cindm_unet1d_forward(cindm_unet1d* h, const float* x, int32_t t, const int32_t* t_dev,
                                    float* eps, int64_t rows, void* ws, size_t ws_bytes, void* stream) {
    REQUIRE(h && x && eps && ws, "null argument");
    REQUIRE(h->finalized, "cindm_unet1d_finalize has not been called");
    REQUIRE(rows > 0 && rows <= 65535, "rows out of range (1..65535)");
    REQUIRE(t_dev || (t >= 0 && t < h->d.timesteps), "timestep out of range");
    REQUIRE(ws_bytes >= cindm_unet1d_workspace_bytes(h, rows), "workspace too small");
    REQUIRE(((uintptr_t)ws & 255) == 0 && ((uintptr_t)x & 15) == 0, "workspace must be 256-byte aligned, x 16-byte aligned");
    h->taps.clear(); h->taps_rows = rows;
    if (unet1d_prepare_ws(h, ws, rows, (hipStream_t)stream) != 0) return -1;
    Emitter E = Emitter::live(h, (hipStream_t)stream, ws, rows, t_dev, t);
    emit_forward(E, x, eps);
    h->issued = E.launches;
    if (E.err != hipSuccess) return fail(std::string("kernel launch: ") + hipGetErrorString(E.err));
    return 0;
}

// One forward with every launch under its own pair of events (Emitter::prof); each(record, ms) sees the launches in order.
template <typename Each>
static int unet1d_profiled_forward(cindm_unet1d* h, const float* x, int32_t t, float* eps, int64_t rows, void* ws, size_t ws_bytes,
                                   void* stream, Each each) {
    REQUIRE(h->finalized, "cindm_unet1d_finalize has not been called");
    REQUIRE(rows > 0 && rows <= 65535, "rows out of range (1..65535)");
    REQUIRE(t >= 0 && t < h->d.timesteps, "timestep out of range");
    REQUIRE(ws_bytes >= cindm_unet1d_workspace_bytes(h, rows), "workspace too small");
    std::vector<Emitter::ProfRec> recs;
    if (unet1d_prepare_ws(h, ws, rows, (hipStream_t)stream) != 0) return -1;
    Emitter E = Emitter::live(h, (hipStream_t)stream, ws, rows, nullptr, t);
    E.prof = &recs;
    h->taps.clear(); h->taps_rows = rows;
    emit_forward(E, x, eps);
    hipError_t se = hipStreamSynchronize((hipStream_t)stream);
    for (auto& r : recs) {
        float dt = 0.f;
        (void)hipEventElapsedTime(&dt, r.e0, r.e1);
        each(r, dt / Emitter::prof_reps);
        (void)hipEventDestroy(r.e0); (void)hipEventDestroy(r.e1);
    }
    if (E.err != hipSuccess) return fail(std::string("kernel launch: ") + hipGetErrorString(E.err));
    if (se != hipSuccess) return fail(std::string("hipStreamSynchronize: ") + hipGetErrorString(se));
    return 0;
}

extern "C" int cindm_unet1d_profile(cindm_unet1d* h, const float* x, int32_t t, float* eps, int64_t rows, void* ws,
                                    size_t ws_bytes, void* stream, int32_t counts[6], float ms[6], double flops[6]) {
    REQUIRE(h && x && eps && ws && counts && ms && flops, "null argument");
    for (int i = 0; i < 6; ++i) { counts[i] = 0; ms[i] = 0.f; flops[i] = 0.0; }
    return unet1d_profiled_forward(h, x, t, eps, rows, ws, ws_bytes, stream, [&](const Emitter::ProfRec& r, float dt) {
        counts[r.kind] += 1; ms[r.kind] += dt; flops[r.kind] += r.flops;
    });
}

extern "C" int cindm_unet1d_profile_detail(cindm_unet1d* h, const float* x, int32_t t, float* eps, int64_t rows, void* ws,
                                           size_t ws_bytes, void* stream, int32_t cap, int32_t* n_out, int32_t* kind,
                                           float* ms, double* flops, int32_t* grid_xy_stages) {
    REQUIRE(h && x && eps && ws && n_out && kind && ms && flops && grid_xy_stages, "null argument");
    int n = 0;
    const int rc = unet1d_profiled_forward(h, x, t, eps, rows, ws, ws_bytes, stream, [&](const Emitter::ProfRec& r, float dt) {
        if (n >= cap) return;
        kind[n] = r.kind; ms[n] = dt; flops[n] = r.flops;
        grid_xy_stages[3 * n] = r.gx; grid_xy_stages[3 * n + 1] = r.gy; grid_xy_stages[3 * n + 2] = r.nstage;
        ++n;
    });
    *n_out = n;
    return rc;
}

extern "C" int cindm_unet1d_tap(cindm_unet1d* h, const char* name, int64_t rows, void* ws, float* dst,
                                int64_t dst_cap, int64_t shape[3], void* stream) {
    REQUIRE(h && name && ws && dst, "null argument");
    REQUIRE(rows == h->taps_rows, "tap: rows differ from the last forward");
    auto it = h->taps.find(name);
    if (it == h->taps.end())
        return fail(std::string("unknown tap: ") + name + (h->O("taps") ? "" : " (block outputs inside the level kernels are stored only with set_option(\"taps\", 1))"));
    const auto& tp = it->second;
    const int64_t n = rows * tp.L * tp.C;
    REQUIRE(tp.ld == tp.C, "tap: strided tensor");
    REQUIRE(n <= dst_cap, "tap: destination too small");
    shape[0] = rows; shape[1] = tp.L; shape[2] = tp.C;
    HIPCHK(hipMemcpyAsync(dst, (char*)ws + tp.off, n * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return 0;
}
