// Host side of the 2-D airfoil path (included by cindm_hip.hip): launch sequence of the reference's 2-D Unet.forward
// (model/diffusion_2d.py:369-408) and of GaussianDiffusion.p_sample / p_sample_loop (:788-907) over kernels2d.h.

struct Packed2 {
    size_t off = 0, bias_off = 0; bool has_bias = false;
    int CinP = 0, Npad = 0, N = 0, kind = 0;
    bool h3 = false;          // 3x3 weights packed as split fp16 (conv2d_h3_kernel)
    bool identity = false;    // 1x1 kernel's identity mode: no weights
};

struct cindm_unet2d : ModelCore {
    cindm_unet2d_desc d;
    bool use_h3 = true;                                      // CINDM_MFMA=f32 selects the fp32-MFMA 3x3 kernel
    bool force_f32 = false;                                  // the calibration forward overflowed on the split-fp16 kernels
    std::vector<int> dims;
    float* blob = nullptr;
    std::unordered_map<std::string, Packed2> packed;        // convolutions
    std::unordered_map<std::string, Packed> lin;            // time-path linears (1-D GEMM kernel)
    std::unordered_map<std::string, size_t> vec_off;
    float* ttable = nullptr; int tt_ld = 0;                 // [T][tt_ld]: per ResnetBlock (scale C | shift C)
    std::unordered_map<std::string, int> tt_off;
    int launches = 0;
    struct Tap { size_t off; int HW, C; };
    std::unordered_map<std::string, Tap> taps;
    int64_t taps_imgs = 0;
    int CP() const { return ceil_to(d.channels, 4); }
};

static const OptDef kUnet2dOpts[] = {
    {"mfma_f32", 0, nullptr, OPT_PACK},          // 1: 3x3 convolutions / stem / attention products on the exact fp32 MFMA kernels
    {"la_site", 1, "CINDM_LA_SITE", OPT_PACK},   // LinearAttention sites without the q|k|v tensor
    {"ws_alias", 1, "CINDM_WS_ALIAS", OPT_PACK}, // block-internal temporaries share workspace (0: every intermediate keeps its own slice)
    {"tail_h3", 1, "CINDM_TAIL_H3", OPT_PACK},   // ResnetBlock tails with a res_conv GEMM on the split-fp16 products (0: fp32 MFMA)
    {"la_nsplit", 8, nullptr, OPT_PACK},         // LinearAttention context kernel at C = 64: workgroups (partial records) per image
    {"la_wpi", 32, nullptr, OPT_PACK},           // LinearAttention apply kernel at C = 64: workgroups per image (each loops over its share of 64-pixel tiles)
    {"ws_nosplit", 2, "CINDM_WS_NOSPLIT", OPT_PACK},   // conv2d_ws_kernel: K of a chunk not split over the matrix waves (no in-tile reduction; 0 = round 2's k-groups)
    {"conv_ws", 1, "CINDM_CONV_WS", OPT_PACK},   // 3x3 convolutions: persistent wave-specialised conv2d_ws_kernel; 0 = conv2d_h3_kernel
    {"stress", 0, "CINDM_STRESS", OPT_PACK},     // > 0 (a seed): pseudo-random pauses before the hand-overs inside conv2d_ws_kernel (race tests)
    {"auto_range", 1, "CINDM_AUTO_RANGE", OPT_PACK},
    {"range_fallback", 0, nullptr, OPT_READONLY},
    {"dbg2", 0, "CINDM_DBG2", OPT_PACK},
};

static int build_manifest2(cindm_unet2d* h) {
    const auto& d = h->d;
    const int dim = d.dim, tdim = dim * 4, hid = 128;
    h->dims.clear(); h->dims.push_back(dim);
    for (int i = 0; i < d.n_mults; ++i) h->dims.push_back(dim * d.dim_mults[i]);
    auto conv = [&](const std::string& p, int i, int o, int k, bool bias = true) {
        h->add_param(p + ".weight", {o, i, k, k});
        if (bias) h->add_param(p + ".bias", {o});
    };
    auto rb = [&](const std::string& p, int i, int o) {
        h->add_param(p + ".mlp.1.weight", {2 * o, tdim}); h->add_param(p + ".mlp.1.bias", {2 * o});
        conv(p + ".block1.proj", i, o, 3); h->add_param(p + ".block1.norm.weight", {o}); h->add_param(p + ".block1.norm.bias", {o});
        conv(p + ".block2.proj", o, o, 3); h->add_param(p + ".block2.norm.weight", {o}); h->add_param(p + ".block2.norm.bias", {o});
        if (i != o) conv(p + ".res_conv", i, o, 1);
    };
    auto lattn = [&](const std::string& p, int c) {
        conv(p + ".fn.fn.to_qkv", c, hid * 3, 1, false);
        conv(p + ".fn.fn.to_out.0", hid, c, 1);
        h->add_param(p + ".fn.fn.to_out.1.g", {1, c, 1, 1});
        h->add_param(p + ".fn.norm.g", {1, c, 1, 1});
    };
    conv("init_conv", d.channels, dim, 7);
    h->add_param("time_mlp.1.weight", {tdim, dim}); h->add_param("time_mlp.1.bias", {tdim});
    h->add_param("time_mlp.3.weight", {tdim, tdim}); h->add_param("time_mlp.3.bias", {tdim});
    const int n = d.n_mults;
    for (int ind = 0; ind < n; ++ind) {
        const int ci = h->dims[ind], co = h->dims[ind + 1];
        const std::string p = "downs." + std::to_string(ind);
        rb(p + ".0", ci, ci); rb(p + ".1", ci, ci); lattn(p + ".2", ci);
        if (ind < n - 1) conv(p + ".3.1", ci * 4, co, 1); else conv(p + ".3", ci, co, 3);
    }
    for (int ind = 0; ind < n; ++ind) {
        const int ci = h->dims[n - 1 - ind], co = h->dims[n - ind];
        const std::string p = "ups." + std::to_string(ind);
        rb(p + ".0", co + ci, co); rb(p + ".1", co + ci, co); lattn(p + ".2", co);
        if (ind < n - 1) conv(p + ".3.1", co, ci, 3); else conv(p + ".3", co, ci, 3);
    }
    const int mid = h->dims[n];
    rb("mid_block1", mid, mid);
    conv("mid_attn.fn.fn.to_qkv", mid, hid * 3, 1, false);
    conv("mid_attn.fn.fn.to_out", hid, mid, 1);
    h->add_param("mid_attn.fn.norm.g", {1, mid, 1, 1});
    rb("mid_block2", mid, mid);
    rb("final_res_block", dim * 2, dim);
    conv("final_conv", dim, d.channels, 1);
    return 0;
}

extern "C" int cindm_unet2d_create(const cindm_unet2d_desc* desc, cindm_unet2d** out) {
    REQUIRE(desc && out, "null argument");
    REQUIRE(desc->n_mults >= 1 && desc->n_mults <= 4, "n_mults out of range");
    REQUIRE(desc->dim == 64, "2-D Unet: dim must be 64 (GroupNorm group widths 8/16 are what the kernels tile for)");
    for (int i = 0; i < desc->n_mults; ++i) REQUIRE(desc->dim_mults[i] == 1 || desc->dim_mults[i] == 2, "2-D Unet: dim_mults entries must be 1 or 2");
    REQUIRE(desc->channels >= 4 && desc->channels <= 32, "channels must be in [4, 32]");
    REQUIRE(desc->image_size >= 16 && (desc->image_size & (desc->image_size - 1)) == 0 && desc->image_size <= 64,
            "image_size must be a power of two in [16, 64]");
    REQUIRE((desc->image_size >> (desc->n_mults - 1)) >= 16, "the coarsest level must be at least 16 x 16 (pixel tiles are 4 x 16)");
    REQUIRE(desc->channels <= 24, "channels must be <= 24 (the stem kernel stages 24 input channels)");
    REQUIRE(desc->timesteps >= 1, "timesteps must be >= 1");
    auto* h = new cindm_unet2d();
    h->d = *desc;
    h->init_options(kUnet2dOpts);
    build_manifest2(h);
    *out = h;
    return 0;
}
extern "C" int cindm_unet2d_get_option(const cindm_unet2d* h, const char* key, int32_t* value) { return core_get_option(h, key, value); }
extern "C" int cindm_unet2d_set_option(cindm_unet2d* h, const char* key, int32_t value) { return core_set_option(h, key, value) < 0 ? -1 : 0; }
extern "C" void cindm_unet2d_destroy(cindm_unet2d* h) {
    if (!h) return;
    if (h->blob) (void)hipFree(h->blob);
    if (h->ttable) (void)hipFree(h->ttable);
    delete h;
}
extern "C" int cindm_unet2d_num_params(const cindm_unet2d* h) { return core_num_params(h); }
extern "C" int cindm_unet2d_param_info(const cindm_unet2d* h, int idx, char* name, int cap, int64_t shape[4], int* ndim) {
    return core_param_info(h, idx, name, cap, shape, ndim);
}
extern "C" int cindm_unet2d_set_param(cindm_unet2d* h, const char* key, const float* src, int64_t numel, int on_device) {
    return core_set_param(h, key, src, numel, on_device);
}
extern "C" int cindm_unet2d_set_sinusoid_table(cindm_unet2d* h, const float* t, int64_t numel) {
    return core_set_sinusoid(h, t, numel, h ? (int64_t)h->d.timesteps * h->d.dim : 0);
}
extern "C" int cindm_unet2d_padded_channels(const cindm_unet2d* h) { return h ? h->CP() : 0; }

// ---- packing ---------------------------------------------------------------------------------------------
// fp32 fragment packing of the 1-D GEMM kernel (time-path linears): [n-tile of 32][stage][q][thread][4]
template <typename F>
static void pack_frag_f32(BlobBuilder& bb, size_t& off, int& CinP_out, int KC, int C0, int Co, F getw) {
    int C0p = ceil_to(C0, KC);
    int nst = C0p / KC;
    if (nst > 1 && (nst & 1)) C0p += KC;
    const int CinP = C0p;
    nst = CinP / KC;
    const int Npad = ceil_to(Co, TN), CPW = KC / 4, CS = CPW / 4;
    off = bb.alloc((size_t)(Npad / TN) * nst * 256 * 2 * CS);
    float* base = bb.data.data() + off;
    for (int nt = 0; nt < Npad / TN; ++nt)
        for (int st = 0; st < nst; ++st) {
            float* dst = base + ((size_t)nt * nst + st) * 256 * (2 * CS);
            for (int tid = 0; tid < 256; ++tid) {
                const int wv = tid >> 6, lane = tid & 63;
                for (int cs = 0; cs < CS; ++cs)
                    for (int nb = 0; nb < 2; ++nb) {
                        const int c = st * KC + wv * CPW + cs * 4 + (lane >> 4);
                        const int n = nt * TN + nb * 16 + (lane & 15);
                        const float v = (c < C0 && n < Co) ? getw(n, c) : 0.f;
                        const int jj = cs * 2 + nb;
                        dst[((size_t)(jj / 4) * 256 + tid) * 4 + (jj % 4)] = v;
                    }
            }
        }
    CinP_out = CinP;
}

// conv2d_tile_kernel packing: [n-tile of 64][stage = chunk*SPC + tap row][q = tap_in_stage*CS + cs][thread][nb];
// getw(n, c, tap) -> weight of output n, input channel c (of the concatenated sources), tap (0 outside the layer).
template <typename F>
static void pack_tile_f32(BlobBuilder& bb, Packed2& pk, int KC, int TPS, int SPC, int C0, int C1, int Co, F getw) {
    int C0p = ceil_to(C0, KC), C1p = C1 ? ceil_to(C1, KC) : 0;
    int nch = (C0p + C1p) / KC;
    if (nch > 1 && (nch & 1)) { if (C1) C1p += KC; else C0p += KC; }          // even chunk count (zero chunk)
    pk.CinP = C0p + C1p; nch = pk.CinP / KC;
    pk.N = Co; pk.Npad = ceil_to(Co, T2N);
    const int CPW = KC / 4, CS = CPW / 4, NBF = TPS * CS, nst = nch * SPC;
    pk.off = bb.alloc((size_t)(pk.Npad / T2N) * nst * 256 * NBF * 4);
    float* base = bb.data.data() + pk.off;
    for (int nt = 0; nt < pk.Npad / T2N; ++nt)
        for (int cc = 0; cc < nch; ++cc)
            for (int tr = 0; tr < SPC; ++tr) {
                float* dst = base + ((size_t)nt * nst + cc * SPC + tr) * 256 * NBF * 4;
                for (int tid = 0; tid < 256; ++tid) {
                    const int wv = tid >> 6, lane = tid & 63;
                    for (int j = 0; j < TPS; ++j)
                        for (int cs = 0; cs < CS; ++cs)
                            for (int nb = 0; nb < 4; ++nb) {
                                const int cp = cc * KC + wv * CPW + cs * 4 + (lane >> 4);
                                const int n = nt * T2N + nb * 16 + (lane & 15);
                                int c = -1;
                                if (cp < C0) c = cp;
                                else if (cp >= C0p && cp - C0p < C1) c = C0 + (cp - C0p);
                                const float v = (c >= 0 && n < Co) ? getw(n, c, tr * TPS + j) : 0.f;
                                dst[((size_t)(j * CS + cs) * 256 + tid) * 4 + nb] = v;
                            }
                }
            }
}

static const Param& P2(const cindm_unet2d* h, const std::string& k) { return h->params[h->index.at(k)]; }

// kind: CONV_3X3 / CONV_1X1_WIDE (every 1x1) / CONV_UP2 (3x3 over the x2 upsampled source) / CONV_UNSHUF (weight [Co][4C][1][1]) /
// CONV_STEM7; ws: weight standardisation (WeightStandardizedConv2d :116-124, folded here once: biased variance over
// (Ci, kh, kw), eps 1e-5); split: channels of the first of two concatenated sources.
// WeightStandardizedConv2d folded into the weights (biased variance, eps 1e-5): what the kernels multiply by.  With
// var << 1e-5 the result is (w - mean) / sqrt(1e-5), as small as the checkpoint's own weights: the range rule looks at it.
static std::vector<float> ws_folded2(const Param& w) {
    const int Co = (int)w.shape[0];
    std::vector<float> wv(w.host);
    const size_t per = w.numel / Co;
    for (int o = 0; o < Co; ++o) {
        float* p = wv.data() + (size_t)o * per;
        double m = 0; for (size_t i = 0; i < per; ++i) m += p[i];
        const float mean = (float)(m / per);
        double v = 0; for (size_t i = 0; i < per; ++i) { const double dd = (double)p[i] - mean; v += dd * dd; }
        const float var = (float)(v / per);
        const float rs = 1.0f / sqrtf(var + 1e-5f);
        for (size_t i = 0; i < per; ++i) p[i] = (p[i] - mean) * rs;
    }
    return wv;
}

static int pack_conv2d(cindm_unet2d* h, BlobBuilder& bb, const std::string& prefix, int kind, bool ws, int split) {
    const Param& w = P2(h, prefix + ".weight");
    const int Co = (int)w.shape[0], Ci = (int)w.shape[1], k = (int)w.shape[2];
    const std::vector<float> wv = ws ? ws_folded2(w) : w.host;
    Packed2 pk; pk.kind = kind;
    if (kind == CONV_1X1_WIDE) {
        // [n-tile of 64][q = k-step / 4][thread = wave*64 + lane][4 k-steps]: the A fragment of conv1x1_wide_kernel,
        // W[n = tile*64 + wave*16 + (lane & 15)][k = 4*(4q + j) + (lane >> 4)]
        REQUIRE(k == 1 && (Ci == 64 || Ci == 128 || Ci == 192), "1x1: 64, 128 or 192 input channels (concatenated sources in cat order)");
        pk.N = Co; pk.Npad = ceil_to(Co, T2N); pk.CinP = Ci;
        const int NQ = Ci / 16;
        pk.off = bb.alloc((size_t)(pk.Npad / T2N) * NQ * 256 * 4);
        float* base = bb.data.data() + pk.off;
        for (int it = 0; it < pk.Npad / T2N; ++it)
            for (int q = 0; q < NQ; ++q)
                for (int tid = 0; tid < 256; ++tid)
                    for (int j = 0; j < 4; ++j) {
                        const int wv_ = tid >> 6, lane = tid & 63;
                        const int n = it * T2N + wv_ * 16 + (lane & 15), kk2 = 4 * (4 * q + j) + (lane >> 4);
                        base[(((size_t)it * NQ + q) * 256 + tid) * 4 + j] = (n < Co) ? wv[(size_t)n * Ci + kk2] : 0.f;
                    }
        if (h->use_h3 && prefix == "final_conv" && Ci == 64 && Co <= 32) {
            // conv1x1_h3p_kernel<64, 2, false>: [k-step 2][plane][thread = ct * 64 + lane][8 halfs] = W[n = ct*16 + (lane & 15)][32 ks + 8 (lane >> 4) + e]
            Packed2 p3; p3.kind = CONV_1X1_WIDE; p3.h3 = true; p3.N = Co; p3.Npad = 32; p3.CinP = 64;
            p3.off = bb.alloc((size_t)2 * 2 * 128 * 8 / 2);
            uint16_t* b16 = reinterpret_cast<uint16_t*>(bb.data.data() + p3.off);
            auto bits = [](float v) { _Float16 hv = (_Float16)v; uint16_t u; std::memcpy(&u, &hv, 2); return u; };
            for (int ks = 0; ks < 2; ++ks)
                for (int tid = 0; tid < 128; ++tid)
                    for (int e = 0; e < 8; ++e) {
                        const int ct = tid >> 6, lane = tid & 63;
                        const int n = ct * 16 + (lane & 15), kk2 = 32 * ks + 8 * (lane >> 4) + e;
                        const float v = (n < Co) ? wv[(size_t)n * Ci + kk2] : 0.f;
                        const _Float16 hv = (_Float16)v;
                        const size_t o = (((size_t)ks * 2) * 128 + tid) * 8 + e;
                        b16[o] = bits(v);
                        b16[o + 128 * 8] = bits((v - (float)hv) * H3_SCALE);
                    }
            h->packed[prefix + "#p3"] = p3;
        }
        auto ends_with = [&](const char* s) { const size_t n = std::strlen(s); return prefix.size() >= n && prefix.compare(prefix.size() - n, n, s) == 0; };
        // the 1x1 GEMMs that were co-bound by the fp32 matrix pipe: ResnetBlock res_conv tails and the bottleneck attention's
        // projections.  (The qkv projection with LayerNorm-on-load INSIDE this kernel gave sporadically wrong pixels at 128
        // images -- whole rows, workgroups after the first residency wave only; unexplained -- so its LayerNorm is a
        // separate ln_apply_kernel pass and the projection a plain-source GEMM.)
        const bool tail = ends_with(".res_conv") || prefix == "mid_attn.fn.fn.to_out" || prefix == "mid_attn.fn.fn.to_qkv";
        if (tail && h->use_h3 && (Ci == 128 || Ci == 192) && Co % 4 == 0) {
            // conv1x1_tail_h3_kernel: [n-tile][k-step of 32][plane][thread][8 halfs] = W[n][32 ks + 8 (lane >> 4) + e], hi / scaled lo
            Packed2 p3; p3.kind = CONV_1X1_WIDE; p3.h3 = true; p3.N = Co; p3.Npad = pk.Npad; p3.CinP = Ci;
            const int KS = Ci / 32;
            const size_t halfs = (size_t)(pk.Npad / T2N) * KS * 2 * 256 * 8;
            p3.off = bb.alloc(halfs / 2);
            uint16_t* b16 = reinterpret_cast<uint16_t*>(bb.data.data() + p3.off);
            auto bits = [](float v) { _Float16 hv = (_Float16)v; uint16_t u; std::memcpy(&u, &hv, 2); return u; };
            for (int it = 0; it < pk.Npad / T2N; ++it)
                for (int ks = 0; ks < KS; ++ks)
                    for (int tid = 0; tid < 256; ++tid)
                        for (int e = 0; e < 8; ++e) {
                            const int wv_ = tid >> 6, lane = tid & 63;
                            const int n = it * T2N + wv_ * 16 + (lane & 15), kk2 = 32 * ks + 8 * (lane >> 4) + e;
                            const float v = (n < Co) ? wv[(size_t)n * Ci + kk2] : 0.f;
                            const _Float16 hv = (_Float16)v;
                            const size_t o = ((((size_t)it * KS + ks) * 2) * 256 + tid) * 8 + e;
                            b16[o] = bits(v);
                            b16[o + 256 * 8] = bits((v - (float)hv) * H3_SCALE);
                        }
            h->packed[prefix + "#t3"] = p3;
        }
    } else if (kind == CONV_STEM7) {
        REQUIRE(k == 7 && Ci <= 24, "stem: 7x7 convolution of at most 24 input channels expected");
        pk.N = Co; pk.Npad = ceil_to(Co, T2N); pk.CinP = 24;
        if (h->use_h3) {
            // split-fp16 stem: [n-tile][tap slot i < 25][q = nb*2 + plane][thread][8 halfs]; thread (kg = wave & 1,
            // nh = wave >> 1, lane) holds tap 2i + kg, channels (lane>>4)*8 + e, column nh*32 + nb*16 + (lane & 15)
            pk.h3 = true;
            const size_t halfs = (size_t)(pk.Npad / T2N) * STEM3_NI * 4 * 256 * 8;
            pk.off = bb.alloc(halfs / 2);
            uint16_t* base16 = reinterpret_cast<uint16_t*>(bb.data.data() + pk.off);
            auto bits = [](float v) { _Float16 hv = (_Float16)v; uint16_t u; std::memcpy(&u, &hv, 2); return u; };
            for (int nt = 0; nt < pk.Npad / T2N; ++nt)
                for (int i = 0; i < STEM3_NI; ++i)
                    for (int nb = 0; nb < 2; ++nb)
                        for (int tid = 0; tid < 256; ++tid) {
                            const int wv_ = tid >> 6, lane = tid & 63, kg = wv_ & 1, nh = wv_ >> 1;
                            const int tap = 2 * i + kg;
                            const int n = nt * T2N + nh * 32 + nb * 16 + (lane & 15);
                            for (int e = 0; e < 8; ++e) {
                                const int c = (lane >> 4) * 8 + e;
                                const float v = (tap < 49 && c < Ci && n < Co) ? wv[((size_t)n * Ci + c) * 49 + tap] : 0.f;
                                const _Float16 hv = (_Float16)v;
                                const float lo = (v - (float)hv) * 2048.0f;
                                const size_t q0 = ((((size_t)nt * STEM3_NI + i) * 4) + nb * 2) * 256;
                                base16[(q0 + tid) * 8 + e] = bits((float)hv);
                                base16[(q0 + 256 + tid) * 8 + e] = bits(lo);
                            }
                        }
            // conv2d_stem7_h3d_kernel's pack (dense reduction axis): [n-tile][slot i < 19][q = nb*2 + plane][thread][8 halfs]; thread
            // (kg, nh, lane) holds k-step ks = 2i + kg: ks < 35 -> kernel row ks / 5, k = 32 (ks % 5) + 8 (lane >> 4) + e = 24 dx + c;
            // ks = 35 + j -> kernel row (lane >> 4) + 4 j, dx = 6, c = 16 + e
            {
                Packed2 pd; pd.kind = CONV_STEM7; pd.h3 = true; pd.N = Co; pd.Npad = pk.Npad; pd.CinP = 24;
                pd.off = bb.alloc((size_t)(pk.Npad / T2N) * STEMD_NI * 4 * 256 * 8 / 2);
                uint16_t* d16 = reinterpret_cast<uint16_t*>(bb.data.data() + pd.off);
                for (int nt = 0; nt < pk.Npad / T2N; ++nt)
                    for (int i = 0; i < STEMD_NI; ++i)
                        for (int nb = 0; nb < 2; ++nb)
                            for (int tid = 0; tid < 256; ++tid) {
                                const int wv_ = tid >> 6, lane = tid & 63, kg = wv_ & 1, nh = wv_ >> 1, lg = lane >> 4;
                                const int ks = 2 * i + kg;
                                const int n = nt * T2N + nh * 32 + nb * 16 + (lane & 15);
                                for (int e = 0; e < 8; ++e) {
                                    int dy = -1, dx = 0, c = 0;
                                    if (ks < 35) { const int kidx = 32 * (ks % 5) + 8 * lg + e; dy = ks / 5; dx = kidx / 24; c = kidx % 24; }
                                    else if (ks < STEMD_KS) { dy = lg + 4 * (ks - 35); dx = 6; c = 16 + e; }
                                    const float v = (dy >= 0 && dy < 7 && c < Ci && n < Co) ? wv[((size_t)n * Ci + c) * 49 + dy * 7 + dx] : 0.f;
                                    const _Float16 hv = (_Float16)v;
                                    const float lo = (v - (float)hv) * 2048.0f;
                                    const size_t q0 = ((((size_t)nt * STEMD_NI + i) * 4) + nb * 2) * 256;
                                    d16[(q0 + tid) * 8 + e] = bits((float)hv);
                                    d16[(q0 + 256 + tid) * 8 + e] = bits(lo);
                                }
                            }
                h->packed[prefix + "#d7"] = pd;
            }
        } else {
        pk.off = bb.alloc((size_t)(pk.Npad / T2N) * STEM_NST * 256 * STEM_NBF * 4);
        float* base = bb.data.data() + pk.off;
        for (int nt = 0; nt < pk.Npad / T2N; ++nt)
            for (int st = 0; st < STEM_NST; ++st)
                for (int q = 0; q < STEM_NBF; ++q)
                    for (int tid = 0; tid < 256; ++tid) {
                        const int wv_ = tid >> 6, lane = tid & 63;
                        const int kidx = 4 * (st * STEM_NBF + q) + wv_;
                        const int tap = kidx / 6, cs = kidx % 6, c = cs * 4 + (lane >> 4);
                        for (int nb = 0; nb < 4; ++nb) {
                            const int n = nt * T2N + nb * 16 + (lane & 15);
                            const float v = (kidx < 294 && c < Ci && n < Co) ? wv[((size_t)n * Ci + c) * 49 + tap] : 0.f;
                            base[((((size_t)nt * STEM_NST + st) * STEM_NBF + q) * 256 + tid) * 4 + nb] = v;
                        }
                    }
        }
    } else {
        const int Cin_eff = (kind == CONV_UNSHUF) ? Ci / 4 : Ci;
        const int C0 = split ? split : Cin_eff, C1 = Cin_eff - C0;
        const int kk = k * k;
        auto getw = [&](int n, int c, int tt) -> float {
            if (kind == CONV_UNSHUF) return wv[(size_t)n * Ci + c * 4 + tt];
            return wv[((size_t)n * Ci + c) * kk + tt];
        };
        if ((kind == CONV_3X3 || kind == CONV_UP2) && h->use_h3) {
            // split-fp16 packing for conv2d_h3_kernel: [n-tile of 64][chunk of 64 channels][tap][q = nb*2 + plane][thread]
            // [8 halfs] = B[k = (lane>>4)*8 + e][n = (lane & 15)] of v_mfma_f32_16x16x32_f16 for the wave's k-group
            // (wave & 1) and column half (wave >> 1)
            REQUIRE(k == 3, "3x3 expected");
            const int KC = 64;
            const int C0p = ceil_to(C0, KC), C1p = C1 ? ceil_to(C1, KC) : 0;
            pk.CinP = C0p + C1p; pk.N = Co; pk.Npad = ceil_to(Co, T2N); pk.h3 = true;
            const int nch = pk.CinP / KC;
            const size_t halfs = (size_t)(pk.Npad / T2N) * nch * 9 * 4 * 256 * 8;
            pk.off = bb.alloc(halfs / 2);
            uint16_t* base = reinterpret_cast<uint16_t*>(bb.data.data() + pk.off);
            auto bits = [](float v) { _Float16 hv = (_Float16)v; uint16_t u; std::memcpy(&u, &hv, 2); return u; };
            for (int nt = 0; nt < pk.Npad / T2N; ++nt)
                for (int ch = 0; ch < nch; ++ch)
                    for (int tap = 0; tap < 9; ++tap)
                        for (int nb = 0; nb < 2; ++nb)
                            for (int tid = 0; tid < 256; ++tid) {
                                const int wv_ = tid >> 6, lane = tid & 63, kg = wv_ & 1, nh = wv_ >> 1;
                                const int n = nt * T2N + nh * 32 + nb * 16 + (lane & 15);
                                for (int e = 0; e < 8; ++e) {
                                    const int cp = ch * KC + kg * 32 + (lane >> 4) * 8 + e;
                                    int c = -1;
                                    if (cp < C0) c = cp;
                                    else if (cp >= C0p && cp - C0p < C1) c = C0 + (cp - C0p);
                                    const float v = (c >= 0 && n < Co) ? getw(n, c, tap) : 0.f;
                                    const _Float16 hv = (_Float16)v;
                                    const float lo = (v - (float)hv) * 2048.0f;
                                    const size_t q0 = ((((size_t)nt * nch + ch) * 9 + tap) * 4 + nb * 2) * 256;
                                    base[(q0 + tid) * 8 + e] = bits((float)hv);
                                    base[(q0 + 256 + tid) * 8 + e] = bits(lo);
                                }
                            }
        }
        else if (kind == CONV_UNSHUF) {
            REQUIRE(k == 1, "unshuffle 1x1 expected");
            pack_tile_f32(bb, pk, 32, 4, 1, C0, C1, Co, getw);
            if (h->use_h3 && Ci == 256 && Co == 64) {
                // conv_unshuf_h3p_kernel: [k-step 8][plane][thread = ct * 64 + lane][8 halfs] = W[n = ct*16 + (lane & 15)][tap*64 + c], k = 32 ks + 8 (lane >> 4) + e
                Packed2 p3; p3.kind = CONV_UNSHUF; p3.h3 = true; p3.N = Co; p3.Npad = 64; p3.CinP = 256;
                p3.off = bb.alloc((size_t)8 * 2 * 256 * 8 / 2);
                uint16_t* b16 = reinterpret_cast<uint16_t*>(bb.data.data() + p3.off);
                auto bits = [](float v) { _Float16 hv = (_Float16)v; uint16_t u; std::memcpy(&u, &hv, 2); return u; };
                for (int ks = 0; ks < 8; ++ks)
                    for (int tid = 0; tid < 256; ++tid)
                        for (int e = 0; e < 8; ++e) {
                            const int ct = tid >> 6, lane = tid & 63;
                            const int n = ct * 16 + (lane & 15), kk2 = 32 * ks + 8 * (lane >> 4) + e;
                            const float v = getw(n, kk2 & 63, kk2 >> 6);
                            const _Float16 hv = (_Float16)v;
                            const size_t o = (((size_t)ks * 2) * 256 + tid) * 8 + e;
                            b16[o] = bits(v);
                            b16[o + 256 * 8] = bits((v - (float)hv) * H3_SCALE);
                        }
                h->packed[prefix + "#u3"] = p3;
            }
        }
        else { REQUIRE(k == 3, "3x3 expected"); pack_tile_f32(bb, pk, 32, 3, 3, C0, C1, Co, getw); }
    }
    auto bi = h->index.find(prefix + ".bias");
    if (bi != h->index.end()) {
        pk.has_bias = true; pk.bias_off = bb.alloc(pk.Npad);
        const Param& b = h->params[bi->second];
        for (int n = 0; n < Co; ++n) bb.data[pk.bias_off + n] = b.host[n];
    }
    h->packed[prefix] = pk;
    return 0;
}

// LinearAttention projections as split-fp16 fragments for la2d_context_kernel / la2d_apply_out_kernel:
// [tile of 16 output channels][k32][plane hi / scaled lo][lane][e] = W[tile*16 + lane%16][k32*32 + (lane/16)*8 + e]
static void pack_la_site2(cindm_unet2d* h, BlobBuilder& bb, const std::string& attn_prefix) {
    const Param& wq = P2(h, attn_prefix + ".to_qkv.weight");
    const Param& wo = P2(h, attn_prefix + ".to_out.0.weight");
    const int C = (int)wq.shape[1];
    if ((int)wq.shape[0] != 384 || (int)wo.shape[1] != 128 || (int)wo.shape[0] != C || (C != 64 && C != 128)) return;
    auto frag_h3 = [&](const Param& w, int Co, int Ci, const std::string& name) {
        Packed2 pk; pk.kind = CONV_1X1_WIDE; pk.CinP = Ci; pk.Npad = Co; pk.N = Co; pk.h3 = true;
        const int K32 = Ci / 32;
        pk.off = bb.alloc((size_t)(Co / 16) * K32 * 2 * 64 * 4);
        uint16_t* base = reinterpret_cast<uint16_t*>(bb.data.data() + pk.off);
        auto bits = [](float v) { _Float16 hv = (_Float16)v; uint16_t u; std::memcpy(&u, &hv, 2); return u; };
        for (int t = 0; t < Co / 16; ++t)
            for (int k = 0; k < K32; ++k)
                for (int lane = 0; lane < 64; ++lane)
                    for (int e = 0; e < 8; ++e) {
                        const float v = w.host[(size_t)(t * 16 + (lane & 15)) * Ci + k * 32 + (lane >> 4) * 8 + e];
                        const _Float16 hv = (_Float16)v;
                        const float lo = (v - (float)hv) * 2048.0f;
                        const size_t q0 = ((size_t)t * K32 + k) * 2;
                        base[((q0 + 0) * 64 + lane) * 8 + e] = bits((float)hv);
                        base[((q0 + 1) * 64 + lane) * 8 + e] = bits(lo);
                    }
        h->packed[name] = pk;
    };
    frag_h3(wq, 384, C, attn_prefix + ".to_qkv#la");
    frag_h3(wo, C, 128, attn_prefix + ".to_out.0#la");
}

static void pack_linear2(cindm_unet2d* h, BlobBuilder& bb, const std::string& prefix) {
    const Param& w = P2(h, prefix + ".weight");
    const int Co = (int)w.shape[0], Ci = (int)w.shape[1];
    Packed pk; pk.T = 1; pk.KC = (Ci % 128 == 0) ? 128 : 64; pk.N = Co; pk.Npad = ceil_to(Co, TN);
    auto getw = [&](int n, int c) -> float { return w.host[(size_t)n * Ci + c]; };
    pack_frag_f32(bb, pk.off, pk.CinP, pk.KC, Ci, Co, getw);
    pk.has_bias = true; pk.bias_off = bb.alloc(pk.Npad);
    const Param& b = P2(h, prefix + ".bias");
    for (int n = 0; n < Co; ++n) bb.data[pk.bias_off + n] = b.host[n];
    h->lin[prefix] = pk;
}

static void pack_vec2(cindm_unet2d* h, BlobBuilder& bb, const std::string& key) {
    const Param& v = P2(h, key);
    size_t o = bb.alloc(v.numel);
    std::memcpy(bb.data.data() + o, v.host.data(), v.numel * sizeof(float));
    h->vec_off[key] = o;
}

// ---- emission --------------------------------------------------------------------------------------------
struct Ten2 { float* p = nullptr; int H = 0, W = 0, C = 0, ld = 0; };

struct Emitter2 {
    cindm_unet2d* h;
    hipStream_t stream;
    bool dry;
    char* ws; size_t ws_off = 0;
    int64_t NI;
    const int* t_ptr; int t_imm;
    int launches = 0;
    hipError_t err = hipSuccess;
    // instrumented mode (cindm_unet2d_profile): every launch bracketed by HIP events on the launch stream.
    // kinds: 0 conv3x3 (incl. upsampled), 1 conv1x1 / unshuffle, 2 stem 7x7, 3 qkv 1x1 (wide), 4 linear attention,
    // 5 full attention, 6 statistics merge / LayerNorm-residual
    struct ProfRec { int kind; hipEvent_t e0, e1; double flops; };
    std::vector<ProfRec>* prof = nullptr;
    void pbegin(int kind, double flops) {
        if (!prof || dry) return;
        ProfRec r; r.kind = kind; r.flops = flops;
        (void)hipEventCreate(&r.e0); (void)hipEventCreate(&r.e1);
        (void)hipEventRecord(r.e0, stream);
        prof->push_back(r);
    }
    void pend() { if (prof && !dry) (void)hipEventRecord(prof->back().e1, stream); }

    // Block-internal temporaries (the two Block.proj outputs, statistics partials, q|k|v, partial contexts) are released
    // when their block has been emitted and the next block's temporaries take their place: launches execute in stream
    // order, so a later launch can only overwrite what every earlier launch has finished with.  Block OUTPUTS (skips,
    // taps) keep their own slices.  ws_alias = 0 gives every intermediate its own slice again.
    size_t ws_peak = 0;
    size_t mark() const { return ws_off; }
    void release(size_t m) { ws_peak = std::max(ws_peak, ws_off); if (h->O("ws_alias")) ws_off = m; }
    size_t peak() const { return std::max(ws_peak, ws_off); }
    float* alloc(size_t nfloats) {
        size_t o = ws_off;
        ws_off += ((nfloats * sizeof(float) + 255) / 256) * 256;
        return dry ? nullptr : reinterpret_cast<float*>(ws + o);
    }
    Ten2 ten(int H, int W, int C) { Ten2 t; t.H = H; t.W = W; t.C = C; t.ld = C; t.p = alloc((size_t)NI * H * W * C); return t; }
    const float* V(const std::string& k) const { return h->blob + h->vec_off.at(k); }
    void tap(const std::string& name, const Ten2& t) {
        if (dry) return;
        h->taps[name] = {(size_t)(reinterpret_cast<char*>(t.p) - ws), t.H * t.W, t.C};
    }
    static void plain(Src& s, const Ten2& t) { s.p = t.p; s.ld = t.ld; s.C = t.C; s.mode = SRC2_PLAIN; s.P = 1; s.gw = 1; s.cnt = 1.f; }

    // 3x3 convolutions on the split-fp16 path use conv2d_ws_kernel's 8 x 16 pixel tiles where they divide the image
    // conv_ws: 1 = all of them, 2 = only the plain-source ones, 3 = only the GroupNorm-on-load ones (debugging splits)
    bool use_ws(const Packed2& pk, int Hout, int Wout, int mode = SRC2_PLAIN) const {
        const int v = h->O("conv_ws");
        const bool sel = v == 1 || (v == 2 && mode == SRC2_PLAIN) || (v == 3 && mode == SRC2_GN_SS_SILU);
        // 32-bit element offsets inside the kernel: images * pixels * widest row < 2^31
        const bool small = (double)NI * Hout * Wout * 4.0 * std::max(pk.CinP, pk.Npad) < 2147483648.0;
        const bool geo = pk.h3 && (pk.kind == CONV_3X3 || pk.kind == CONV_UP2) && Hout % V2Y == 0 && Wout % V2X == 0 && pk.N % 4 == 0 && small;
        if (geo && sel && mode == SRC2_GN_SS_SILU) {
            // the kernel holds at most WS_MAXP statistics partials per (image, group); they come from the block's first
            // convolution (same geometry, plain source)
            const bool prod_ws = v == 1 || v == 2;
            const int pin = prod_ws ? (Hout / V2Y) * (Wout / V2X) * WS_SPT : (Hout / T2Y) * (Wout / T2X);
            if (pin > WS_MAXP) return false;
        }
        return geo && sel;
    }
    int tile_rows(const Packed2& pk, int Hout, int Wout, int mode = SRC2_PLAIN) const { return use_ws(pk, Hout, Wout, mode) ? V2Y : T2Y; }
    void base(Conv2dArgs& a, const Packed2& pk, int Hin, int Win, int Hout, int Wout, int mode = SRC2_PLAIN) {
        std::memset(&a, 0, sizeof(a));
        a.W = pk.identity ? nullptr : h->blob + pk.off; a.bias = pk.has_bias ? h->blob + pk.bias_off : nullptr;
        a.CinP = pk.CinP; a.Npad = pk.Npad; a.N = pk.N;
        a.NI = (int)NI; a.Hin = Hin; a.Win = Win; a.Hout = Hout; a.Wout = Wout;
        a.tiles_x = Wout / T2X;
        a.tpi = (Hout / tile_rows(pk, Hout, Wout, mode)) * (Wout / T2X);
        a.rows_total = (int64_t)NI * Hout * Wout; a.tiles_per_group = 0;
        a.t_ptr = t_ptr; a.t_imm = t_imm; a.nsrc = 1;
        a.dbg = h->O("dbg2");
        a.stress = h->O("stress");
    }
    void launch(const Packed2& pk, const Conv2dArgs& a) {
        ++launches;
        if (dry) return;
        dim3 grid(a.Npad / T2N, (unsigned)(a.NI * a.tpi));
        const int mode = a.src[0].mode;
        bool ok = true;
        auto alt_pack = [&](const char* suffix) -> const Packed2* {     // a second pack of the same layer (key = its name + suffix)
            for (const auto& kv : h->packed)
                if (&kv.second == &pk) {
                    auto it = h->packed.find(kv.first + suffix);
                    return it != h->packed.end() ? &it->second : nullptr;
                }
            return nullptr;
        };
        // final_conv (64 -> channels) on the pipelined split-fp16 1x1 kernel (option final_h3): bias only, plain source
        const Packed2* final3 = nullptr;
        if (pk.kind == CONV_1X1_WIDE && !pk.h3 && !pk.identity && mode == SRC2_PLAIN && a.nsrc == 1 && a.src[0].C == 64 &&
            a.N <= 32 && a.ldo >= ((a.N + 3) & ~3) && a.ldo % 4 == 0 && !(a.rows_total & 63) && !a.stats_out && !a.e_y && !a.res && !a.ln_out && !a.lnr_g)
            final3 = alt_pack("#p3");
        // the pixel-unshuffle 1x1 on the same kernel (option unshuf_h3): 64 -> 64 channels, whole 64-pixel output tiles
        const Packed2* unshuf3 = nullptr;
        if (pk.kind == CONV_UNSHUF && a.nsrc == 1 && a.src[0].C == 64 && a.N == 64 && !(a.rows_total & 63) &&
            !a.stats_out && !a.e_y && !a.res && !a.ln_out) {
            unshuf3 = alt_pack("#u3");
        }
        const Packed2* stem_d = nullptr;
        if (pk.kind == CONV_STEM7 && pk.h3 && !a.stats_out && a.Hout % STEMD_TY == 0) {
            stem_d = alt_pack("#d7");
        }
        {
            const double cin = (double)a.src[0].C + (a.nsrc > 1 ? (double)a.src[1].C : 0.0);
            const double taps = (pk.kind == CONV_3X3 || pk.kind == CONV_UP2) ? 9.0 : (pk.kind == CONV_STEM7) ? 49.0 : 1.0;
            const double cin_eff = (pk.kind == CONV_STEM7) ? (double)h->d.channels : (pk.kind == CONV_UNSHUF) ? 4.0 * cin : cin;
            const int kind = (pk.kind == CONV_3X3 || pk.kind == CONV_UP2) ? 0 : (pk.kind == CONV_STEM7) ? 2 : (pk.kind == CONV_1X1_WIDE && mode == SRC2_LN) ? 3 : 1;
            pbegin(kind, 2.0 * a.NI * a.Hout * a.Wout * a.N * cin_eff * taps);
        }
#define C2_LAUNCH(K_, M_) hipLaunchKernelGGL((conv2d_tile_kernel<K_, M_>), grid, dim3(256), 0, stream, a)
        if (pk.h3 && pk.kind != CONV_1X1_WIDE && (a.e_y || a.res || a.ln_out)) ok = false;   // the 3x3 epilogues carry bias + GroupNorm partials only
        else if (use_ws(pk, a.Hout, a.Wout, mode)) {
            const dim3 g2(WS_GRID);
            // ws_nosplit: 1 = never split K over the matrix waves; 2 (default) = split it only where it still pays -- plain-source layers of
            // more than one 64-channel chunk, whose reduction is amortised over the chunks (in-kernel clocks, profiles/r05_ws_phase_clocks.txt:
            // 5.50 us per item with the k-groups, 5.60 without; every other kind is faster without: 6.60 -> 6.42, 8.72 -> 7.40, 6.28 -> 5.88)
            const int nsv = h->O("ws_nosplit");
            const bool ksplit = nsv == 0 || (nsv == 2 && mode == SRC2_PLAIN && pk.CinP > 64);
#define WS_LAUNCH(K_, M_) do { if (ksplit) hipLaunchKernelGGL((conv2d_ws_kernel<K_, M_, 0>), g2, dim3(512), 0, stream, a); \
                               else hipLaunchKernelGGL((conv2d_ws_kernel<K_, M_, 1>), g2, dim3(512), 0, stream, a); } while (0)
            if (pk.kind == CONV_3X3 && mode == SRC2_PLAIN) WS_LAUNCH(CONV_3X3, SRC2_PLAIN);
            else if (pk.kind == CONV_3X3 && mode == SRC2_GN_SS_SILU) WS_LAUNCH(CONV_3X3, SRC2_GN_SS_SILU);
            else if (pk.kind == CONV_UP2 && mode == SRC2_PLAIN) WS_LAUNCH(CONV_UP2, SRC2_PLAIN);
            else ok = false;
#undef WS_LAUNCH
        }
        else if (pk.h3 && pk.kind == CONV_STEM7 && mode == SRC2_PLAIN && stem_d) {
            Conv2dArgs b = a;
            b.W = h->blob + stem_d->off;
            hipLaunchKernelGGL(conv2d_stem7_h3d_kernel, dim3(grid.x, (unsigned)(a.NI * (a.Hout / STEMD_TY) * a.tiles_x)), dim3(256), 0, stream, b);
        }
        else if (pk.h3 && pk.kind == CONV_STEM7 && mode == SRC2_PLAIN) hipLaunchKernelGGL(conv2d_stem7_h3_kernel, grid, dim3(256), 0, stream, a);
        else if (pk.h3 && pk.kind == CONV_3X3 && mode == SRC2_PLAIN) hipLaunchKernelGGL((conv2d_h3_kernel<CONV_3X3, SRC2_PLAIN>), grid, dim3(256), 0, stream, a);
        else if (pk.h3 && pk.kind == CONV_3X3 && mode == SRC2_GN_SS_SILU) hipLaunchKernelGGL((conv2d_h3_kernel<CONV_3X3, SRC2_GN_SS_SILU>), grid, dim3(256), 0, stream, a);
        else if (pk.h3 && pk.kind == CONV_UP2 && mode == SRC2_PLAIN) hipLaunchKernelGGL((conv2d_h3_kernel<CONV_UP2, SRC2_PLAIN>), grid, dim3(256), 0, stream, a);
        else if (pk.h3 && pk.kind != CONV_1X1_WIDE) ok = false;
        else if (pk.kind == CONV_3X3 && mode == SRC2_PLAIN) C2_LAUNCH(CONV_3X3, SRC2_PLAIN);
        else if (pk.kind == CONV_3X3 && mode == SRC2_GN_SS_SILU) C2_LAUNCH(CONV_3X3, SRC2_GN_SS_SILU);
        else if (pk.kind == CONV_UP2 && mode == SRC2_PLAIN) C2_LAUNCH(CONV_UP2, SRC2_PLAIN);
        else if (pk.kind == CONV_UNSHUF && mode == SRC2_PLAIN && unshuf3) {
            Conv2dArgs b = a;
            b.W = h->blob + unshuf3->off;
            hipLaunchKernelGGL((conv1x1_h3p_kernel<256, 4, true>), dim3((unsigned)std::min<int64_t>(a.rows_total >> 6, 256)), dim3(512), 0, stream, b);
        }
        else if (pk.kind == CONV_UNSHUF && mode == SRC2_PLAIN) C2_LAUNCH(CONV_UNSHUF, SRC2_PLAIN);
        else if (pk.kind == CONV_STEM7 && mode == SRC2_PLAIN) hipLaunchKernelGGL(conv2d_stem7_kernel, grid, dim3(256), 0, stream, a);
        else if (final3) {
            Conv2dArgs b = a;
            b.W = h->blob + final3->off;
            hipLaunchKernelGGL((conv1x1_h3p_kernel<64, 2, false>), dim3((unsigned)std::min<int64_t>(a.rows_total >> 6, 1024)), dim3(256), 0, stream, b);
        }
        else if (pk.kind == CONV_1X1_WIDE && pk.h3) {          // ResnetBlock tail with a GEMM on the split-fp16 products
            const dim3 g1((unsigned)((size_t)a.NI * a.Hout * a.Wout / 64));
            // the ResnetBlock tails proper (64 output channels, SiLU(GN(y1)) operand, nothing else): the pipelined loop over tiles
            const bool pipe = a.e_y && !a.res && !a.ln_out && !a.lnr_g && (a.Npad == T2N || a.Npad == 2 * T2N) && a.N == a.Npad &&
                              a.src[0].C % 4 == 0 && (a.nsrc == 1 || a.src[1].C % 4 == 0) &&
                              a.src[0].C + (a.nsrc > 1 ? a.src[1].C : 0) == pk.CinP;
            const dim3 gp((unsigned)std::min<int64_t>(a.rows_total >> 6, a.Npad == T2N ? 512 : 256));
            if (mode != SRC2_PLAIN || a.lnr_g || (a.rows_total & 63)) ok = false;
            else if (pipe && pk.CinP == 128 && a.Npad == T2N) hipLaunchKernelGGL((conv1x1_tail_h3p_kernel<128, 4>), gp, dim3(256), 0, stream, a);
            else if (pipe && pk.CinP == 192 && a.Npad == 2 * T2N) hipLaunchKernelGGL((conv1x1_tail_h3p_kernel<192, 8>), gp, dim3(512), 0, stream, a);
            else if (pk.CinP == 128) hipLaunchKernelGGL((conv1x1_tail_h3_kernel<128>), g1, dim3(256), 0, stream, a);
            else if (pk.CinP == 192) hipLaunchKernelGGL((conv1x1_tail_h3_kernel<192>), g1, dim3(256), 0, stream, a);
            else ok = false;
        }
        else if (pk.kind == CONV_1X1_WIDE) {
            const dim3 g1((unsigned)((size_t)a.NI * a.Hout * a.Wout / 64));
#define W_LAUNCH(KT_, M_, R_, E_) hipLaunchKernelGGL((conv1x1_wide_kernel<KT_, M_, R_, E_>), g1, dim3(256), 0, stream, a)
            const bool epi = a.bias || a.e_y || a.res || a.ln_out || pk.identity || (a.N & 63);
            // the identity tail out = x + SiLU(GN(y1)) as an element-wise pass (option "tail_ew", default on)
            const bool ew = pk.identity && mode == SRC2_PLAIN && a.e_y && !a.bias && !a.res && !a.lnr_g &&
                            a.nsrc == 1 && a.src[0].C == pk.CinP && a.N == pk.CinP && !(a.rows_total & 63) && (pk.CinP == 64 || pk.CinP == 128);
            if (ew) {
                if (pk.CinP == 64) hipLaunchKernelGGL(tail_identity_kernel<64>, g1, dim3(256), 0, stream, a);
                else hipLaunchKernelGGL(tail_identity_kernel<128>, g1, dim3(256), 0, stream, a);
            } else
            if (pk.CinP == 64 && mode == SRC2_LN && !epi) W_LAUNCH(64, SRC2_LN, true, false);
            else if (pk.CinP == 128 && mode == SRC2_LN && !epi) W_LAUNCH(128, SRC2_LN, true, false);
            else if (pk.CinP == 64 && mode == SRC2_PLAIN) W_LAUNCH(64, SRC2_PLAIN, false, true);
            else if (pk.CinP == 128 && mode == SRC2_PLAIN && a.lnr_g)
                hipLaunchKernelGGL((conv1x1_wide_kernel<128, SRC2_PLAIN, false, true, true>), g1, dim3(256), 0, stream, a);
            else if (pk.CinP == 128 && mode == SRC2_PLAIN) W_LAUNCH(128, SRC2_PLAIN, false, true);
            else if (pk.CinP == 192 && mode == SRC2_PLAIN) W_LAUNCH(192, SRC2_PLAIN, false, true);
            else ok = false;
#undef W_LAUNCH
        }
        else ok = false;
#undef C2_LAUNCH
        pend();
        if (!ok) err = hipErrorInvalidValue;
        hipError_t e = hipGetLastError();
        if (e != hipSuccess && err == hipSuccess) err = e;
    }
};

// ResnetBlock (:200-224): A: y0 = WSconv3x3(x) (+GN partials) ; merge ; B: y1 = WSconv3x3(SiLU(GN(y0)*(scale+1)+shift)) ;
// merge ; C: out = SiLU(GN(y1)) + (res_conv(x) | x)  (+ LayerNorm row partials when an attention follows)
static Ten2 emit_rb2(Emitter2& E, const std::string& p, const Ten2& x0, const Ten2* x1, int cout, bool want_ln, float** ln_out) {
    cindm_unet2d* h = E.h;
    const int H = x0.H, W = x0.W, HW = H * W, gw = cout / 8;
    const Packed2& w0 = h->packed.at(p + ".block1.proj");
    const Packed2& w1 = h->packed.at(p + ".block2.proj");
    Ten2 out = E.ten(H, W, cout);
    float* lnbuf = want_ln ? E.alloc((size_t)E.NI * HW * (cout / 16) * 2) : nullptr;     // read by the attention that follows
    if (want_ln) *ln_out = lnbuf;
    const size_t scope = E.mark();
    Ten2 y0 = E.ten(H, W, cout), y1 = E.ten(H, W, cout);
    // GroupNorm statistics travel as per-tile (mean, M2) partials [image][8][tpi][2]; the consumers merge them
    const bool ws0 = E.use_ws(w0, H, W, SRC2_PLAIN);
    const int tpi0 = (H / (ws0 ? V2Y : T2Y)) * (W / T2X) * (ws0 ? WS_SPT : 1);
    const bool ws1 = E.use_ws(w1, H, W, SRC2_GN_SS_SILU);
    const int tpi1 = (H / (ws1 ? V2Y : T2Y)) * (W / T2X) * (ws1 ? WS_SPT : 1);
    const float pcnt0 = ws0 ? (float)(V2M / WS_SPT * gw) : (float)(T2Y * T2X * gw), pcnt1 = ws1 ? (float)(V2M / WS_SPT * gw) : (float)(T2Y * T2X * gw);
    float* pt0 = E.alloc((size_t)E.NI * 8 * tpi0 * 2);
    float* pt1 = E.alloc((size_t)E.NI * 8 * tpi1 * 2);
    Conv2dArgs a;
    E.base(a, w0, H, W, H, W);
    Emitter2::plain(a.src[0], x0);
    if (x1) { Emitter2::plain(a.src[1], *x1); a.nsrc = 2; }
    a.out = y0.p; a.ldo = y0.ld; a.stats_out = pt0; a.so_gw = gw;
    E.launch(w0, a);
    E.base(a, w1, H, W, H, W, SRC2_GN_SS_SILU);
    Src& s = a.src[0];
    s.p = y0.p; s.ld = y0.ld; s.C = cout; s.mode = SRC2_GN_SS_SILU; s.stats = pt0; s.P = tpi0; s.gw = gw; s.cnt = pcnt0;
    s.gamma = E.V(p + ".block1.norm.weight"); s.beta = E.V(p + ".block1.norm.bias");
    s.tb = h->ttable + h->tt_off.at(p); s.tb_ld = h->tt_ld;
    a.out = y1.p; a.ldo = y1.ld; a.stats_out = pt1; a.so_gw = gw;
    E.launch(w1, a);
    auto rc = h->packed.find(p + ".res_conv");
    if (rc != h->packed.end()) {
        auto rc3 = h->packed.find(p + ".res_conv#t3");
        const bool t3 = rc3 != h->packed.end() && h->O("tail_h3") && ((E.NI * (int64_t)HW) & 63) == 0;
        const Packed2& rpk = t3 ? rc3->second : rc->second;
        E.base(a, rpk, H, W, H, W);
        if (t3) a.bias = rc->second.has_bias ? h->blob + rc->second.bias_off : nullptr;
        Emitter2::plain(a.src[0], x0);
        if (x1) { Emitter2::plain(a.src[1], *x1); a.nsrc = 2; }
        a.e_y = y1.p; a.e_ld = y1.ld; a.e_stats = pt1; a.e_P = tpi1; a.e_gw = gw; a.e_cnt = pcnt1;
        a.e_gamma = E.V(p + ".block2.norm.weight"); a.e_beta = E.V(p + ".block2.norm.bias");
        a.out = out.p; a.ldo = out.ld;
        if (want_ln) a.ln_out = lnbuf;
        E.launch(rpk, a);
    } else {
        // identity residual: a 1x1 "convolution" with an identity weight matrix keeps one code path (the epilogue adds
        // SiLU(GN(y1))); its cost is one K = C GEMM of the smallest kind
        const Packed2& id = h->packed.at("__identity" + std::to_string(cout));
        E.base(a, id, H, W, H, W);
        Emitter2::plain(a.src[0], x0);
        a.e_y = y1.p; a.e_ld = y1.ld; a.e_stats = pt1; a.e_P = tpi1; a.e_gw = gw; a.e_cnt = pcnt1;
        a.e_gamma = E.V(p + ".block2.norm.weight"); a.e_beta = E.V(p + ".block2.norm.bias");
        a.out = out.p; a.ldo = out.ld;
        if (want_ln) a.ln_out = lnbuf;
        E.launch(id, a);
    }
    E.tap(p, out);
    E.release(scope);
    return out;
}

static bool la_site_ok(const cindm_unet2d* h, const std::string& p, int HW) {
    return h->packed.count(p + ".fn.fn.to_qkv#la") && HW % 512 == 0;      // four workgroups per image, whole slices each
}

// Residual(PreNorm(LinearAttention)) (:226-254): qkv = Wqkv LN(x)g ; k column statistics ; partial contexts ; apply ;
// z = Wo att + bo ; out = LN(z) g2 + x
static Ten2 emit_lattn2(Emitter2& E, const std::string& p, const Ten2& x, const float* lnp) {
    cindm_unet2d* h = E.h;
    const int H = x.H, W = x.W, HW = H * W, C = x.C;
    const Packed2& wq = h->packed.at(p + ".fn.fn.to_qkv");
    const Packed2& wo = h->packed.at(p + ".fn.fn.to_out.0");
    if (la_site_ok(h, p, HW)) {
        // three launches, no q|k|v tensor: slice contexts, merge, apply + out projection + LayerNorm + residual
        Ten2 out = E.ten(H, W, C);
        const size_t scope = E.mark();
        // four workgroups per image (two per CU at 128 images): each loops over its share of slices / tiles
        const int nsl = HW / la2_px(C);
        int nsplit = nsl < 4 ? nsl : 4;
        if (C == 64 && h->O("la_nsplit") > 0) { nsplit = h->O("la_nsplit"); while (nsplit > 1 && (nsplit > nsl || nsl % nsplit || nsplit > 64)) nsplit >>= 1; }
        const int spw = nsl / nsplit;
        // (apply kernel, C = 64: three workgroups fit a CU -- option la_wpi = workgroups per image)
        const int ntl = HW / 64;
        int wpi = ntl < 4 ? ntl : 4;
        if (C == 64 && h->O("la_wpi") > 0) { wpi = h->O("la_wpi"); while (wpi > 1 && (wpi > ntl || ntl % wpi)) wpi >>= 1; }
        const int tpw = ntl / wpi;
        float* part = E.alloc((size_t)E.NI * 4 * nsplit * LA2_REC);
        float* ctx = E.alloc((size_t)E.NI * 4 * 1024);
        E.launches += 3;
        if (!E.dry) {
            La2dArgs l;
            l.x = x.p; l.ldx = x.ld; l.out = out.p; l.ldo = out.ld;
            l.g = E.V(p + ".fn.norm.g"); l.g2 = E.V(p + ".fn.fn.to_out.1.g");
            l.Wqkv = h->blob + h->packed.at(p + ".fn.fn.to_qkv#la").off; l.Wo = h->blob + h->packed.at(p + ".fn.fn.to_out.0#la").off;
            l.bo = h->blob + wo.bias_off; l.part = part; l.ctx = ctx; l.HW = HW; l.nsplit = nsplit; l.spw = spw; l.tpw = tpw;
            l.dbg = 0;
            E.pbegin(4, 2.0 * E.NI * HW * (C * 384.0 + 2.0 * 4 * 32 * 32 + 128.0 * C));
            // (the per-head products run on the split-fp16 MFMA -- template argument H16 = true; round 5's A/B against the exact fp32 form:
            // same-box 5.37 - 5.48 -> 5.31 ms per step, DESIGN 4.5e)
            if (C == 64) hipLaunchKernelGGL((la2d_context_kernel<64>), dim3((unsigned)E.NI * nsplit), dim3(256), 0, E.stream, l);
            else hipLaunchKernelGGL((la2d_context_kernel<128>), dim3((unsigned)E.NI * nsplit), dim3(256), 0, E.stream, l);
            hipLaunchKernelGGL(la2d_merge_kernel, dim3((unsigned)E.NI * 4), dim3(256), 0, E.stream, part, ctx, nsplit, HW);
            if (C == 64) hipLaunchKernelGGL((la2d_apply_out_kernel<64>), dim3((unsigned)E.NI * wpi), dim3(256), 0, E.stream, l);
            else hipLaunchKernelGGL((la2d_apply_out_kernel<128>), dim3((unsigned)E.NI * wpi), dim3(256), 0, E.stream, l);
            E.pend();
            hipError_t e = hipGetLastError();
            if (e != hipSuccess && E.err == hipSuccess) E.err = e;
        }
        E.tap(p, out);
        E.release(scope);
        return out;
    }
    Ten2 out = E.ten(H, W, C);
    const size_t scope = E.mark();
    Ten2 qkv = E.ten(H, W, 384), att = E.ten(H, W, 128);
    float* kst = E.alloc((size_t)E.NI * 4 * LA_SPLIT * 32 * 2);
    float* ctxp = E.alloc((size_t)E.NI * 4 * LA_SPLIT * 1024);
    Conv2dArgs a;
    E.base(a, wq, H, W, H, W);
    Src& s = a.src[0];
    s.p = x.p; s.ld = x.ld; s.C = C; s.mode = SRC2_LN; s.stats = lnp; s.P = C / 16; s.cnt = 16.f; s.gw = 1;
    s.gamma = E.V(p + ".fn.norm.g");
    a.out = qkv.p; a.ldo = 384;
    E.launch(wq, a);
    E.launches += 2;
    if (!E.dry) {
        E.pbegin(4, 2.0 * 2.0 * E.NI * 4.0 * HW * 32.0 * 32.0);
        hipLaunchKernelGGL(la_context_kernel, dim3((unsigned)E.NI * 4 * LA_SPLIT), dim3(256), 0, E.stream, qkv.p, kst, ctxp, HW);
        hipLaunchKernelGGL(la_apply_kernel, dim3((HW + 255) / 256, (unsigned)E.NI * 4), dim3(256), 0, E.stream, qkv.p, kst, ctxp, att.p, HW);
        E.pend();
    }
    // to_out: Conv 1x1 + LayerNorm * g, and the Residual add, in one launch (the LayerNorm lives in the projection's epilogue)
    E.base(a, wo, H, W, H, W);
    Emitter2::plain(a.src[0], att);
    a.lnr_g = E.V(p + ".fn.fn.to_out.1.g");
    a.res = x.p; a.ldres = x.ld;
    a.out = out.p; a.ldo = out.ld;
    E.launch(wo, a);
    E.tap(p, out);
    E.release(scope);
    return out;
}

// Residual(PreNorm(Attention)) (:256-278) at the bottleneck
static Ten2 emit_fattn2(Emitter2& E, const std::string& p, const Ten2& x, const float* lnp) {
    cindm_unet2d* h = E.h;
    const int H = x.H, W = x.W, HW = H * W, C = x.C;
    const Packed2& wq0 = h->packed.at(p + ".fn.fn.to_qkv");
    const Packed2& wo0 = h->packed.at(p + ".fn.fn.to_out");
    const bool t3o = h->O("tail_h3") && h->packed.count(p + ".fn.fn.to_out#t3") && ((E.NI * (int64_t)HW) & 63) == 0;
    const bool t3q = h->O("tail_h3") && h->packed.count(p + ".fn.fn.to_qkv#t3") && C == 128 && ((E.NI * (int64_t)HW) & 63) == 0;
    const Packed2& wq = t3q ? h->packed.at(p + ".fn.fn.to_qkv#t3") : wq0;
    const Packed2& wo = t3o ? h->packed.at(p + ".fn.fn.to_out#t3") : wo0;
    Ten2 out = E.ten(H, W, C);
    const size_t scope = E.mark();
    Ten2 qkv = E.ten(H, W, 384), att = E.ten(H, W, 128);
    Conv2dArgs a;
    E.base(a, wq, H, W, H, W);
    if (t3q) {
        // LayerNorm * g as its own pass, then the projection as a plain-source GEMM on the split-fp16 tail kernel
        Ten2 xn = E.ten(H, W, C);
        ++E.launches;
        if (!E.dry) {
            const int64_t n4 = E.NI * (int64_t)HW * (C / 4);
            E.pbegin(6, 0.0);
            hipLaunchKernelGGL(ln_apply_kernel, dim3((unsigned)((n4 / 4 + 255) / 256)), dim3(256), 0, E.stream, x.p, lnp, C / 16, 16.f,
                               E.V(p + ".fn.norm.g"), xn.p, C, n4);
            E.pend();
        }
        Emitter2::plain(a.src[0], xn);
    } else {
        Src& s = a.src[0];
        s.p = x.p; s.ld = x.ld; s.C = C; s.mode = SRC2_LN; s.stats = lnp; s.P = C / 16; s.cnt = 16.f; s.gw = 1;
        s.gamma = E.V(p + ".fn.norm.g");
    }
    a.out = qkv.p; a.ldo = 384;
    E.launch(wq, a);
    ++E.launches;
    if (!E.dry) {
        E.pbegin(5, 2.0 * 2.0 * E.NI * 4.0 * (double)HW * HW * 32.0);
        if (h->use_h3 && HW % 128 == 0)
            hipLaunchKernelGGL(attn_full_h3b_kernel, dim3(HW / 128, (unsigned)E.NI * 4), dim3(256), 0, E.stream, qkv.p, att.p, HW);
        else if (h->use_h3) hipLaunchKernelGGL(attn_full_h3_kernel, dim3(HW / 64, (unsigned)E.NI * 4), dim3(256), 0, E.stream, qkv.p, att.p, HW);
        else hipLaunchKernelGGL(attn_full_kernel, dim3(HW / 64, (unsigned)E.NI * 4), dim3(256), 0, E.stream, qkv.p, att.p, HW);
        E.pend();
    }
    E.base(a, wo, H, W, H, W);
    if (t3o) a.bias = wo0.has_bias ? h->blob + wo0.bias_off : nullptr;
    Emitter2::plain(a.src[0], att);
    a.res = x.p; a.ldres = x.ld;
    a.out = out.p; a.ldo = out.ld;
    E.launch(wo, a);
    E.tap(p, out);
    E.release(scope);
    return out;
}

static Ten2 emit_conv2(Emitter2& E, const std::string& prefix, const std::string& tapname, const Ten2& x, int Hout, int Wout) {
    const Packed2& w = E.h->packed.at(prefix);
    Ten2 out = E.ten(Hout, Wout, w.N);
    Conv2dArgs a;
    E.base(a, w, x.H, x.W, Hout, Wout);
    Emitter2::plain(a.src[0], x);
    a.out = out.p; a.ldo = out.ld;
    E.launch(w, a);
    if (!tapname.empty()) E.tap(tapname, out);
    return out;
}

static int emit_forward2(Emitter2& E, const float* x, float* eps) {
    cindm_unet2d* h = E.h;
    const auto& d = h->d;
    const int n = d.n_mults, S = d.image_size, CP = h->CP();
    Ten2 in; in.p = const_cast<float*>(x); in.H = S; in.W = S; in.C = CP; in.ld = CP;
    Ten2 cur = emit_conv2(E, "init_conv", "init_conv", in, S, S);
    const Ten2 r = cur;
    std::vector<Ten2> skips;
    float* lnp = nullptr;
    for (int ind = 0; ind < n; ++ind) {
        const int ci = h->dims[ind];
        const std::string p = "downs." + std::to_string(ind);
        cur = emit_rb2(E, p + ".0", cur, nullptr, ci, false, nullptr);
        skips.push_back(cur);
        cur = emit_rb2(E, p + ".1", cur, nullptr, ci, !la_site_ok(h, p + ".2", cur.H * cur.W), &lnp);
        cur = emit_lattn2(E, p + ".2", cur, lnp);
        skips.push_back(cur);
        if (ind < n - 1) cur = emit_conv2(E, p + ".3.1", p + ".3", cur, cur.H / 2, cur.W / 2);
        else cur = emit_conv2(E, p + ".3", p + ".3", cur, cur.H, cur.W);
    }
    const int mid = h->dims[n];
    cur = emit_rb2(E, "mid_block1", cur, nullptr, mid, true, &lnp);
    cur = emit_fattn2(E, "mid_attn", cur, lnp);
    cur = emit_rb2(E, "mid_block2", cur, nullptr, mid, false, nullptr);
    for (int ind = 0; ind < n; ++ind) {
        const int ci = h->dims[n - 1 - ind], co = h->dims[n - ind];
        const std::string p = "ups." + std::to_string(ind);
        Ten2 s1 = skips.back(); skips.pop_back();
        cur = emit_rb2(E, p + ".0", cur, &s1, co, false, nullptr);
        Ten2 s2 = skips.back(); skips.pop_back();
        cur = emit_rb2(E, p + ".1", cur, &s2, co, !la_site_ok(h, p + ".2", cur.H * cur.W), &lnp);
        cur = emit_lattn2(E, p + ".2", cur, lnp);
        if (ind < n - 1) cur = emit_conv2(E, p + ".3.1", p + ".3", cur, cur.H * 2, cur.W * 2);
        else cur = emit_conv2(E, p + ".3", p + ".3", cur, cur.H, cur.W);
        (void)ci;
    }
    cur = emit_rb2(E, "final_res_block", cur, &r, d.dim, false, nullptr);
    {
        const Packed2& w = h->packed.at("final_conv");
        Conv2dArgs a;
        E.base(a, w, cur.H, cur.W, cur.H, cur.W);
        Emitter2::plain(a.src[0], cur);
        a.out = eps; a.ldo = CP;
        E.launch(w, a);
    }
    return 0;
}

static int unet2d_finalize_pack(cindm_unet2d* h, void* stream_) {
    REQUIRE(h, "null handle");
    hipStream_t stream = (hipStream_t)stream_;
    for (auto& p : h->params) if (!p.set) return fail("missing key in state_dict: " + p.name);
    const auto& d = h->d;
    const int T = d.timesteps, dim = d.dim, tdim = dim * 4;
    if (h->sinus.empty()) {
        h->sinus.resize((size_t)T * dim);
        const int half = dim / 2;
        const float e = (float)(std::log(10000.0) / (half - 1));
        for (int t = 0; t < T; ++t)
            for (int i = 0; i < half; ++i) {
                const float f = expf((float)i * -e), arg = (float)t * f;
                h->sinus[(size_t)t * dim + i] = sinf(arg);
                h->sinus[(size_t)t * dim + half + i] = cosf(arg);
            }
    }
    BlobBuilder bb;
    h->use_h3 = !h->O("mfma_f32") && !h->force_f32;
    // range rule of the split-fp16 products, as in cindm_unet1d_finalize.  The weight-standardised convolutions (.proj.) are
    // checked as the kernels see them, folded: they are O(1) only while a filter's variance is well above the fold's 1e-5;
    // a checkpoint of tiny .proj. weights folds to tiny tensors (x 2^-24: max 5e-7 .. 9e-7) whose planes lose 3e-5 of them.
    h->opt["range_fallback"] = h->force_f32 ? 2 : 0;
    if (h->use_h3 && h->O("auto_range")) {
        for (const auto& p : h->params) {
            if (p.shape.size() != 4) continue;
            const bool ws = p.name.find(".proj.") != std::string::npos;
            if (!(ws ? max_abs_in_fp16_window(ws_folded2(p)) : max_abs_in_fp16_window(p.host))) { h->use_h3 = false; h->opt["range_fallback"] = 1; break; }
        }
    }
    h->packed.clear(); h->lin.clear(); h->vec_off.clear(); h->tt_off.clear();
    std::vector<std::pair<std::string, int>> rbs;          // (prefix, Cout)
    int tt_ld = 0;
    for (const auto& p : h->params) {
        const std::string& k = p.name;
        auto ends = [&](const char* s) { size_t n = std::strlen(s); return k.size() >= n && k.compare(k.size() - n, n, s) == 0; };
        if (ends(".weight") && p.shape.size() == 4) {
            const std::string pre = k.substr(0, k.size() - 7);
            const bool ws = ends(".proj.weight");
            int kind = (p.shape[2] == 3) ? CONV_3X3 : (p.shape[2] == 7) ? CONV_STEM7 : CONV_1X1_WIDE, split = 0;
            if (pre.rfind("downs.", 0) == 0 && ends(".3.1.weight")) kind = CONV_UNSHUF;
            if (pre.rfind("ups.", 0) == 0 && ends(".3.1.weight")) kind = CONV_UP2;
            // concatenated inputs: ups.*.{0,1} (block1.proj, res_conv) = cat(x[Cout... see emit), final_res_block = cat(x, r)
            const bool cat_in = (pre.rfind("ups.", 0) == 0 || pre.rfind("final_res_block", 0) == 0) &&
                                (ends(".block1.proj.weight") || ends(".res_conv.weight"));
            if (cat_in) {
                // first source = running x: ups.i.{0,1}: dims[n - ind] channels; final_res_block: dim channels
                if (pre.rfind("final_res_block", 0) == 0) split = dim;
                else {
                    const int ind = std::stoi(pre.substr(4, pre.find('.', 4) - 4));
                    split = h->dims[d.n_mults - ind];
                }
            }
            if (pack_conv2d(h, bb, pre, kind, ws, split) != 0) return -1;
            if (h->use_h3 && h->O("la_site") && ends(".fn.fn.to_out.0.weight"))
                pack_la_site2(h, bb, k.substr(0, k.size() - std::strlen(".to_out.0.weight")));
        } else if (k == "time_mlp.1.weight" || k == "time_mlp.3.weight") {
            pack_linear2(h, bb, k.substr(0, k.size() - 7));
        } else if (ends(".mlp.1.weight")) {
            pack_linear2(h, bb, k.substr(0, k.size() - 7));
            const std::string rp = k.substr(0, k.size() - std::strlen(".mlp.1.weight"));
            h->tt_off[rp] = tt_ld;
            rbs.push_back({rp, (int)p.shape[0] / 2});
            tt_ld += ceil_to((int)p.shape[0], TN);
        } else if (ends(".norm.weight") || ends(".norm.bias") || ends(".g")) {
            pack_vec2(h, bb, k);
        }
    }
    // ResnetBlocks without res_conv: the 1x1 kernel's identity mode (no weights)
    for (int C : {dim, 2 * dim}) {
        Packed2 pk; pk.kind = CONV_1X1_WIDE; pk.identity = true; pk.CinP = C; pk.N = C; pk.Npad = C;
        h->packed["__identity" + std::to_string(C)] = pk;
    }
    h->tt_ld = tt_ld;
    if (h->blob) { (void)hipFree(h->blob); h->blob = nullptr; }
    if (h->ttable) { (void)hipFree(h->ttable); h->ttable = nullptr; }
    HIPCHK(hipMalloc((void**)&h->blob, bb.data.size() * sizeof(float)));
    HIPCHK(hipMemcpy(h->blob, bb.data.data(), bb.data.size() * sizeof(float), hipMemcpyHostToDevice));
    HIPCHK(hipMalloc((void**)&h->ttable, (size_t)T * tt_ld * sizeof(float)));
    HIPCHK(hipMemsetAsync(h->ttable, 0, (size_t)T * tt_ld * sizeof(float), stream));
    // time path for every timestep: sinus -> Linear -> GELU -> Linear -> per block SiLU -> Linear(2*Cout)
    float *sin_d = nullptr, *y1 = nullptr, *temb = nullptr;
    HIPCHK(hipMalloc((void**)&sin_d, (size_t)T * dim * sizeof(float)));
    HIPCHK(hipMalloc((void**)&y1, (size_t)T * tdim * sizeof(float)));
    HIPCHK(hipMalloc((void**)&temb, (size_t)T * tdim * sizeof(float)));
    HIPCHK(hipMemcpyAsync(sin_d, h->sinus.data(), (size_t)T * dim * sizeof(float), hipMemcpyHostToDevice, stream));
    Emitter E1{nullptr, stream, false, nullptr, 0, T, nullptr, 0};
    auto lin_launch = [&](const Packed& pk, const float* src, int C, int mode, float* out, int ldo) {
        GemmArgs a; std::memset(&a, 0, sizeof(a));
        a.W = h->blob + pk.off; a.bias = h->blob + pk.bias_off; a.CinP = pk.CinP; a.Npad = pk.Npad; a.N = pk.N; a.KC = pk.KC;
        a.Bp = T; a.Lin = 1; a.Lout = 1; a.stride = 1; a.pad = 0; a.spt = TM; a.nsrc = 1;
        a.lout_magic = 65536; a.lin_magic = 65536;
        a.src[0].p = src; a.src[0].ld = C; a.src[0].C = C; a.src[0].mode = mode; a.src[0].P = 1; a.src[0].gw = 1; a.src[0].cnt = 1.f;
        a.out = out; a.ldo = ldo;
        E1.launch(1, a);
    };
    lin_launch(h->lin.at("time_mlp.1"), sin_d, dim, SRC_PLAIN, y1, tdim);
    lin_launch(h->lin.at("time_mlp.3"), y1, tdim, SRC_GELU, temb, tdim);
    for (const auto& rbp : rbs)
        lin_launch(h->lin.at(rbp.first + ".mlp.1"), temb, tdim, SRC_SILU, h->ttable + h->tt_off.at(rbp.first), tt_ld);
    if (E1.err != hipSuccess) return fail(std::string("finalize launch: ") + hipGetErrorString(E1.err));
    HIPCHK(hipStreamSynchronize(stream));
    (void)hipFree(sin_d); (void)hipFree(y1); (void)hipFree(temb);
    Emitter2 D{h, nullptr, true, nullptr, 0, 1, nullptr, 0};
    emit_forward2(D, nullptr, nullptr);
    h->launches = D.launches;
    h->finalized = true;
    return 0;
}

extern "C" size_t cindm_unet2d_workspace_bytes(const cindm_unet2d* h, int64_t images) {
    if (!h || !h->finalized || images <= 0) return 0;
    Emitter2 D{const_cast<cindm_unet2d*>(h), nullptr, true, nullptr, 0, images, nullptr, 0};
    emit_forward2(D, nullptr, nullptr);
    return D.peak() + 256;
}
extern "C" int cindm_unet2d_launches_per_forward(const cindm_unet2d* h) { return h ? h->launches : 0; }

extern "C" int cindm_unet2d_forward(cindm_unet2d* h, const float* x, int32_t t, const int32_t* t_dev, float* eps,
                                    int64_t images, void* ws, size_t ws_bytes, void* stream) {
    REQUIRE(h && x && eps && ws, "null argument");
    REQUIRE(h->finalized, "cindm_unet2d_finalize has not been called");
    const int tpi = (h->d.image_size / T2Y) * (h->d.image_size / T2X);
    REQUIRE(images > 0 && images * tpi <= 65535, "too many images for one launch (grid.y limit)");
    REQUIRE(t_dev || (t >= 0 && t < h->d.timesteps), "timestep out of range");
    REQUIRE(ws_bytes >= cindm_unet2d_workspace_bytes(h, images), "workspace too small");
    REQUIRE(((uintptr_t)ws & 255) == 0 && ((uintptr_t)x & 15) == 0, "workspace must be 256-byte aligned, x 16-byte aligned");
    h->taps.clear(); h->taps_imgs = images;
    Emitter2 E{h, (hipStream_t)stream, false, (char*)ws, 0, images, t_dev, t};
    emit_forward2(E, x, eps);
    if (E.err != hipSuccess) return fail(std::string("kernel launch: ") + hipGetErrorString(E.err));
    return 0;
}

// finalize = repack (unet2d_finalize_pack) + calibration forward on the split-fp16 kernels, as cindm_unet1d_finalize
extern "C" int cindm_unet2d_finalize(cindm_unet2d* h, void* stream_) {
    REQUIRE(h, "null handle");
    if (h->finalized) return 0;
    h->force_f32 = false;
    if (unet2d_finalize_pack(h, stream_) != 0) return -1;
    if (!h->use_h3 || !h->O("auto_range")) return 0;
    const int HW = h->d.image_size * h->d.image_size, CP = h->CP();
    const size_t wsb = cindm_unet2d_workspace_bytes(h, 1);
    auto fwd = [&](int t, const float* x, float* eps, void* ws) { return cindm_unet2d_forward(h, x, t, nullptr, eps, 1, ws, wsb, stream_); };
    bool finite = true;       // (one image, device layout [pixel][padded channel])
    if (calibrate_at_finalize((size_t)HW * CP, h->d.channels, CP, 0x9E3779B1u, h->d.timesteps, wsb, (hipStream_t)stream_, fwd, &finite) != 0) return -1;
    h->taps.clear();
    if (!finite) {
        h->force_f32 = true;
        if (unet2d_finalize_pack(h, stream_) != 0) return -1;
    }
    return 0;
}

extern "C" int cindm_unet2d_profile(cindm_unet2d* h, const float* x, int32_t t, float* eps, int64_t images, void* ws,
                                    size_t ws_bytes, void* stream, int32_t counts[7], float ms[7], double flops[7]) {
    REQUIRE(h && x && eps && ws && counts && ms && flops, "null argument");
    REQUIRE(h->finalized, "cindm_unet2d_finalize has not been called");
    REQUIRE(t >= 0 && t < h->d.timesteps, "timestep out of range");
    REQUIRE(ws_bytes >= cindm_unet2d_workspace_bytes(h, images), "workspace too small");
    std::vector<Emitter2::ProfRec> recs;
    Emitter2 E{h, (hipStream_t)stream, false, (char*)ws, 0, images, nullptr, t};
    E.prof = &recs;
    h->taps.clear(); h->taps_imgs = images;
    emit_forward2(E, x, eps);
    hipError_t se = hipStreamSynchronize((hipStream_t)stream);
    for (int i = 0; i < 7; ++i) { counts[i] = 0; ms[i] = 0.f; flops[i] = 0.0; }
    for (auto& r : recs) {
        float dt = 0.f;
        (void)hipEventElapsedTime(&dt, r.e0, r.e1);
        counts[r.kind] += 1; ms[r.kind] += dt; flops[r.kind] += r.flops;
        (void)hipEventDestroy(r.e0); (void)hipEventDestroy(r.e1);
    }
    if (E.err != hipSuccess) return fail(std::string("kernel launch: ") + hipGetErrorString(E.err));
    if (se != hipSuccess) return fail(std::string("hipStreamSynchronize: ") + hipGetErrorString(se));
    return 0;
}

extern "C" int cindm_unet2d_tap(cindm_unet2d* h, const char* name, int64_t images, void* ws, float* dst, int64_t dst_cap,
                                int64_t shape[3], void* stream) {
    REQUIRE(h && name && ws && dst, "null argument");
    REQUIRE(images == h->taps_imgs, "tap: image count differs from the last forward");
    auto it = h->taps.find(name);
    if (it == h->taps.end()) return fail(std::string("unknown tap: ") + name);
    const int64_t n = images * it->second.HW * it->second.C;
    REQUIRE(n <= dst_cap, "tap: destination too small");
    shape[0] = images; shape[1] = it->second.HW; shape[2] = it->second.C;
    HIPCHK(hipMemcpyAsync(dst, (char*)ws + it->second.off, n * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return 0;
}

// x_T of the 2-D chains (ddpm2d_host.inc), drawn by the counter-based generator
extern "C" int cindm_fill_noise2d(float* x, int64_t B, int32_t nb, int32_t hw, int32_t channels, int32_t padded_channels,
                                  uint64_t seed, int64_t sample_offset, int32_t step_tag, void* stream) {
    REQUIRE(x && B > 0 && nb > 0, "bad argument");
    REQUIRE((padded_channels & 3) == 0 && B * nb * (int64_t)hw * padded_channels < (1ll << 31), "bad state size");
    const int64_t n = B * nb * (int64_t)hw * (padded_channels / 4);
    hipLaunchKernelGGL(fill_noise2d_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, (int)B, nb,
                       hw, channels, padded_channels, seed, sample_offset, (uint32_t)step_tag);
    HIPCHK(hipGetLastError());
    return 0;
}
