// Host side of the ForceUnet / airfoil design-gradient entry points (include/cindm_hip.h, section "ForceUnet").
// Reference: ForceUnet model/diffusion_2d.py:411-486; force_fn / overlap_fn / design_fn
// inference/inverse_design_2d.py:98-143, :208-214.  Forward ops are recorded with closures that, run in reverse, push
// the gradient back to the network input (weights are frozen: no weight gradients exist anywhere).
#include "forceunet.h"
#include "forceunet_la.h"
#include "forceunet_stem.h"
#include "forceunet_attn.h"
#include <deque>
#include <functional>

struct FuPacked { size_t off = 0, off_b = 0, bias = 0, off_h3 = 0, off_h3b = 0, off_sb = 0, off_sf3 = 0, off_sb3 = 0; bool has_bias = false, h3 = false, stem_b = false, unshuf = false; int KS = 1, Cin = 0, Cout = 0, CinP = 0, CoutP = 0, NB = 4, CinPb = 0, CoutPb = 0, NBb = 4; };

struct cindm_forceunet : ModelCore {
    cindm_forceunet_desc d;
    std::vector<int> dims;
    float* blob = nullptr;
    std::unordered_map<std::string, FuPacked> conv;
    std::unordered_map<std::string, size_t> vec;
    bool fwd_h3 = true;      // forward 3x3 convolutions on the diffusion path's persistent split-fp16 kernel (option "h3" = 0 / range fallback: off)
    bool bwd_h3 = true;      // ... and the input-gradient ones behind a GroupNorm, scaled by the gradient's maximum (option "h3_bwd" = 0: off)
    unsigned* err_dev = nullptr;       // raised by a timed-out exchange of fu_gn_silu_bwd_cluster_kernel (cindm_forceunet_status)
    int nx_force = 0;                  // the exchange-free re-run of a chain / gradient call is in progress
    int recovered = 0;                 // chains / calls re-run on the exchange-free derivative after a time-out
    // option "taps": where the block outputs of the last forward / grad / vjp call lie in the caller's workspace (cindm_forceunet_tap)
    struct Tap { size_t off_p, off_g; int C, H; };
    std::unordered_map<std::string, Tap> taps;
    int64_t taps_imgs = 0;
    bool taps_grad = false;            // that call ran the backward: the gradient at every tap exists
};

// kernel-path options (cindm_forceunet_set_option), as on the U-Net handles
static const OptDef kForceUnetOpts[] = {
    {"h3", 1, nullptr, OPT_PACK},             // forward 3x3 convolutions on the split-fp16 kernel (1) or the exact fp32-MFMA kernel (0)
    {"h3_bwd", 1, nullptr, OPT_PACK},         // ... the input-gradient ones
    {"auto_range", 1, nullptr, OPT_PACK},     // calibration forward at finalize
    {"range_fallback", 0, nullptr, OPT_READONLY},   // 1 when the range rule switched the forward convolutions to fp32
    {"stress", 0, nullptr, OPT_RUNTIME},      // > 0 (a seed): pseudo-random pauses before the in-kernel hand-overs (race tests)
    {"la_fused", 1, nullptr, OPT_PACK},       // LinearAttention sites of 64 / 128 channels without q | k | v tensors (forceunet_la.h); 0 = layer by layer
    // GroupNorm + SiLU derivative in one register-resident pass instead of reduce + apply: 1 = workgroup per (image, group),
    // 2 = workgroup per (image, slab of pixels) with whole rows, partial sums exchanged between the image's workgroups
    {"gn_bwd_fused", 2, nullptr, OPT_PACK},
    {"ws_nosplit", 2, nullptr, OPT_PACK},     // conv2d_ws_kernel: K of a chunk not split over the matrix waves (as on the 2-D U-Net)
    {"no_exchange", 0, nullptr, OPT_RUNTIME}, // 1 = no kernel that waits for another workgroup (gn_bwd_fused behaves as 1)
    {"recover", 1, nullptr, OPT_RUNTIME},     // 0: a timed-out exchange is an error instead of an exchange-free re-run
    {"dbg", 0, nullptr, OPT_RUNTIME},         // 39: force the exchange time-out (tests)
    // 1: every block output and its gradient stay readable after a call (cindm_forceunet_tap): a residual chain copies the gradient
    // into the destination's own buffer instead of sharing one (same arithmetic, same workspace).  Off on every sampling path.
    {"taps", 0, nullptr, OPT_RUNTIME},
};

extern "C" int cindm_forceunet_set_option(cindm_forceunet* h, const char* key, int32_t value) { return core_set_option(h, key, value) < 0 ? -1 : 0; }

// 1 when an in-kernel exchange of this handle timed out since the last call (the flag is cleared), 0 otherwise, -1 on error.
// Synchronises `stream`.
extern "C" int cindm_forceunet_status(cindm_forceunet* h, void* stream) {
    REQUIRE(h, "null handle");
    if (!h->err_dev) return 0;
    unsigned v = 0;
    HIPCHK(hipStreamSynchronize((hipStream_t)stream));
    HIPCHK(hipMemcpy(&v, h->err_dev, sizeof(v), hipMemcpyDeviceToHost));
    if (v) HIPCHK(hipMemset(h->err_dev, 0, sizeof(v)));
    return v ? 1 : 0;
}
extern "C" int cindm_forceunet_recovered(const cindm_forceunet* h) { return h ? h->recovered : 0; }

extern "C" int cindm_forceunet_get_option(const cindm_forceunet* h, const char* key, int32_t* value) { return core_get_option(h, key, value); }

extern "C" int cindm_forceunet_create(const cindm_forceunet_desc* desc, cindm_forceunet** out) {
    REQUIRE(desc && out, "null argument");
    REQUIRE(desc->dim == 64 && desc->n_mults >= 1 && desc->n_mults <= 4, "ForceUnet: dim must be 64, 1..4 levels");
    REQUIRE(desc->channels >= 1 && desc->channels <= 16, "ForceUnet: channels in [1, 16]");
    REQUIRE(desc->image_size >= 8 && (desc->image_size & (desc->image_size - 1)) == 0 && desc->image_size <= 128, "image_size must be a power of two in [8, 128]");
    {
        const int coarsest = desc->image_size >> (desc->n_mults - 1);
        REQUIRE(coarsest == 8 || coarsest == 16 || coarsest == 32,
                "ForceUnet: the coarsest level must be 8 x 8, 16 x 16 or 32 x 32 (pixel tiles are 8 x 8; the bottleneck attention streams "
                "its keys in chunks of 64 tokens, at most 1024): image_size = 8 * 2^(levels - 1) is the reference's shape (64, four levels)");
    }
    const int dim = desc->dim, n = desc->n_mults;
    std::vector<int> dims{dim};
    for (int i = 0; i < n; ++i) dims.push_back(dim * desc->dim_mults[i]);
    REQUIRE(dims[n] == 512, "ForceUnet: the bottleneck width must be 512 (final = Linear(512, 2), model/diffusion_2d.py:458)");
    for (int i = 0; i <= n; ++i)
        REQUIRE(dims[i] >= 64 && dims[i] <= 1024 && (dims[i] & (dims[i] - 1)) == 0,
                "ForceUnet: level widths must be powers of two in 64..1024 (GroupNorm kernels fix a channel quad per thread)");
    auto* h = new cindm_forceunet();
    h->d = *desc;
    h->dims = dims;
    h->init_options(kForceUnetOpts);
    auto conv = [&](const std::string& p, int ci, int co, int k, bool bias = true) {
        h->add_param(p + ".weight", {co, ci, k, k});
        if (bias) h->add_param(p + ".bias", {co});
    };
    auto rb = [&](const std::string& p, int c) {
        for (const char* b : {"block1", "block2"}) {
            conv(p + "." + b + ".proj", c, c, 3);
            h->add_param(p + "." + b + ".norm.weight", {c}); h->add_param(p + "." + b + ".norm.bias", {c});
        }
    };
    conv("init_conv", desc->channels, dim, 7);
    for (int ind = 0; ind < n; ++ind) {
        const int ci = h->dims[ind], co = h->dims[ind + 1];
        const std::string p = "downs." + std::to_string(ind);
        rb(p + ".0", ci); rb(p + ".1", ci);
        conv(p + ".2.fn.fn.to_qkv", ci, 384, 1, false);
        conv(p + ".2.fn.fn.to_out.0", 128, ci, 1);
        h->add_param(p + ".2.fn.fn.to_out.1.g", {1, ci, 1, 1});
        h->add_param(p + ".2.fn.norm.g", {1, ci, 1, 1});
        if (ind < n - 1) conv(p + ".3.1", ci * 4, co, 1); else conv(p + ".3", ci, co, 3);
    }
    const int mid = h->dims[n];
    rb("mid_block1", mid);
    conv("mid_attn.fn.fn.to_qkv", mid, 384, 1, false);
    conv("mid_attn.fn.fn.to_out", 128, mid, 1);
    h->add_param("mid_attn.fn.norm.g", {1, mid, 1, 1});
    rb("mid_block2", mid);
    h->add_param("final.weight", {2, 512}); h->add_param("final.bias", {2});
    *out = h;
    return 0;
}
extern "C" void cindm_forceunet_destroy(cindm_forceunet* h) {
    if (!h) return;
    if (h->blob) (void)hipFree(h->blob);
    if (h->err_dev) (void)hipFree(h->err_dev);
    delete h;
}
extern "C" int cindm_forceunet_num_params(const cindm_forceunet* h) { return core_num_params(h); }
extern "C" int cindm_forceunet_param_info(const cindm_forceunet* h, int idx, char* name, int cap, int64_t shape[4], int* ndim) {
    return core_param_info(h, idx, name, cap, shape, ndim);
}
extern "C" int cindm_forceunet_set_param(cindm_forceunet* h, const char* key, const float* src, int64_t numel, int on_device) {
    return core_set_param(h, key, src, numel, on_device);
}

// conv weight [Co][Ci][KS][KS] -> forward fragments Wp[tap][kc][ntq][lane][NB] and the backward-data ones (input <->
// output channels swapped, taps flipped).  WeightStandardizedConv2d (:111-124) is folded here (biased variance, eps 1e-5).
static std::vector<float> fu_ws_folded(const Param& w) {
    const int Co = (int)w.shape[0];
    std::vector<float> W(w.host);
    const size_t per = w.numel / Co;
    for (int o = 0; o < Co; ++o) {
        double m = 0.0;
        for (size_t i = 0; i < per; ++i) m += W[o * per + i];
        m /= (double)per;
        const float mf = (float)m;
        double v = 0.0;
        for (size_t i = 0; i < per; ++i) { const double dd = (double)W[o * per + i] - m; v += dd * dd; }
        const float rs = 1.0f / sqrtf((float)(v / (double)per) + 1e-5f);
        for (size_t i = 0; i < per; ++i) W[o * per + i] = (W[o * per + i] - mf) * rs;
    }
    return W;
}

static void fu_pack_conv(cindm_forceunet* h, BlobBuilder& bb, const std::string& prefix, bool ws) {
    const Param& w = h->params[h->index.at(prefix + ".weight")];
    const int Co = (int)w.shape[0], Ci = (int)w.shape[1], KS = (int)w.shape[2], T = KS * KS;
    std::vector<float> W = ws ? fu_ws_folded(w) : w.host;
    const bool unshuf = KS == 1 && prefix.size() > 4 && prefix.compare(prefix.size() - 4, 4, ".3.1") == 0;
    if (unshuf) {
        // the 1x1 behind 'b c (h p1) (w p2) -> b (c p1 p2) h w': input channel c*4 + p moves to p*C + c, so that the kernels
        // read / write 4 consecutive channels of one full-resolution pixel (fu_conv_kernel<1, 4, UNSHUF>)
        const int C = Ci / 4;
        std::vector<float> P(W.size());
        for (int o = 0; o < Co; ++o)
            for (int c = 0; c < C; ++c)
                for (int pp = 0; pp < 4; ++pp) P[(size_t)o * Ci + pp * C + c] = W[(size_t)o * Ci + c * 4 + pp];
        W.swap(P);
    }
    FuPacked pk; pk.KS = KS; pk.Cin = Ci; pk.Cout = Co; pk.unshuf = unshuf;
    auto pack = [&](int cin, int cout, bool bwd, size_t& off, int& cinp, int& coutp, int& nb) {
        nb = (cout % 64 == 0) ? 4 : 1;
        cinp = ceil_to(cin, 16); coutp = ceil_to(cout, 16 * nb);
        const int kcs = cinp / 4, nq = coutp / (16 * nb);
        off = bb.alloc((size_t)T * kcs * nq * 64 * nb);
        float* base = bb.data.data() + off;
        for (int tap = 0; tap < T; ++tap)
            for (int kc = 0; kc < kcs; ++kc)
                for (int q = 0; q < nq; ++q)
                    for (int lane = 0; lane < 64; ++lane)
                        for (int e = 0; e < nb; ++e) {
                            const int ci = kc * 4 + (lane >> 4), co = (q * nb + e) * 16 + (lane & 15);
                            float v = 0.f;
                            if (ci < cin && co < cout) {
                                // forward: x channel ci -> y channel co, tap (ty, tx); backward: dy channel ci (= Co index) -> dx channel co (= Ci index), flipped tap
                                if (!bwd) v = W[((size_t)co * Ci + ci) * T + tap];
                                else v = W[((size_t)ci * Ci + co) * T + (T - 1 - tap)];
                            }
                            base[((((size_t)tap * kcs + kc) * nq + q) * 64 + lane) * nb + e] = v;
                        }
    };
    pack(Ci, Co, false, pk.off, pk.CinP, pk.CoutP, pk.NB);
    pack(Co, Ci, true, pk.off_b, pk.CinPb, pk.CoutPb, pk.NBb);
    if (KS == 7 && Ci == 4 && Co == 64) {
        // fu_stem_bwd_kernel: Wp[a][co][n = b*4 + ci] = W[co][ci][6 - a][6 - b], columns 28..31 zero
        pk.stem_b = true;
        pk.off_sb = bb.alloc((size_t)7 * 64 * 32);
        float* base = bb.data.data() + pk.off_sb;
        for (int a_ = 0; a_ < 7; ++a_)
            for (int co = 0; co < 64; ++co)
                for (int n = 0; n < 32; ++n) {
                    const int b_ = n >> 2, ci = n & 3;
                    base[((size_t)a_ * 64 + co) * 32 + n] = b_ < 7 ? W[((size_t)co * Ci + ci) * T + (6 - a_) * 7 + (6 - b_)] : 0.f;
                }
        // split-fp16 fragments of fu_stem_h3_kernel / fu_stem_bwd_h3_kernel (forceunet_stem.h)
        auto put = [](uint16_t* hi, uint16_t* lo, float v) {
            const _Float16 hv = (_Float16)v, lv = (_Float16)((v - (float)hv) * H3_SCALE);
            std::memcpy(hi, &hv, 2); std::memcpy(lo, &lv, 2);
        };
        pk.off_sf3 = bb.alloc((size_t)7 * 4 * 2 * 64 * 8 / 2);
        pk.off_sb3 = bb.alloc((size_t)7 * 2 * 2 * 2 * 64 * 8 / 2);
        uint16_t* f16 = reinterpret_cast<uint16_t*>(bb.data.data() + pk.off_sf3);
        uint16_t* b16 = reinterpret_cast<uint16_t*>(bb.data.data() + pk.off_sb3);
        for (int ta = 0; ta < 7; ++ta)
            for (int lane = 0; lane < 64; ++lane)
                for (int j = 0; j < 8; ++j) {
                    const int lr = lane & 15, lq = lane >> 4;
                    for (int tile = 0; tile < 4; ++tile) {
                        const int dx = 2 * lq + (j >> 2), ci = j & 3, co = tile * 16 + lr;
                        const float v = dx < 7 ? W[((size_t)co * Ci + ci) * T + ta * 7 + dx] : 0.f;
                        const size_t q = ((size_t)(ta * 4 + tile) * 2) * 64 * 8;
                        put(f16 + q + (size_t)lane * 8 + j, f16 + q + 64 * 8 + (size_t)lane * 8 + j, v);
                    }
                    for (int kk = 0; kk < 2; ++kk)
                        for (int nb = 0; nb < 2; ++nb) {
                            const int n = nb * 16 + lr, b_ = n >> 2, ci = n & 3, co = kk * 32 + lq * 8 + j;
                            const float v = b_ < 7 ? W[((size_t)co * Ci + ci) * T + (6 - ta) * 7 + (6 - b_)] : 0.f;
                            const size_t q = ((size_t)((ta * 2 + kk) * 2 + nb) * 2) * 64 * 8;
                            put(b16 + q + (size_t)lane * 8 + j, b16 + q + 64 * 8 + (size_t)lane * 8 + j, v);
                        }
                }
    }
    if (KS == 3 && Ci % 64 == 0 && Co % 64 == 0) {
        // the forward pass of these layers also has conv2d_ws_kernel's weight layout (unet2d_host.inc, pack_conv2d):
        // [n-tile of 64][chunk of 64 channels][tap][q = nb*2 + plane][thread][8 halfs], hi / scaled-lo fp16
        pk.h3 = true;
        auto bits = [](float v) { _Float16 hv = (_Float16)v; uint16_t u; std::memcpy(&u, &hv, 2); return u; };
        // bwd: the input-gradient convolution = the same kernel over dy with input <-> output channels swapped, taps flipped
        auto pack_h3 = [&](bool bwd, size_t& off) {
            const int cin = bwd ? Co : Ci, cout = bwd ? Ci : Co;
            const int nch = cin / 64, ntl = cout / 64;
            const size_t halfs = (size_t)ntl * nch * 9 * 4 * 256 * 8;
            off = bb.alloc(halfs / 2);
            uint16_t* base = reinterpret_cast<uint16_t*>(bb.data.data() + off);
            for (int nt = 0; nt < ntl; ++nt)
                for (int ch = 0; ch < nch; ++ch)
                    for (int tap = 0; tap < 9; ++tap)
                        for (int nb = 0; nb < 2; ++nb)
                            for (int tid = 0; tid < 256; ++tid) {
                                const int wv_ = tid >> 6, lane = tid & 63, kg = wv_ & 1, nh = wv_ >> 1;
                                const int n = nt * 64 + nh * 32 + nb * 16 + (lane & 15);
                                for (int e = 0; e < 8; ++e) {
                                    const int c = ch * 64 + kg * 32 + (lane >> 4) * 8 + e;
                                    const float v = bwd ? W[((size_t)c * Ci + n) * T + (8 - tap)] : W[((size_t)n * Ci + c) * T + tap];
                                    const _Float16 hv = (_Float16)v;
                                    const size_t q0 = ((((size_t)nt * nch + ch) * 9 + tap) * 4 + nb * 2) * 256;
                                    base[(q0 + tid) * 8 + e] = bits((float)hv);
                                    base[(q0 + 256 + tid) * 8 + e] = bits((v - (float)hv) * H3_SCALE);
                                }
                            }
        };
        pack_h3(false, pk.off_h3);
        pack_h3(true, pk.off_h3b);
    }
    auto bi = h->index.find(prefix + ".bias");
    if (bi != h->index.end()) {
        pk.has_bias = true;
        pk.bias = bb.alloc(Co);
        std::memcpy(bb.data.data() + pk.bias, h->params[bi->second].host.data(), Co * sizeof(float));
    }
    h->conv[prefix] = pk;
}

extern "C" int cindm_forceunet_finalize(cindm_forceunet* h, void* stream) {
    REQUIRE(h, "null handle");
    if (h->finalized) return 0;
    if (!h->err_dev) { HIPCHK(hipMalloc((void**)&h->err_dev, 256)); HIPCHK(hipMemset(h->err_dev, 0, 256)); }
    for (auto& p : h->params) if (!p.set) return fail("missing key in state_dict: " + p.name);
    BlobBuilder bb;
    h->conv.clear(); h->vec.clear();
    for (const auto& p : h->params) {
        const std::string& k = p.name;
        auto ends = [&](const char* s) { size_t n = std::strlen(s); return k.size() >= n && k.compare(k.size() - n, n, s) == 0; };
        if (ends(".weight") && p.shape.size() == 4) fu_pack_conv(h, bb, k.substr(0, k.size() - 7), ends(".proj.weight"));
        else if (ends(".norm.weight") || ends(".norm.bias") || ends(".g") || k == "final.weight" || k == "final.bias") {
            const size_t o = bb.alloc(p.numel);
            std::memcpy(bb.data.data() + o, p.host.data(), p.numel * sizeof(float));
            h->vec[k] = o;
        }
    }
    // LinearAttention sites with 64 / 128 channels: the la2d_* split-fp16 fragments of to_qkv / to_out.0 (kernels2d.h) and the
    // fp32 fragments of the transposed products of the input-gradient pass (forceunet_la.h)
    for (int ind = 0; ind < h->d.n_mults; ++ind) {
        const std::string ap = "downs." + std::to_string(ind) + ".2.fn.fn";
        const Param& wq = h->params[h->index.at(ap + ".to_qkv.weight")];
        const Param& wo = h->params[h->index.at(ap + ".to_out.0.weight")];
        const int C = (int)wq.shape[1];
        if (C != 64 && C != 128) continue;
        auto bits = [](float v) { _Float16 hv = (_Float16)v; uint16_t u; std::memcpy(&u, &hv, 2); return u; };
        auto frag_h3 = [&](const Param& w, int Co, int Ci, const std::string& name) {
            const int K32 = Ci / 32;
            const size_t o = bb.alloc((size_t)(Co / 16) * K32 * 2 * 64 * 4);
            uint16_t* base = reinterpret_cast<uint16_t*>(bb.data.data() + o);
            for (int t = 0; t < Co / 16; ++t)
                for (int k = 0; k < K32; ++k)
                    for (int lane = 0; lane < 64; ++lane)
                        for (int e = 0; e < 8; ++e) {
                            const float v = w.host[(size_t)(t * 16 + (lane & 15)) * Ci + k * 32 + (lane >> 4) * 8 + e];
                            const _Float16 hv = (_Float16)v;
                            const size_t q0 = ((size_t)t * K32 + k) * 2;
                            base[((q0 + 0) * 64 + lane) * 8 + e] = bits((float)hv);
                            base[((q0 + 1) * 64 + lane) * 8 + e] = bits((v - (float)hv) * 2048.0f);
                        }
            h->vec[name] = o;
        };
        frag_h3(wq, 384, C, ap + "#la.qkv");
        frag_h3(wo, C, 128, ap + "#la.out");
        // split-fp16 fragments of the transposed matrices of the input-gradient pass (same [tile][k32][plane][lane][8] form):
        // Wo^T [128 x C], Wq^T [C x 128], [Wk^T | Wv^T] [C x 256]
        auto frag_h3_mat = [&](const std::vector<float>& M, int Co, int Ci, const std::string& name) {
            Param tmp; tmp.host = M;
            frag_h3(tmp, Co, Ci, name);
        };
        {
            std::vector<float> woT((size_t)128 * C), wqT((size_t)C * 128), wkvT((size_t)C * 256);
            for (int c = 0; c < C; ++c)
                for (int j = 0; j < 128; ++j) {
                    woT[(size_t)j * C + c] = wo.host[(size_t)c * 128 + j];
                    wqT[(size_t)c * 128 + j] = wq.host[(size_t)j * C + c];
                    wkvT[(size_t)c * 256 + j] = wq.host[(size_t)(128 + j) * C + c];
                    wkvT[(size_t)c * 256 + 128 + j] = wq.host[(size_t)(256 + j) * C + c];
                }
            frag_h3_mat(woT, 128, C, ap + "#la.WoT");
            frag_h3_mat(wqT, C, 128, ap + "#la.WqT");
            frag_h3_mat(wkvT, C, 256, ap + "#la.WkvT");
        }
    }
    if (h->blob) { (void)hipFree(h->blob); h->blob = nullptr; }
    HIPCHK(hipMalloc((void**)&h->blob, bb.data.size() * sizeof(float)));
    HIPCHK(hipMemcpy(h->blob, bb.data.data(), bb.data.size() * sizeof(float), hipMemcpyHostToDevice));
    h->finalized = true;
    h->fwd_h3 = h->O("h3") != 0;
    h->bwd_h3 = h->O("h3_bwd") != 0;
    h->opt["range_fallback"] = 0;
    if (h->fwd_h3 && h->O("auto_range")) {
        // weight window of the range rule (as cindm_unet1d_finalize): the convolutions that are NOT weight-standardised feed
        // the un-normalised residual stream, whose scale the split-fp16 3x3 convolutions then see as their input.  fp16
        // subnormals survive pack, staging and MFMA (measured at max|w| = 2^-12, where a quarter of the hi plane and most of
        // the lo plane are subnormal: tests/test_gpu_f64_range.py, DESIGN 4.8), so nothing flushes inside the window; below
        // it hi and lo run out of subnormal bits together -- a silent loss -- and above it hi overflows.  A weight outside
        // switches the forward convolutions to the exact fp32 kernel.  The input-gradient ones rescale the gradient by its
        // maximum and reuse the weight planes, which the window already covers: held to the same budget at both edges there.
        for (const auto& p : h->params) {
            if (p.shape.size() != 4 || p.name.find(".proj.") != std::string::npos) continue;
            if (!max_abs_in_fp16_window(p.host)) { h->fwd_h3 = false; h->opt["range_fallback"] = 1; break; }
        }
        // The weight-standardised convolutions are the ones that RUN on the split-fp16 kernels, on the planes of the FOLDED
        // weights.  Those are O(1) only while a filter's variance is well above the fold's 1e-5: tiny .proj. weights fold to
        // tiny tensors (x 2^-24: max 5e-7 .. 9e-7, planes 3e-5 off), and the same window applies to them.
        for (const auto& p : h->params) {
            if (!h->fwd_h3 || p.shape.size() != 4 || p.name.find(".proj.") == std::string::npos) continue;
            if (!max_abs_in_fp16_window(fu_ws_folded(p))) { h->fwd_h3 = false; h->opt["range_fallback"] = 1; break; }
        }
    }
    if (h->fwd_h3 && h->O("auto_range")) {
        // range guard as in the diffusion U-Nets: one calibration forward (unit-scale image) on the split-fp16 convolutions;
        // a non-finite output switches this handle's forward convolutions back to the fp32 MFMA kernel
        const int S = h->d.image_size; const size_t n = (size_t)S * S * h->d.channels;     // one image, [pixel][channels]
        std::vector<float> hx(n); uint32_t stt = 0x2545F491u;
        for (auto& v : hx) { float a = 0.f; for (int k = 0; k < 4; ++k) { stt = stt * 1664525u + 1013904223u; a += (float)(stt >> 8) * (1.0f / 16777216.0f); } v = (a - 2.0f) * 1.7320508f; }
        float *dx = nullptr, *dout = nullptr; void* ws = nullptr;
        const size_t wsb = cindm_forceunet_workspace_bytes(h, 1, 0);
        HIPCHK(hipMalloc((void**)&dx, n * 4)); HIPCHK(hipMalloc((void**)&dout, 2 * 4)); HIPCHK(hipMalloc(&ws, wsb));
        HIPCHK(hipMemcpy(dx, hx.data(), n * 4, hipMemcpyHostToDevice));
        float ho[2] = {0.f, 0.f};
        const int rc = cindm_forceunet_forward(h, dx, dout, 1, ws, wsb, stream);
        if (rc == 0) { HIPCHK(hipStreamSynchronize((hipStream_t)stream)); HIPCHK(hipMemcpy(ho, dout, 8, hipMemcpyDeviceToHost)); }
        (void)hipFree(dx); (void)hipFree(dout); (void)hipFree(ws);
        if (rc != 0 || !std::isfinite(ho[0]) || !std::isfinite(ho[1])) { h->fwd_h3 = false; h->opt["range_fallback"] = 1; }
    }
    return 0;
}

// ---- forward recording / reverse replay -----------------------------------------------------------------------------
struct FT { float* p = nullptr; float* g = nullptr; int C = 0, H = 0; bool gset = false;
            unsigned* amax = nullptr;
            // p == nullptr: the tensor is SiLU(GroupNorm(gn_src)) and was never written -- its one consumer (the ResnetBlock's second 3x3
            // on conv2d_ws_kernel) applies it while staging (option gn_on_load): gn_part = the producer's [image][8][gn_P][2] partials
            const float* gn_src = nullptr; const float* gn_part = nullptr; const float* gn_gamma = nullptr; const float* gn_beta = nullptr; int gn_P = 0; };    // [images] bit patterns of max |g| per image (written with g by the GroupNorm backward): conv2d_ws_kernel<.., SRC2_SCALED>

struct FuRun {
    cindm_forceunet* h; hipStream_t st; char* ws; size_t off = 0; bool dry; int64_t NI; bool want_grad;
    bool taps = false;                 // option "taps" on an entry that serves them: pass_grad copies instead of sharing
    std::deque<FT> ts;
    std::vector<std::function<void()>> bwd;
    hipError_t err = hipSuccess;
    float* alloc(size_t n) { size_t o = off; off += ((n * 4 + 255) / 256) * 256; return dry ? nullptr : reinterpret_cast<float*>(ws + o); }
    FT* ten(int C, int H) { ts.emplace_back(); FT& t = ts.back(); t.C = C; t.H = H; t.p = alloc((size_t)NI * H * H * C); if (want_grad) t.g = alloc((size_t)NI * H * H * C); return &t; }
    const float* V(const std::string& k) const { return h->blob + h->vec.at(k); }
    int64_t numel(const FT* t) const { return NI * (int64_t)t->H * t->H * t->C; }
    static unsigned blocks(int64_t n) { return (unsigned)((n + 255) / 256); }
    void chk() { hipError_t e = hipGetLastError(); if (e != hipSuccess && err == hipSuccess) err = e; }
    float beta_of(FT* t) { const float b = t->gset ? 1.f : 0.f; t->gset = true; return b; }

    // dst.g += src.g where src is dead after the calling backward step: the FIRST contribution to dst shares src's buffer
    // instead of copying it (later contributions accumulate into that buffer in place; every user reads ->g when it runs).
    // With taps the first contribution is copied into dst's own buffer (every FT has one from ten()), so that src.g survives the
    // call: copying, then accumulating the same contributions in the same order, is the same arithmetic bit for bit.
    void pass_grad(FT* src, FT* dst) {
        if (!dst->gset) {
            dst->gset = true;
            if (!taps) { dst->g = src->g; return; }
            hipLaunchKernelGGL(fu_add_kernel, dim3(blocks(numel(src))), dim3(256), 0, st, src->g, dst->g, 0.f, numel(src));
            return;
        }
        hipLaunchKernelGGL(fu_add_kernel, dim3(blocks(numel(src))), dim3(256), 0, st, src->g, dst->g, 1.f, numel(src));
    }
    void conv_launch(const FuPacked& pk, bool bwd_w, const float* x, float* y, int H, float beta, bool use_bias, int unshuf_src = 0) {
        FuConvArgs a;
        a.x = x; a.y = y; a.H = H; a.Wd = H; a.NI = (int)NI; a.beta = beta; a.Csrc = 0;
        if (!bwd_w) { a.W = h->blob + pk.off; a.Cin = pk.Cin; a.CinP = pk.CinP; a.Cout = pk.Cout; a.CoutP = pk.CoutP; }
        else { a.W = h->blob + pk.off_b; a.Cin = pk.Cout; a.CinP = pk.CinPb; a.Cout = pk.Cin; a.CoutP = pk.CoutPb; }
        a.bias = (use_bias && pk.has_bias && !bwd_w) ? h->blob + pk.bias : nullptr;
        const int nb = bwd_w ? pk.NBb : pk.NB;
        const dim3 grid((unsigned)(a.CoutP / (16 * nb)), (unsigned)(NI * (H / 8) * (H / 8)));
#define FU_CONV(KS_, NB_) hipLaunchKernelGGL((fu_conv_kernel<KS_, NB_>), grid, dim3(256), 0, st, a)
        if (pk.KS == 7) { if (nb == 4) FU_CONV(7, 4); else FU_CONV(7, 1); }
        else if (pk.KS == 3) { if (nb == 4) FU_CONV(3, 4); else FU_CONV(3, 1); }
        else if (unshuf_src) {                             // 1x1 behind the pixel-unshuffle: H is the half resolution, Cin (Cout) = 4 * Csrc
            a.Csrc = unshuf_src;
            if (!bwd_w) hipLaunchKernelGGL((fu_conv_kernel<1, 4, 1>), grid, dim3(256), 0, st, a);
            else hipLaunchKernelGGL((fu_conv_kernel<1, 4, 2>), grid, dim3(256), 0, st, a);
        }
        else { if (nb == 4) FU_CONV(1, 4); else FU_CONV(1, 1); }
#undef FU_CONV
        chk();
    }
    bool ws_ok(const FuPacked& pk, int H) const {
        // 8 x 16 pixel tiles; the 8 x 8 level pairs two images per tile (CONV_3X3_PAIR)
        const bool geom = (H % V2Y == 0 && H % V2X == 0) || (H == 8 && NI % 2 == 0);
        return pk.h3 && geom && (double)NI * H * H * 4.0 * std::max(pk.Cin, pk.Cout) < 2147483648.0;
    }
    // 3x3 convolution on the diffusion path's persistent split-fp16 kernel: forward (x -> y, bias) or input gradient
    // (dy -> dx [+= when beta], flipped / transposed weights, dy scaled by the power of two its maximum *amax asks for)
    void conv_ws_launch(const FuPacked& pk, bool bwd_w, const float* x, float* y, int H, float beta, const unsigned* amax, float* gn_part = nullptr,
                        const FT* gsrc = nullptr) {
        Conv2dArgs a; std::memset(&a, 0, sizeof(a));
        const int cin = bwd_w ? pk.Cout : pk.Cin, cout = bwd_w ? pk.Cin : pk.Cout;
        a.src[0].p = x; a.src[0].ld = cin; a.src[0].C = cin; a.src[0].mode = bwd_w ? SRC2_SCALED : SRC2_PLAIN; a.src[0].P = 1; a.src[0].gw = 1; a.src[0].cnt = 1.f;
        a.src[0].stats = reinterpret_cast<const float*>(amax);
        if (gsrc) {      // forward over SiLU(GroupNorm(gsrc->gn_src)), normalised while the window is staged (no time scale / shift here)
            Src& s = a.src[0];
            s.p = gsrc->gn_src; s.mode = SRC2_GN_SS_SILU; s.stats = gsrc->gn_part; s.P = gsrc->gn_P; s.gw = cin / 8; s.cnt = (float)(V2M / WS_SPT * (cin / 8));
            s.gamma = gsrc->gn_gamma; s.beta = gsrc->gn_beta;
        }
        a.nsrc = 1; a.W = h->blob + (bwd_w ? pk.off_h3b : pk.off_h3); a.bias = (!bwd_w && pk.has_bias) ? h->blob + pk.bias : nullptr;
        a.CinP = cin; a.Npad = cout; a.N = cout;
        const bool pair = H == 8;
        a.NI = pair ? (int)(NI / 2) : (int)NI; a.Hin = H; a.Win = H; a.Hout = H; a.Wout = H;
        a.tiles_x = pair ? 1 : H / V2X; a.tpi = pair ? 1 : (H / V2Y) * (H / V2X);
        a.out = y; a.ldo = cout; a.rows_total = NI * (int64_t)H * H;
        if (bwd_w && beta != 0.f) { a.res = y; a.ldres = cout; }
        if (gn_part) { a.stats_out = gn_part; a.so_gw = cout / 8; }     // GroupNorm (mean, M2) partials per (tile, memory wave)
        a.stress = h->O("stress");
        // as the diffusion U-Net's selection (unet2d_host.inc): the k-groups stay where their reduction is amortised over several 64-channel
        // chunks -- plain-source and input-gradient layers of more than one chunk, the paired 8 x 8 level (8 chunks) -- and go elsewhere
        // (round 5's first surrogate trace with K never split: conv2d_ws<0,5> 353 -> 373 us, <6,5> 317 -> 368 us per launch)
        const int nsv = h->O("ws_nosplit");
        const bool ksplit = nsv == 0 || (nsv == 2 && !gsrc && cin > 64);
#define FU_WS(KIND_, MODE_) do { if (ksplit) hipLaunchKernelGGL((conv2d_ws_kernel<KIND_, MODE_, 0>), dim3(WS_GRID), dim3(512), 0, st, a); \
                                 else hipLaunchKernelGGL((conv2d_ws_kernel<KIND_, MODE_, 1>), dim3(WS_GRID), dim3(512), 0, st, a); } while (0)
        if (pair) { if (bwd_w) FU_WS(CONV_3X3_PAIR, SRC2_SCALED); else FU_WS(CONV_3X3_PAIR, SRC2_PLAIN); }
        else if (gsrc) FU_WS(CONV_3X3, SRC2_GN_SS_SILU);
        else { if (bwd_w) FU_WS(CONV_3X3, SRC2_SCALED); else FU_WS(CONV_3X3, SRC2_PLAIN); }
#undef FU_WS
        chk();
    }
    // GroupNorm statistics of a convolution's output straight from the split-fp16 kernel's store path: tiles inside one
    // image (not the paired 8 x 8 level), groups of 8 or 16 channels (what the kernel's partial sums are written for)
    bool gn_fused(const FuPacked& pk, int H) const { return h->fwd_h3 && ws_ok(pk, H) && H != 8 && (pk.Cout == 64 || pk.Cout == 128); }
    // gn_part_follows: the caller is block() -- a GroupNorm consumes the output and its backward leaves the gradient's maximum
    FT* conv(FT* x, const std::string& name, float* gn_part = nullptr, bool gn_part_follows = false) {
        const FuPacked& pk = h->conv.at(name);
        FT* y = ten(pk.Cout, x->H);
        if (!dry) {
            if (x->gn_src) conv_ws_launch(pk, false, nullptr, y->p, x->H, 0.f, nullptr, gn_part, x);      // (block() checked that this path serves it)
            else if (h->fwd_h3 && ws_ok(pk, x->H)) conv_ws_launch(pk, false, x->p, y->p, x->H, 0.f, nullptr, gn_part);
            else if (h->fwd_h3 && pk.stem_b && pk.has_bias && (x->H == 64 || x->H == 32 || x->H == 16)) {
                FuStemArgs sa{x->p, h->blob + pk.off_sf3, h->blob + pk.bias, y->p, x->H, (int)NI};
                const dim3 grid((unsigned)(NI * (x->H / 8)));
                if (x->H == 64) hipLaunchKernelGGL(fu_stem_h3_kernel<64>, grid, dim3(256), 0, st, sa);
                else if (x->H == 32) hipLaunchKernelGGL(fu_stem_h3_kernel<32>, grid, dim3(256), 0, st, sa);
                else hipLaunchKernelGGL(fu_stem_h3_kernel<16>, grid, dim3(256), 0, st, sa);
                chk();
            }
            else conv_launch(pk, false, x->p, y->p, x->H, 0.f, true);
        }
        // input gradient: split-fp16 too when the GroupNorm backward left the gradient's maximum (block()); exact fp32 MFMA otherwise
        unsigned* own_amax = (want_grad && h->bwd_h3 && pk.KS == 3 && ws_ok(pk, x->H) && !gn_part_follows) ? reinterpret_cast<unsigned*>(alloc((size_t)NI)) : nullptr;
        if (want_grad && !dry) bwd.push_back([this, x, y, &pk, own_amax] {
            if (pk.stem_b && x->H == 64 && h->bwd_h3) {
                FuStemBwdH3Args sa{y->g, h->blob + pk.off_sb3, x->g, x->H, (int)NI, beta_of(x)};
                hipLaunchKernelGGL(fu_stem_bwd_h3_kernel, dim3((unsigned)(NI * (x->H / 16))), dim3(256), 0, st, sa);
                chk();
            } else if (pk.stem_b && x->H == 64) {
                FuStemBwdArgs sa{y->g, h->blob + pk.off_sb, x->g, x->H, (int)NI, beta_of(x)};
                hipLaunchKernelGGL(fu_stem_bwd_kernel, dim3((unsigned)(NI * (x->H / 4))), dim3(256), 0, st, sa);
                chk();
            } else if (y->amax) conv_ws_launch(pk, true, y->g, x->g, x->H, beta_of(x), y->amax);
            else if (own_amax) {
                // a 3x3 convolution not behind a GroupNorm (the last level's down-sampling one): its own maximum pass first
                (void)hipMemsetAsync(own_amax, 0, (size_t)NI * sizeof(unsigned), st);
                {
                    const int64_t per4 = numel(y) / 4 / NI;
                    const unsigned bpi = (unsigned)std::max<int64_t>(1, std::min<int64_t>(per4 / 1024, 16));      // workgroups per image
                    hipLaunchKernelGGL(fu_absmax_kernel, dim3(bpi, (unsigned)NI), dim3(256), 0, st, y->g, per4, own_amax);
                }
                conv_ws_launch(pk, true, y->g, x->g, x->H, beta_of(x), own_amax);
            }
            else conv_launch(pk, true, y->g, x->g, x->H, beta_of(x), false);
        });
        return y;
    }
    // Block (:182-198) without scale/shift: SiLU(GroupNorm(WSConv3x3(x))) [+ res]
    // next3x3: the name of the ONE convolution that consumes the result, when that is all that reads it (a ResnetBlock's first block):
    // if both convolutions run on conv2d_ws_kernel with whole-image tiles the activation is not written -- the consumer normalises
    // the producer's raw output while staging it (the diffusion U-Net's GroupNorm-on-load mode; option gn_on_load)
    FT* block(FT* x, const std::string& p, FT* res, const std::string& next3x3 = std::string()) {
        const FuPacked& cpk = h->conv.at(p + ".proj");
        const bool fused_stats = gn_fused(cpk, x->H);
        const int P = (x->H / V2Y) * (x->H / V2X) * WS_SPT;     // partials per (image, group): one per tile and memory wave
        float* part = fused_stats ? alloc((size_t)NI * 8 * P * 2) : nullptr;
        FT* c = conv(x, p + ".proj", part, true);
        unsigned* amax = reinterpret_cast<unsigned*>(alloc((size_t)NI));
        unsigned* pmax = nullptr;                                  // per-workgroup maxima of the GroupNorm backward's output
        const int64_t nwg = (NI * (int64_t)x->H * x->H * cpk.Cout / 4 + 255) / 256;       // workgroups of fu_gn_silu_bwd_apply_kernel (whole ones per image)
        // the fused derivative: E = HW (C / 32) / 512 float4 per thread and tensor must be 1, 2, 4 or 16 (every level of the paper's shapes)
        const int gE = (int)((int64_t)x->H * x->H * (cpk.Cout / 32) / 512);
        const bool gfused = h->O("gn_bwd_fused") && cpk.Cout % 32 == 0 && 512 % (cpk.Cout / 32) == 0 &&
                            (int64_t)gE * 512 == (int64_t)x->H * x->H * (cpk.Cout / 32) && (gE == 1 || gE == 2 || gE == 4 || gE == 16);
        if (h->bwd_h3 && ws_ok(h->conv.at(p + ".proj"), x->H)) { c->amax = amax; if (want_grad) pmax = reinterpret_cast<unsigned*>(alloc((size_t)std::max<int64_t>(nwg, NI * 8))); }
        float* stats = alloc((size_t)NI * 16);
        float* sums = alloc((size_t)NI * 16);
        // gn_bwd_fused = 2: whole pixel rows per workgroup, the workgroups of an image exchange their partial sums (granules)
        const bool gcluster = gfused && h->O("gn_bwd_fused") >= 2 && want_grad && x->H * x->H >= 16 && !h->O("no_exchange") && !h->nx_force;
        unsigned long long* gxch = gcluster ? reinterpret_cast<unsigned long long*>(alloc((size_t)NI * 512)) : nullptr;      // 16 slabs x 8 groups x 2 sums, 8 bytes each
        const bool defer = !next3x3.empty() && !res && fused_stats && x->H != 8 && P <= WS_MAXP &&
                           h->fwd_h3 && ws_ok(h->conv.at(next3x3), x->H) && h->conv.at(next3x3).KS == 3;
        FT* y;
        if (defer) { ts.emplace_back(); y = &ts.back(); y->C = c->C; y->H = c->H; if (want_grad) y->g = alloc((size_t)NI * c->H * c->H * c->C); }
        else y = ten(c->C, c->H);
        const float* gam = dry ? nullptr : V(p + ".norm.weight"); const float* bet = dry ? nullptr : V(p + ".norm.bias");
        const int HW = c->H * c->H, C = c->C;
        if (defer) { y->gn_src = dry ? reinterpret_cast<const float*>(1) : c->p; y->gn_part = part; y->gn_gamma = gam; y->gn_beta = bet; y->gn_P = P; }
        if (!dry) {
            if (fused_stats) hipLaunchKernelGGL(fu_gn_merge_kernel, dim3((unsigned)NI), dim3(64), 0, st, part, stats, P, (float)(32 * (C / 8)), c->amax, gxch);
            else hipLaunchKernelGGL(fu_gn_stats_kernel, dim3((unsigned)NI), dim3(256), 0, st, c->p, stats, HW, C, c->amax, gxch);
            if (!defer) hipLaunchKernelGGL(fu_gn_silu_kernel, dim3(blocks(numel(c) / 4)), dim3(256), 0, st, c->p, stats, gam, bet, res ? res->p : nullptr, y->p, numel(c) / 4, HW, C);
            chk();
        }
        if (want_grad && !dry) bwd.push_back([=] {
            if (res) pass_grad(y, res);
            if (gcluster) {
                const int stress = h->O("stress");
                const int NS = gE == 16 ? 16 : 8;                 // workgroups per image (the 64 x 64 level: 16, two per CU)
                const dim3 gg((unsigned)NI * NS);
#define FU_GNC(E_, NS_) hipLaunchKernelGGL((fu_gn_silu_bwd_cluster_kernel<E_, NS_>), gg, dim3(512), 0, st, c->p, y->g, stats, gam, bet, c->g, beta_of(c), HW, C, pmax, gxch, stress, h->err_dev, h->O("dbg"))
                if (gE == 16) FU_GNC(8, 16); else if (gE == 4) FU_GNC(4, 8); else if (gE == 2) FU_GNC(2, 8); else FU_GNC(1, 8);
#undef FU_GNC
                if (pmax) hipLaunchKernelGGL(fu_amax_reduce_kernel, dim3((unsigned)NI), dim3(256), 0, st, pmax, c->amax, NS);
            } else if (gfused) {
                const dim3 gg((unsigned)NI * 8);
#define FU_GNB(E_) hipLaunchKernelGGL(fu_gn_silu_bwd_fused_kernel<E_>, gg, dim3(512), 0, st, c->p, y->g, stats, gam, bet, c->g, beta_of(c), HW, C, (int)NI, pmax)
                if (gE == 16) FU_GNB(16); else if (gE == 4) FU_GNB(4); else if (gE == 2) FU_GNB(2); else FU_GNB(1);
#undef FU_GNB
                if (pmax) hipLaunchKernelGGL(fu_amax_reduce_kernel, dim3((unsigned)NI), dim3(256), 0, st, pmax, c->amax, 8);
            } else {
            hipLaunchKernelGGL(fu_gn_silu_bwd_reduce_kernel, dim3((unsigned)NI), dim3(256), 0, st, c->p, y->g, stats, gam, bet, sums, HW, C);
            hipLaunchKernelGGL(fu_gn_silu_bwd_apply_kernel, dim3(blocks(numel(c) / 4)), dim3(256), 0, st, c->p, y->g, stats, sums, gam, bet, c->g, beta_of(c), numel(c) / 4, HW, C, pmax);
            if (pmax) hipLaunchKernelGGL(fu_amax_reduce_kernel, dim3((unsigned)NI), dim3(256), 0, st, pmax, c->amax, (int)(nwg / NI));
            }
            chk();
        });
        return y;
    }
    FT* resblock(FT* x, const std::string& p) { FT* h1 = block(x, p + ".block1", nullptr, p + ".block2.proj"); return block(h1, p + ".block2", x); }
    static unsigned ln_blocks(int64_t rows, int C) { const int64_t rpb = 4 * (64 / std::min(64, C / 4)); return (unsigned)((rows + rpb - 1) / rpb); }   // rows per wave: 64 / LPR
    FT* layernorm(FT* x, const std::string& gkey, FT* res) {
        FT* y = ten(x->C, x->H);
        const float* g = dry ? nullptr : V(gkey);
        const int64_t rows = NI * (int64_t)x->H * x->H;
        if (!dry) { hipLaunchKernelGGL(fu_ln_kernel, dim3(ln_blocks(rows, x->C)), dim3(256), 0, st, x->p, g, res ? res->p : nullptr, y->p, rows, x->C); chk(); }
        if (want_grad && !dry) bwd.push_back([=] {
            if (res) pass_grad(y, res);
            hipLaunchKernelGGL(fu_ln_bwd_kernel, dim3(ln_blocks(rows, x->C)), dim3(256), 0, st, x->p, g, y->g, x->g, beta_of(x), rows, x->C);
            chk();
        });
        return y;
    }
    // Residual(PreNorm(LinearAttention)) :226-254
    // the site without q | k | v tensors (forceunet_la.h): forward = la2d_context / merge / la2d_apply_out, backward = pass A,
    // dctx merge, pass B
    FT* linattn_fused(FT* x, const std::string& p) {
        const int C = x->C, HW = x->H * x->H;
        FT* out = ten(C, x->H);
        const int nsl = HW / la2_px(C), nsplit = nsl < 4 ? nsl : 4, spw = nsl / nsplit;
        const int ntl = HW / 64, wpi = ntl < 4 ? ntl : 4;
        float* part = alloc((size_t)NI * 4 * nsplit * LA2_REC);
        float* ctx = alloc((size_t)NI * 4096);
        float* kst = alloc((size_t)NI * 256);
        float *dpart = nullptr, *dctx = nullptr, *Tt = nullptr, *dyq = nullptr;
        if (want_grad) { dpart = alloc((size_t)NI * wpi * 4096); dctx = alloc((size_t)NI * 4096); Tt = alloc((size_t)NI * 128); dyq = alloc((size_t)NI * HW * C); }
        if (dry) return out;
        const std::string ap = p + ".fn.fn";
        La2dArgs l;
        std::memset(&l, 0, sizeof(l));
        l.x = x->p; l.ldx = C; l.out = out->p; l.ldo = C;
        l.g = V(p + ".fn.norm.g"); l.g2 = V(ap + ".to_out.1.g");
        l.Wqkv = V(ap + "#la.qkv"); l.Wo = V(ap + "#la.out"); l.bo = h->blob + h->conv.at(ap + ".to_out.0").bias;
        // the forward apply kernel at C = 64 fits three workgroups per CU: more, shorter workgroups (as in unet2d_host.inc, la_wpi)
        int wpi_f = wpi;
        if (C == 64) { wpi_f = 32; while (wpi_f > 1 && (wpi_f > ntl || ntl % wpi_f)) wpi_f >>= 1; }
        l.part = part; l.ctx = ctx; l.HW = HW; l.nsplit = nsplit; l.spw = spw; l.tpw = ntl / wpi_f;
        if (C == 64) hipLaunchKernelGGL(la2d_context_kernel<64>, dim3((unsigned)NI * nsplit), dim3(256), 0, st, l);
        else hipLaunchKernelGGL(la2d_context_kernel<128>, dim3((unsigned)NI * nsplit), dim3(256), 0, st, l);
        hipLaunchKernelGGL(fu_la_merge_kernel, dim3((unsigned)NI * 4), dim3(256), 0, st, part, ctx, kst, nsplit, HW);
        if (C == 64) hipLaunchKernelGGL(la2d_apply_out_kernel<64>, dim3((unsigned)NI * wpi_f), dim3(256), 0, st, l);
        else hipLaunchKernelGGL(la2d_apply_out_kernel<128>, dim3((unsigned)NI * wpi), dim3(256), 0, st, l);
        chk();
        if (want_grad) bwd.push_back([=] {
            FuLaArgs b;
            std::memset(&b, 0, sizeof(b));
            b.x = x->p; b.ldx = C; b.dout = out->g; b.g1 = l.g; b.g2 = l.g2; b.Wqkv = l.Wqkv; b.Wo = l.Wo; b.bo = l.bo;
            b.WoT = V(ap + "#la.WoT"); b.WqT = V(ap + "#la.WqT"); b.WkvT = V(ap + "#la.WkvT");
            b.ctx = ctx; b.kst = kst; b.dctx_part = dpart; b.dctx = dctx; b.T = Tt; b.dyq = dyq;
            b.dx = x->g; b.beta = beta_of(x); b.HW = HW; b.inv_n = 1.0f / (float)HW;
            // backward tiles: 64 pixels at C = 64, 32 at C = 128.  (Round 5 also compiled 32-pixel tiles at C = 64 for TWO workgroups per CU:
            // 256 registers with 47 / 51 spilled, 32.25 -> 32.6 ms per gradient call -- removed in round 6.)
            b.tpw = HW / ((C == 64 ? 64 : 32) * wpi);
            const dim3 grid((unsigned)NI * wpi);
            if (C == 64) hipLaunchKernelGGL((fu_la_bwd_a_kernel<64, 64>), grid, dim3(256), 0, st, b);
            else hipLaunchKernelGGL((fu_la_bwd_a_kernel<128, 32>), grid, dim3(256), 0, st, b);
            hipLaunchKernelGGL(fu_la_dctx_merge_kernel, dim3((unsigned)NI * 4), dim3(256), 0, st, dpart, ctx, dctx, Tt, wpi);
            if (C == 64) hipLaunchKernelGGL((fu_la_bwd_b_kernel<64, 64>), grid, dim3(256), 0, st, b);
            else hipLaunchKernelGGL((fu_la_bwd_b_kernel<128, 32>), grid, dim3(256), 0, st, b);
            chk();
        });
        return out;
    }
    FT* linattn(FT* x, const std::string& p) {
        if (h->O("la_fused") && (x->C == 64 || x->C == 128) && (x->H * x->H) % 256 == 0 && h->vec.count(p + ".fn.fn#la.qkv"))
            return linattn_fused(x, p);
        FT* y = layernorm(x, p + ".fn.norm.g", nullptr);
        FT* qkv = conv(y, p + ".fn.fn.to_qkv");
        const int n = x->H * x->H;
        const size_t big = (size_t)NI * n * 128;
        float* kstat = alloc((size_t)NI * 256);
        float* ctx = alloc((size_t)NI * 4096);
        float* qs = alloc(big); float* ks = alloc(big);
        float *dctx = nullptr, *Tt = nullptr;
        if (want_grad) { dctx = alloc((size_t)NI * 4096); Tt = alloc((size_t)NI * 128); }
        FT* la = ten(128, x->H);
        const int nblk = std::min(8, n / 16);                   // 16-pixel blocks per rowmat workgroup (n is a multiple of 64)
        const dim3 gh(4, (unsigned)NI), gp((unsigned)(n / (16 * nblk)), (unsigned)NI);
        const int64_t nph = NI * (int64_t)n * 32;            // float4 lanes of the [pixels][128] tensors
        const float inv_n = 1.0f / (float)n;
        if (!dry) {
            hipLaunchKernelGGL(fu_la_kstat_kernel, dim3((unsigned)NI), dim3(256), 0, st, qkv->p, kstat, n);
            hipLaunchKernelGGL(fu_la_prep_kernel, dim3(blocks(nph)), dim3(256), 0, st, qkv->p, kstat, qs, ks, n, nph);
            hipLaunchKernelGGL(fu_la_outer_kernel, gh, dim3(256), 0, st, ks, 128, 0, qkv->p, 384, 256, ctx, inv_n, n);          // ctx = ks^T v / n
            hipLaunchKernelGGL(fu_la_rowmat_kernel, gp, dim3(256), 0, st, qs, 128, 0, ctx, la->p, 128, 0, 1.0f, n, nblk);     // out = qs ctx
            chk();
        }
        if (want_grad && !dry) bwd.push_back([=] {
            hipLaunchKernelGGL(fu_la_outer_kernel, gh, dim3(256), 0, st, qs, 128, 0, la->g, 128, 0, dctx, 1.0f, n);            // dctx = qs^T dout
            hipLaunchKernelGGL(fu_la_tdot_kernel, dim3((unsigned)NI), dim3(128), 0, st, ctx, dctx, Tt);                          // T = sum_n ks dks
            hipLaunchKernelGGL(fu_la_bwd_fused_kernel, gp, dim3(256), 0, st, qs, ks, qkv->p, la->g, ctx, dctx, Tt, qkv->g, inv_n, n, nblk);
            qkv->gset = true;
            chk();
        });
        FT* pr = conv(la, p + ".fn.fn.to_out.0");
        return layernorm(pr, p + ".fn.fn.to_out.1.g", x);
    }
    // Residual(PreNorm(Attention)) :256-278: n = H * H = 64 tokens on the MFMA kernels (the reference's shape), 256 / 1024 tokens
    // (a 16 x 16 / 32 x 32 coarsest level) on the streaming fp32 kernels
    FT* attn(FT* x, const std::string& p) {
        FT* y = layernorm(x, p + ".fn.norm.g", nullptr);
        FT* qkv = conv(y, p + ".fn.fn.to_qkv");
        const int n = x->H * x->H;
        FT* ao = ten(128, x->H);
        float* ast = n > 64 ? alloc((size_t)NI * 4 * n * 3) : nullptr;      // row maximum, row sum, dout . out
        const dim3 gg(4, (unsigned)NI, (unsigned)(n / 64));
        if (!dry) {
            if (n == 64) hipLaunchKernelGGL(fu_attn64_kernel, dim3(4, (unsigned)NI), dim3(256), 0, st, qkv->p, ao->p);
            else if (n > 64) hipLaunchKernelGGL(fu_attn_gen_kernel, gg, dim3(64), 0, st, qkv->p, ao->p, ast, n);
            else hipLaunchKernelGGL(fu_attn_kernel, dim3(4, (unsigned)NI), dim3(64), 0, st, qkv->p, ao->p, n);
            chk();
        }
        if (want_grad && !dry) bwd.push_back([=] {
            if (n == 64) hipLaunchKernelGGL(fu_attn64_bwd_kernel, dim3(4, (unsigned)NI), dim3(256), 0, st, qkv->p, ao->g, qkv->g);
            else if (n > 64) {
                hipLaunchKernelGGL(fu_attn_gen_bwd_q_kernel, gg, dim3(64), 0, st, qkv->p, ao->p, ao->g, ast, qkv->g, n);
                hipLaunchKernelGGL(fu_attn_gen_bwd_kv_kernel, gg, dim3(64), 0, st, qkv->p, ao->g, ast, qkv->g, n);
            }
            else hipLaunchKernelGGL(fu_attn_bwd_kernel, dim3(4, (unsigned)NI), dim3(64), 0, st, qkv->p, ao->g, qkv->g, n);
            qkv->gset = true;
            chk();
        });
        FT* pr = conv(ao, p + ".fn.fn.to_out");
        // + x: plain residual add
        FT* z = ten(x->C, x->H);
        if (!dry) {
            hipLaunchKernelGGL(fu_add_kernel, dim3(blocks(numel(z))), dim3(256), 0, st, pr->p, z->p, 0.f, numel(z));
            hipLaunchKernelGGL(fu_add_kernel, dim3(blocks(numel(z))), dim3(256), 0, st, x->p, z->p, 1.f, numel(z));
            chk();
        }
        if (want_grad && !dry) bwd.push_back([=] {
            pass_grad(z, pr);                                // read only (to_out's input gradient) before anything adds to x.g
            pass_grad(z, x);
            chk();
        });
        return z;
    }
    // Downsample (:92-97): pixel-unshuffle + 1x1, as ONE convolution that reads the full-resolution tensor through the
    // rearrangement (and scatters its input gradient back through it)
    FT* conv_unshuffled(FT* x, const std::string& name) {
        const FuPacked& pk = h->conv.at(name);
        FT* y = ten(pk.Cout, x->H / 2);
        if (!dry) conv_launch(pk, false, x->p, y->p, x->H / 2, 0.f, true, x->C);
        if (want_grad && !dry) bwd.push_back([this, x, y, &pk] { conv_launch(pk, true, y->g, x->g, x->H / 2, beta_of(x), false, x->C); });
        return y;
    }
};

// forward (and, when dinp is given, the gradient of sum_img lambda |out0| + out1 with respect to the input)
static int fu_network(cindm_forceunet* h, const float* inp, float* out, float* dinp, float lambda_force, int64_t NI,
                      void* ws, size_t ws_bytes, hipStream_t st, bool dry, size_t* need, const float* dout = nullptr, bool serve_taps = false) {
    FuRun R{h, st, (char*)ws, 0, dry, NI, dinp != nullptr};
    // serve_taps: the three entries whose workspace the caller holds (not the design gradient, which lays out its own)
    R.taps = serve_taps && !dry && h->O("taps") != 0;
    if (serve_taps && !dry && !h->taps.empty()) { h->taps.clear(); h->taps_imgs = 0; }
    std::vector<std::pair<std::string, FT*>> named;      // block outputs under the reference's module names
    const std::string top;
    auto tap = [&](const std::string& p, const char* name, FT* t) { if (R.taps) named.emplace_back(p + name, t); return t; };
    const int n = h->d.n_mults, S = h->d.image_size;
    FT xin; xin.p = const_cast<float*>(inp); xin.g = dinp; xin.C = h->d.channels; xin.H = S;
    FT* x = tap(top, "init_conv", R.conv(&xin, "init_conv"));
    for (int ind = 0; ind < n; ++ind) {
        const std::string p = "downs." + std::to_string(ind);
        x = tap(p, ".0", R.resblock(x, p + ".0"));
        x = tap(p, ".1", R.resblock(x, p + ".1"));
        x = tap(p, ".2", R.linattn(x, p + ".2"));
        x = tap(p, ".3", ind < n - 1 ? R.conv_unshuffled(x, p + ".3.1") : R.conv(x, p + ".3"));
    }
    x = tap(top, "mid_block1", R.resblock(x, "mid_block1"));
    x = tap(top, "mid_attn", R.attn(x, "mid_attn"));
    x = tap(top, "mid_block2", R.resblock(x, "mid_block2"));
    if (need) *need = R.off + 256;
    if (dry) return 0;
    REQUIRE(R.off + 256 <= ws_bytes, "workspace too small");
    const int HW = x->H * x->H;
    hipLaunchKernelGGL(fu_head_kernel, dim3((unsigned)NI), dim3(256), 0, st, x->p, R.V("final.weight"), R.V("final.bias"), out, HW, x->C);
    if (dinp) {
        hipLaunchKernelGGL(fu_head_bwd_kernel, dim3(FuRun::blocks(R.numel(x))), dim3(256), 0, st, out, R.V("final.weight"), lambda_force, x->g, HW, x->C, R.numel(x), dout);
        x->gset = true;
        for (auto it = R.bwd.rbegin(); it != R.bwd.rend(); ++it) (*it)();
    }
    R.chk();
    if (R.err != hipSuccess) return fail(std::string("ForceUnet launch: ") + hipGetErrorString(R.err));
    if (R.taps) {
        // taken after the backward has been issued: pass_grad redirects ->g while it runs (without taps; with them every tensor keeps
        // the buffer ten() gave it)
        for (const auto& nt : named) {
            const FT* t = nt.second;
            h->taps[nt.first] = {(size_t)(reinterpret_cast<char*>(t->p) - R.ws), t->g ? (size_t)(reinterpret_cast<char*>(t->g) - R.ws) : (size_t)0, t->C, t->H};
        }
        h->taps_imgs = NI; h->taps_grad = dinp != nullptr;
    }
    return 0;
}

extern "C" size_t cindm_forceunet_workspace_bytes(const cindm_forceunet* h, int64_t images, int32_t with_grad) {
    if (!h || !h->finalized || images <= 0) return 0;
    size_t need = 0;
    float dummy = 0.f;
    fu_network(const_cast<cindm_forceunet*>(h), nullptr, nullptr, with_grad ? &dummy : nullptr, 0.f, images, nullptr, 0, nullptr, true, &need);
    return need;
}

extern "C" int cindm_forceunet_forward(cindm_forceunet* h, const float* x, float* out, int64_t images, void* ws, size_t ws_bytes, void* stream) {
    REQUIRE(h && x && out && ws, "null argument");
    REQUIRE(h->finalized, "cindm_forceunet_finalize has not been called");
    return fu_network(h, x, out, nullptr, 0.f, images, ws, ws_bytes, (hipStream_t)stream, false, nullptr, nullptr, true);
}

extern "C" int cindm_forceunet_grad(cindm_forceunet* h, const float* x, float lambda_force, float* out, float* dx, int64_t images,
                                    void* ws, size_t ws_bytes, void* stream) {
    REQUIRE(h && x && out && dx && ws, "null argument");
    REQUIRE(h->finalized, "cindm_forceunet_finalize has not been called");
    return fu_network(h, x, out, dx, lambda_force, images, ws, ws_bytes, (hipStream_t)stream, false, nullptr, nullptr, true);
}

// vector-Jacobian product: dx = d( sum_img dout[img] . out[img] ) / dx for a caller-given dout [images, 2] -- the backward of
// ForceUnet.forward under torch.autograd, so the reference's own force_fn (autograd.grad of any function of the model's
// output, inference/inverse_design_2d.py:113-117) runs on this model unchanged
extern "C" int cindm_forceunet_vjp(cindm_forceunet* h, const float* x, const float* dout, float* out, float* dx, int64_t images,
                                   void* ws, size_t ws_bytes, void* stream) {
    REQUIRE(h && x && dout && out && dx && ws, "null argument");
    REQUIRE(h->finalized, "cindm_forceunet_finalize has not been called");
    return fu_network(h, x, out, dx, 0.f, images, ws, ws_bytes, (hipStream_t)stream, false, nullptr, dout, true);
}

// Test hook (include/cindm_hip.h): a block output of the last forward / grad / vjp call run with option "taps" = 1, or the gradient
// of that call's objective with respect to it, copied out of the caller's workspace.
extern "C" int cindm_forceunet_tap(cindm_forceunet* h, const char* name, int32_t grad, int64_t images, void* ws, float* dst,
                                   int64_t dst_cap, int64_t shape[3], void* stream) {
    REQUIRE(h && name && ws && shape, "null argument");
    auto it = h->taps.find(name);
    if (it == h->taps.end()) return fail(std::string("unknown tap: ") + name);
    REQUIRE(images == h->taps_imgs, "tap: image count differs from the last call");
    REQUIRE(!grad || h->taps_grad, "tap: the last call was forward-only, no gradient was computed");
    const cindm_forceunet::Tap& t = it->second;
    const int64_t n = images * (int64_t)t.H * t.H * t.C;
    shape[0] = images; shape[1] = (int64_t)t.H * t.H; shape[2] = t.C;
    if (!dst) return 0;
    REQUIRE(n <= dst_cap, "tap: destination too small");
    HIPCHK(hipMemcpyAsync(dst, (char*)ws + (grad ? t.off_g : t.off_p), n * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return 0;
}

// design_fn of inference/inverse_design_2d.py:208-214: grad =d force / dx + lambda_overlap * d overlap / dx, on the
// sampler's device layout [B * nb][pixel][CP] (CP = padded channels, Cs = 3 * frames + 3 real ones)
// fpp = frames per network pass: the surrogate sees fpp * B * nb images at once (the deep levels of one frame's 128 images
// leave most of the GPU idle; 768 images fill it)
static size_t fu_design_layout(const cindm_forceunet* h, int64_t B, int nb, int fpp, size_t& o_bsum, size_t& o_inp, size_t& o_dinp,
                               size_t& o_gb, size_t& o_dm, size_t& o_out, size_t& o_net) {
    const int64_t NI = B * nb;
    const size_t HW = (size_t)h->d.image_size * h->d.image_size;
    auto al = [](size_t v) { return (v + 255) / 256 * 256; };
    size_t o = 0;
    o_bsum = o; o += al((size_t)B * HW * 3 * 4);
    o_inp = o; o += al((size_t)NI * fpp * HW * 4 * 4);
    o_dinp = o; o += al((size_t)NI * fpp * HW * 4 * 4);
    o_gb = o; o += al((size_t)NI * HW * 3 * 4);
    o_dm = o; o += al((size_t)NI * HW * 4);
    o_out = o; o += al((size_t)NI * fpp * 2 * 4);
    o_net = o; o += cindm_forceunet_workspace_bytes(h, NI * fpp, 1);
    return o + 256;
}
extern "C" size_t cindm_airfoil_design_workspace_bytes(const cindm_forceunet* h, int64_t B, int32_t nb, int32_t frames_per_pass) {
    if (!h || !h->finalized || B <= 0 || nb <= 0 || frames_per_pass <= 0) return 0;
    size_t a, b, c, d, e, f, g;
    return fu_design_layout(h, B, nb, frames_per_pass, a, b, c, d, e, f, g);
}
extern "C" int cindm_airfoil_design_grad(cindm_forceunet* h, const float* x, int64_t B, int32_t nb, int32_t frames, int32_t CP,
                                         float p_min, float p_max, float lambda_force, float lambda_overlap, int32_t down_factor,
                                         int32_t sum_boundary, float* grad, void* ws, size_t ws_bytes, void* stream) {
    REQUIRE(h && x && grad && ws, "null argument");
    REQUIRE(h->finalized, "cindm_forceunet_finalize has not been called");
    REQUIRE(h->d.channels == 4, "the airfoil objective feeds (pressure, 3 boundary channels): ForceUnet(channels=4)");
    const int S = h->d.image_size, HW = S * S, Cs = 3 * frames + 3;
    REQUIRE(CP >= Cs && frames >= 1 && nb >= 1 && B >= 1, "bad state shape");
    REQUIRE(down_factor >= 1 && S % down_factor == 0, "downsampling_factor must divide the image size");
    // frames per pass: the largest divisor of `frames` whose layout fits the caller's workspace
    size_t o_bsum = 0, o_inp = 0, o_dinp = 0, o_gb = 0, o_dm = 0, o_out = 0, o_net = 0;
    int fpp = 0;
    for (int c = frames; c >= 1; --c) {
        if (frames % c) continue;
        if (fu_design_layout(h, B, nb, c, o_bsum, o_inp, o_dinp, o_gb, o_dm, o_out, o_net) <= ws_bytes) { fpp = c; break; }
    }
    REQUIRE(fpp >= 1, "workspace too small");
    REQUIRE(((uintptr_t)ws & 255) == 0, "workspace must be 256-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    char* w = (char*)ws;
    const int64_t NI = B * nb, npix = NI * HW;
    REQUIRE(NI * fpp * (int64_t)(S / 8) * (S / 8) <= 65535, "too many images per pass (grid.y limit): pass a smaller workspace");
    float* bsum = (float*)(w + o_bsum); float* inp = (float*)(w + o_inp); float* dinp = (float*)(w + o_dinp);
    float* gb = (float*)(w + o_gb); float* dm = (float*)(w + o_dm); float* out = (float*)(w + o_out);
    HIPCHK(hipMemsetAsync(grad, 0, (size_t)npix * CP * sizeof(float), st));
    if (sum_boundary)
        hipLaunchKernelGGL(fu_bsum_kernel, dim3(FuRun::blocks(B * (int64_t)HW * 3)), dim3(256), 0, st, x, bsum, nb, HW, CP, Cs, B * (int64_t)HW * 3);
    const float pscale = sum_boundary ? 0.5f * (p_max - p_min) : 1.0f, gscale = sum_boundary ? 1.0f : (float)nb;
    for (int f0 = 0; f0 < frames; f0 += fpp) {
        for (int j = 0; j < fpp; ++j)
            hipLaunchKernelGGL(fu_build_input_kernel, dim3(FuRun::blocks(npix)), dim3(256), 0, st, x, sum_boundary ? bsum : (const float*)nullptr,
                               inp + (size_t)j * npix * 4, f0 + j, nb, HW, CP, Cs, p_min, p_max, npix);
        if (fu_network(h, inp, out, dinp, lambda_force, NI * fpp, w + o_net, ws_bytes - o_net, st, false, nullptr) != 0) return -1;
        for (int j = 0; j < fpp; ++j)
            hipLaunchKernelGGL(fu_scatter_input_grad_kernel, dim3(FuRun::blocks(npix)), dim3(256), 0, st, dinp + (size_t)j * npix * 4, grad, gb, f0 + j,
                               (f0 + j) == 0 ? 1 : 0, CP, pscale, gscale, npix);
    }
    const int nr = S / down_factor;
    hipLaunchKernelGGL(fu_overlap_dm_kernel, dim3(FuRun::blocks(NI * (int64_t)nr * nr)), dim3(256), 0, st, x, dm, S, down_factor, CP, Cs, NI * (int64_t)nr * nr);
    hipLaunchKernelGGL(fu_finish_grad_kernel, dim3(FuRun::blocks(npix)), dim3(256), 0, st, x, gb, dm, grad, nb, S, down_factor, CP, Cs, lambda_overlap, sum_boundary ? 1 : 0, npix);
    HIPCHK(hipGetLastError());
    return 0;
}

// The guidance shift of the design-guided DDPM chain (ddpm_step2 in ddpm2d_host.inc): x_{t-1} -= eta[t] * g, the third part of its
// captured step.
__global__ void guided_shift2d_kernel(float* __restrict__ x, const float* __restrict__ g, const float* __restrict__ eta,
                                      const int* __restrict__ t_dev, int64_t n4) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n4) return;
    const float e = eta[t_dev[0] + 1];                       // the step before has already decremented the counter
    float4 v = reinterpret_cast<float4*>(x)[i];
    const float4 d = reinterpret_cast<const float4*>(g)[i];
    v.x -= e * d.x; v.y -= e * d.y; v.z -= e * d.z; v.w -= e * d.w;
    reinterpret_cast<float4*>(x)[i] = v;
}
