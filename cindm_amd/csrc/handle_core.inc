// Host state shared by the three model handles (included by cindm_hip.hip): cindm_unet1d, cindm_unet2d and cindm_forceunet
// derive from ModelCore.  It holds the state-dict manifest with the host copies of the parameters, the sinusoid table of the
// U-Nets, the kernel-path options and whether the packed weights are valid ("finalized").  The *_num_params / *_param_info /
// *_set_param / *_set_sinusoid_table / *_get_option / *_set_option entry points of every handle forward to the functions below.

struct Param {
    std::string name;
    std::vector<int64_t> shape;
    size_t numel = 0;
    std::vector<float> host;
    bool set = false;
};

// What a change of an option does to the handle:
//   OPT_PACK      selects what finalize packs: a change un-finalizes the handle (the next *_finalize repacks)
//   OPT_RUNTIME   selects among kernels whose operands are packed already: the handle stays finalized
//   OPT_READONLY  written by the library only (get_option reads it; set_option refuses it as an unknown option)
enum OptKind { OPT_PACK, OPT_RUNTIME, OPT_READONLY };

// One option of a handle: key, default, the environment variable that overrides the default at create (nullptr: none)
// and its kind.  Each handle's table is the one list of its keys.
struct OptDef { const char* key; int def; const char* env; OptKind kind; };

struct ModelCore {
    std::vector<Param> params;             // state-dict manifest in the reference's registration order
    std::unordered_map<std::string, int> index;
    std::vector<float> sinus;              // [timesteps, dim] (the U-Nets; empty: finalize computes it)
    bool finalized = false;                // the packed weights match params, sinus and every OPT_PACK option
    const OptDef* opt_defs = nullptr; int n_opt_defs = 0;
    std::map<std::string, int> opt;
    int O(const char* k) const { auto it = opt.find(k); return it == opt.end() ? 0 : it->second; }

    template <int N> void init_options(const OptDef (&defs)[N]) {
        opt_defs = defs; n_opt_defs = N;
        for (const auto& o : defs) {
            int v = o.def;
            if (o.env) { const char* e = getenv(o.env); if (e) v = atoi(e); }
            opt[o.key] = v;
        }
        const char* e = getenv("CINDM_MFMA");
        if (e && std::strcmp(e, "f32") == 0 && opt.count("mfma_f32")) opt["mfma_f32"] = 1;
    }
    const OptDef* opt_def(const char* key) const {
        for (int i = 0; i < n_opt_defs; ++i) if (std::strcmp(opt_defs[i].key, key) == 0) return &opt_defs[i];
        return nullptr;
    }
    void add_param(const std::string& n, std::vector<int64_t> s) {
        Param p; p.name = n; p.shape = s; p.numel = 1;
        for (auto v : s) p.numel *= (size_t)v;
        index[n] = (int)params.size();
        params.push_back(std::move(p));
    }
};

static int core_num_params(const ModelCore* h) { return h ? (int)h->params.size() : fail("null handle"); }

static int core_param_info(const ModelCore* h, int idx, char* name, int cap, int64_t shape[4], int* ndim) {
    REQUIRE(h && idx >= 0 && idx < (int)h->params.size(), "bad param index");
    const Param& p = h->params[idx];
    if (name && cap > 0) { std::strncpy(name, p.name.c_str(), cap - 1); name[cap - 1] = 0; }
    for (int i = 0; i < 4; ++i) shape[i] = i < (int)p.shape.size() ? p.shape[i] : 1;
    if (ndim) *ndim = (int)p.shape.size();
    return 0;
}

static int core_set_param(ModelCore* h, const char* key, const float* src, int64_t numel, int on_device) {
    REQUIRE(h && key && src, "null argument");
    auto it = h->index.find(key);
    if (it == h->index.end()) return fail(std::string("unexpected key in state_dict: ") + key);
    Param& p = h->params[it->second];
    if ((int64_t)p.numel != numel) return fail(std::string("size mismatch for ") + key);
    p.host.resize(p.numel);
    if (on_device) HIPCHK(hipMemcpy(p.host.data(), src, p.numel * sizeof(float), hipMemcpyDeviceToHost));
    else std::memcpy(p.host.data(), src, p.numel * sizeof(float));
    p.set = true;
    h->finalized = false;
    return 0;
}

static int core_set_sinusoid(ModelCore* h, const float* t, int64_t numel, int64_t want) {
    REQUIRE(h && t, "null argument");
    REQUIRE(numel == want, "sinusoid table must be [timesteps, dim]");
    h->sinus.assign(t, t + numel);
    h->finalized = false;
    return 0;
}

static int core_get_option(const ModelCore* h, const char* key, int32_t* value) {
    REQUIRE(h && key && value, "null argument");
    auto it = h->opt.find(key);
    if (it == h->opt.end()) return fail(std::string("unknown option: ") + key);
    *value = it->second;
    return 0;
}

// 0 = done (an OPT_PACK change un-finalized the handle), 1 = an OPT_RUNTIME option changed its value, -1 = error
static int core_set_option(ModelCore* h, const char* key, int32_t value) {
    REQUIRE(h && key, "null argument");
    const OptDef* def = h->opt_def(key);
    if (!def || def->kind == OPT_READONLY) return fail(std::string("unknown option: ") + key);
    int& cur = h->opt[key];
    if (cur == value) return 0;
    cur = value;
    if (def->kind == OPT_RUNTIME) return 1;
    h->finalized = false;
    return 0;
}

// The weight window of the range rule of the split-fp16 products (hi = fp16(w), lo = fp16((w - hi) * 2^11)): every element
// of a weight tensor is represented to 2^-24 of the tensor's largest magnitude M as long as 2^-12 <= M <= 2^15 (below, hi
// and lo fall into fp16's subnormals together; above, hi overflows).  An all-zero tensor is inside; nan is outside.
static bool max_abs_in_fp16_window(const std::vector<float>& w) {
    float M = 0.f;
    for (float v : w) M = std::max(M, std::fabs(v));
    return !(M > 32768.0f || (M < 1.0f / 4096.0f && M > 0.f) || !(M == M));
}

// The synthetic calibration batch of the range rule (both U-Nets): `n` elements of a unit-variance bell (sum of four uniforms,
// |v| < 3.5) drawn from `seed`, zero in the padding channels (element i is data when i % CP < C); fwd(t, x, eps, ws) runs one
// forward per timestep in {0, T/2, T-1}.  *finite = false when a forward failed or an eps element is inf / nan.
template <typename Fwd>
static int calibrate_at_finalize(size_t n, int C, int CP, uint32_t seed, int T, size_t wsb, hipStream_t stream, Fwd fwd, bool* finite) {
    std::vector<float> hx(n, 0.f), he(n);
    uint32_t st = seed;
    for (size_t i = 0; i < n; ++i) {
        if ((int)(i % CP) >= C) continue;
        float a = 0.f;
        for (int k = 0; k < 4; ++k) { st = st * 1664525u + 1013904223u; a += (float)(st >> 8) * (1.0f / 16777216.0f) - 0.5f; }
        hx[i] = a * 1.7320508f;
    }
    float *dx = nullptr, *de = nullptr; void* ws = nullptr;
    HIPCHK(hipMalloc((void**)&dx, n * 4)); HIPCHK(hipMalloc((void**)&de, n * 4)); HIPCHK(hipMalloc(&ws, wsb));
    HIPCHK(hipMemcpyAsync(dx, hx.data(), n * 4, hipMemcpyHostToDevice, stream));
    *finite = true;
    for (int t : {0, T / 2, T - 1}) {
        if (fwd(t, dx, de, ws) != 0) { *finite = false; break; }
        HIPCHK(hipMemcpyAsync(he.data(), de, n * 4, hipMemcpyDeviceToHost, stream));
        HIPCHK(hipStreamSynchronize(stream));
        for (float v : he) if (!std::isfinite(v)) { *finite = false; break; }
        if (!*finite) break;
    }
    (void)hipFree(dx); (void)hipFree(de); (void)hipFree(ws);
    return 0;
}
