// Host side of libcindm_hip.so: C ABI declared in include/cindm_hip.h.  This file holds the globals, the error macros and
// the RCCL block; the launch sequence of TemporalUnet1D.forward (model/diffusion_1d.py:610-646 of the reference) is in
// unet1d_host.inc, that of one DDPM reverse step (model/diffusion_1d.py:951-1044, :1047-1186, :1190-1376, :1380-1652) in
// ddpm1d_host.inc, the 2-D path in unet2d_host.inc / forceunet_host.inc / ddpm2d_host.inc, the n-body re-simulation in nbody_host.inc.
// gfx950 only.
#include "kernels.h"
#include "kernels_dconv.h"
#include "kernels2d.h"
#include "kernels2d_v2.h"
#include "nbody.h"
#include "../../include/cindm_hip.h"

#include <hip/hip_ext.h>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

using namespace cindm;

static thread_local std::string g_err;
static int fail(const std::string& m) { g_err = m; return -1; }
#define HIPCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return fail(std::string(#x) + ": " + hipGetErrorString(e_)); } while (0)
#define REQUIRE(c, msg) do { if (!(c)) return fail(msg); } while (0)

extern "C" int cindm_abi_version(void) { return CINDM_ABI_VERSION; }
#ifndef CINDM_SRC_HASH
#define CINDM_SRC_HASH "unknown"
#endif
// the hash behind a marker the build script finds in the file's bytes (cindm_amd/build.py: embedded_hash)
extern "C" const char cindm_source_hash_marker[] = "CINDM_SRC_HASH=" CINDM_SRC_HASH;
extern "C" const char* cindm_source_hash(void) { return cindm_source_hash_marker + 15; }
// In-kernel clocks of conv2d_ws_kernel (kernels2d_v2.h, profiling build only): copies [8 categories][2 roles][8 phases] sums of
// 10 ns ticks to dst and clears them.  Returns 0 in the production build (nothing is recorded there), 1 in the profiling build.
extern "C" int cindm_ws_prof_read(unsigned long long* dst) {
    if (!dst) return fail("null argument");
#ifdef CINDM_PHASE_PROF
    const size_t n = sizeof(unsigned long long) * cindm::WSP_CAT * 2 * cindm::WSP_NPH;
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpyFromSymbol(dst, HIP_SYMBOL(cindm::g_ws_prof), n));
    std::vector<unsigned long long> z(cindm::WSP_CAT * 2 * cindm::WSP_NPH, 0ull);
    HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(cindm::g_ws_prof), z.data(), n));
    return 1;
#else
    std::memset(dst, 0, sizeof(unsigned long long) * cindm::WSP_CAT * 2 * cindm::WSP_NPH);
    return 0;
#endif
}
extern "C" const char* cindm_last_error(void) { return g_err.c_str(); }

static inline int ceil_to(int v, int m) { return (v + m - 1) / m * m; }

// Pack generations are drawn from one process-wide counter: a handle created at a recycled heap address can never
// reproduce the (address, generation) pair of a destroyed one, so a cached step graph that embeds the old handle's
// weight pointers is never replayed for the new one.
#include <atomic>
static std::atomic<int> g_generation{0};

#include "handle_core.inc"

// ============================================================================ TemporalUnet1D
#include "unet1d_host.inc"

// ============================================================================ GaussianDiffusion1D

#include "chain_host.inc"
#include "ddpm1d_host.inc"
#include "timecompose_host.inc"

// ============================================================================ 2-D airfoil path
#include "unet2d_host.inc"
#include "forceunet_host.inc"
#include "ddpm2d_host.inc"

// ============================================================================ n-body re-simulation
#include "nbody_host.inc"

// ---- multi-GPU: the one all-gather of the path, on RCCL (include/cindm_hip.h) -----------------------------------------------
#include <dlfcn.h>
#if __has_include(<rccl/rccl.h>)
#include <rccl/rccl.h>
#else
// A ROCm installation without RCCL's headers still builds the library: the five entry points bound below (resolved with dlopen /
// dlsym at first use -- no link dependency either way), declared as RCCL's public header declares them (NCCL 2 ABI).
extern "C" {
typedef struct ncclComm* ncclComm_t;
typedef struct { char internal[128]; } ncclUniqueId;
typedef enum { ncclSuccess = 0 } ncclResult_t;
typedef enum { ncclFloat = 7 } ncclDataType_t;
ncclResult_t ncclGetUniqueId(ncclUniqueId* uniqueId);
ncclResult_t ncclCommInitRank(ncclComm_t* comm, int nranks, ncclUniqueId commId, int rank);
ncclResult_t ncclAllGather(const void* sendbuff, void* recvbuff, size_t sendcount, ncclDataType_t datatype, ncclComm_t comm, hipStream_t stream);
ncclResult_t ncclCommDestroy(ncclComm_t comm);
const char* ncclGetErrorString(ncclResult_t result);
}
#endif
namespace {
struct RcclApi {
    void* lib = nullptr;
    decltype(&ncclGetUniqueId) GetUniqueId = nullptr;
    decltype(&ncclCommInitRank) CommInitRank = nullptr;
    decltype(&ncclAllGather) AllGather = nullptr;
    decltype(&ncclCommDestroy) CommDestroy = nullptr;
    decltype(&ncclGetErrorString) GetErrorString = nullptr;
    std::string why;
};
// One RCCL per process: the copy that is already mapped (PyTorch-ROCm ships its own librccl.so and torch.distributed's "nccl"
// backend uses it), else the ROCm installation's.
RcclApi& rccl() {
    static RcclApi api = [] {
        RcclApi a;
        for (const char* name : {"librccl.so", "librccl.so.1"}) { a.lib = dlopen(name, RTLD_NOW | RTLD_NOLOAD); if (a.lib) break; }
        for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) { if (a.lib) break; a.lib = dlopen(name, RTLD_NOW | RTLD_GLOBAL); }
        if (!a.lib) { a.why = std::string("librccl.so not found: ") + (dlerror() ? dlerror() : ""); return a; }
        a.GetUniqueId = (decltype(a.GetUniqueId))dlsym(a.lib, "ncclGetUniqueId");
        a.CommInitRank = (decltype(a.CommInitRank))dlsym(a.lib, "ncclCommInitRank");
        a.AllGather = (decltype(a.AllGather))dlsym(a.lib, "ncclAllGather");
        a.CommDestroy = (decltype(a.CommDestroy))dlsym(a.lib, "ncclCommDestroy");
        a.GetErrorString = (decltype(a.GetErrorString))dlsym(a.lib, "ncclGetErrorString");
        if (!a.GetUniqueId || !a.CommInitRank || !a.AllGather || !a.CommDestroy || !a.GetErrorString) a.why = "librccl.so lacks an expected symbol";
        return a;
    }();
    return api;
}
}  // namespace
struct cindm_comm { ncclComm_t comm = nullptr; int world = 0, rank = 0; };
#define RCCLCHK(x) do { ncclResult_t r_ = (x); if (r_ != ncclSuccess) return fail(std::string(#x) + ": " + rccl().GetErrorString(r_)); } while (0)

extern "C" int cindm_comm_unique_id(unsigned char id[128]) {
    REQUIRE(id, "null argument");
    REQUIRE(rccl().why.empty(), rccl().why);
    ncclUniqueId u;
    RCCLCHK(rccl().GetUniqueId(&u));
    static_assert(sizeof(u) == 128, "ncclUniqueId is 128 bytes");
    std::memcpy(id, &u, 128);
    return 0;
}
extern "C" int cindm_comm_init(const unsigned char id[128], int32_t world, int32_t rank, cindm_comm** out) {
    REQUIRE(id && out && world >= 1 && rank >= 0 && rank < world, "bad communicator arguments");
    REQUIRE(rccl().why.empty(), rccl().why);
    ncclUniqueId u;
    std::memcpy(&u, id, 128);
    auto* c = new cindm_comm();
    c->world = world; c->rank = rank;
    ncclResult_t r = rccl().CommInitRank(&c->comm, world, u, rank);
    if (r != ncclSuccess) { delete c; return fail(std::string("ncclCommInitRank: ") + rccl().GetErrorString(r)); }
    *out = c;
    return 0;
}
extern "C" int cindm_comm_world(const cindm_comm* c) { return c ? c->world : 0; }
extern "C" int cindm_all_gather_designs(const float* local, float* out, int64_t per_rank_elems, cindm_comm* c, void* stream) {
    REQUIRE(local && out && c && c->comm && per_rank_elems > 0, "bad all-gather arguments");
    RCCLCHK(rccl().AllGather(local, out, (size_t)per_rank_elems, ncclFloat, c->comm, (hipStream_t)stream));
    return 0;
}
extern "C" void cindm_comm_destroy(cindm_comm* c) {
    if (!c) return;
    if (c->comm && rccl().CommDestroy) (void)rccl().CommDestroy(c->comm);
    delete c;
}

// ============================================================================ kernels defined behind all others
#include "kernels_tail.h"
