// The guided 2-D DDIM update as one launch (ddim2d_guided_update_kernel) against the two launches it replaces -- ddim2d_update_kernel
// followed by a second pass x -= w g over the state, the form the guided DDPM chain uses (guided_shift2d_kernel) -- at the shape of
// the guided airfoil workload: 64 designs x 2 boundaries, 64 x 64 pixels, 21 channels padded to 24 (50.3 MB per buffer).
//
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off tools/micro/ddim2d_guided_update.hip -o ddim2d_guided_update
//   ./ddim2d_guided_update [designs=64] [boundaries=2] [rounds=5] [launches per round=30]
//
// Both forms start every timed launch from the same state with the caches flushed (a 512 MiB fill precedes it, outside the timed
// window: in the chain the surrogate and the U-Net run between two updates), are timed with device events around their own kernels
// only, and alternate round by round.  Before timing, one launch of each from the same state is compared bit for bit.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../cindm_amd/csrc/kernels2d.h"
using namespace cindm;

#define CK(e) do { hipError_t e_ = (e); if (e_ != hipSuccess) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, hipGetErrorString(e_)); return 2; } } while (0)

// the second pass of the two-launch form: guided_shift2d_kernel with the weight taken from the step's table row
__global__ void shift_pass_kernel(float* __restrict__ x, const float* __restrict__ g, const float* __restrict__ tab,
                                  const int* __restrict__ t_dev, int64_t n4) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n4) return;
    const float w = tab[4 * t_dev[2] + 3];
    float4 v = reinterpret_cast<float4*>(x)[i];
    const float4 d = reinterpret_cast<const float4*>(g)[i];
    v.x = __fsub_rn(v.x, __fmul_rn(w, d.x)); v.y = __fsub_rn(v.y, __fmul_rn(w, d.y));
    v.z = __fsub_rn(v.z, __fmul_rn(w, d.z)); v.w = __fsub_rn(v.w, __fmul_rn(w, d.w));
    reinterpret_cast<float4*>(x)[i] = v;
}

int main(int argc, char** argv) {
    const int B = argc > 1 ? std::atoi(argv[1]) : 64, nb = argc > 2 ? std::atoi(argv[2]) : 2;
    const int rounds = argc > 3 ? std::atoi(argv[3]) : 5, per = argc > 4 ? std::atoi(argv[4]) : 30;
    const int HW = 64 * 64, C = 21, CP = 24, T = 1000;
    if (B < 1 || nb < 1 || rounds < 1 || per < 1 || (int64_t)B * nb * HW * CP >= (1ll << 31)) { std::fprintf(stderr, "bad arguments\n"); return 2; }
    const size_t n = (size_t)B * nb * HW * CP;
    std::vector<float> hx(n), he(n), hg(n);
    uint32_t s = 12345u;
    auto rnd = [&]() { s = s * 1664525u + 1013904223u; return ((s >> 8) * (1.0f / 8388608.0f)) - 1.0f; };
    for (size_t i = 0; i < n; ++i) { const bool real = (int)(i % CP) < C; hx[i] = real ? rnd() : 0.f; he[i] = real ? rnd() : 0.f; hg[i] = real ? 10.f * rnd() : 0.f; }
    std::vector<float> sched(4 * (size_t)T);
    for (int t = 0; t < T; ++t) { sched[t] = 1.5f; sched[T + t] = 1.1f; sched[2 * T + t] = 0.7f; sched[3 * T + t] = 0.7f; }
    const float tab_h[4] = {0.9f, 0.4f, 0.1f, 0.003f};       // sqrt(alpha_next), c, sigma (> 0: the generator draws), w
    const int tnext_h[1] = {480}, tdev_h[4] = {500, 0, 0, 0};
    float *x0, *x, *eps, *g, *sch, *tab, *flush; int *tnext, *tdev;
    const size_t flush_bytes = 512ull << 20;
    CK(hipMalloc(&x0, n * 4)); CK(hipMalloc(&x, n * 4)); CK(hipMalloc(&eps, n * 4)); CK(hipMalloc(&g, n * 4));
    CK(hipMalloc(&sch, sched.size() * 4)); CK(hipMalloc(&tab, 16)); CK(hipMalloc(&tnext, 4)); CK(hipMalloc(&tdev, 16)); CK(hipMalloc(&flush, flush_bytes));
    CK(hipMemcpy(x0, hx.data(), n * 4, hipMemcpyHostToDevice)); CK(hipMemcpy(eps, he.data(), n * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(g, hg.data(), n * 4, hipMemcpyHostToDevice)); CK(hipMemcpy(sch, sched.data(), sched.size() * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(tab, tab_h, 16, hipMemcpyHostToDevice)); CK(hipMemcpy(tnext, tnext_h, 4, hipMemcpyHostToDevice)); CK(hipMemcpy(tdev, tdev_h, 16, hipMemcpyHostToDevice));
    Ddim2dArgs a; std::memset(&a, 0, sizeof(a));
    a.x = x; a.eps = eps; a.x_out = x; a.B = B; a.nb = nb; a.HW = HW; a.C = C; a.CP = CP; a.use_avg = 1;
    a.sqrt_recip = sch; a.sqrt_recipm1 = sch + T; a.sqrt_ac = sch + 2 * T; a.sqrt_1mac = sch + 3 * T;
    a.t_dev = tdev; a.tab = tab; a.tnext = tnext; a.seed = 1; a.sample_off = 0;
    const unsigned grid = (unsigned)(((int64_t)B * HW * (CP / 4) + 255) / 256), grid4 = (unsigned)((n / 4 + 255) / 256);
    hipStream_t st; CK(hipStreamCreate(&st));
    auto two = [&]() {
        hipLaunchKernelGGL(ddim2d_update_kernel, dim3(grid), dim3(256), 0, st, a);
        hipLaunchKernelGGL(shift_pass_kernel, dim3(grid4), dim3(256), 0, st, x, (const float*)g, (const float*)tab, (const int*)tdev, (int64_t)(n / 4));
    };
    auto one = [&]() { hipLaunchKernelGGL(ddim2d_guided_update_kernel, dim3(grid), dim3(256), 0, st, a, (const float*)g); };
    // the two forms compute the same state
    std::vector<float> r2(n), r1(n);
    CK(hipMemcpyAsync(x, x0, n * 4, hipMemcpyDeviceToDevice, st)); two(); CK(hipMemcpyAsync(r2.data(), x, n * 4, hipMemcpyDeviceToHost, st));
    CK(hipMemcpyAsync(x, x0, n * 4, hipMemcpyDeviceToDevice, st)); one(); CK(hipMemcpyAsync(r1.data(), x, n * 4, hipMemcpyDeviceToHost, st));
    CK(hipStreamSynchronize(st)); CK(hipGetLastError());
    if (std::memcmp(r1.data(), r2.data(), n * 4) != 0 || std::memcmp(r1.data(), hx.data(), n * 4) == 0) { std::printf("MISMATCH between the two forms\n"); return 1; }
    hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    std::vector<float> t_two, t_one;
    for (int r = 0; r < rounds; ++r)
        for (int form = 0; form < 2; ++form) {
            float sum = 0.f;
            for (int k = 0; k < per; ++k) {
                CK(hipMemcpyAsync(x, x0, n * 4, hipMemcpyDeviceToDevice, st));
                CK(hipMemsetAsync(flush, k, flush_bytes, st));
                CK(hipEventRecord(e0, st));
                if (form == 0) two(); else one();
                CK(hipEventRecord(e1, st));
                CK(hipEventSynchronize(e1));
                float ms = 0.f; CK(hipEventElapsedTime(&ms, e0, e1)); sum += ms;
            }
            (form == 0 ? t_two : t_one).push_back(1e3f * sum / per);
        }
    CK(hipGetLastError());
    auto med = [](std::vector<float> v) { std::sort(v.begin(), v.end()); return v[v.size() / 2]; };
    auto lo = [](const std::vector<float>& v) { return *std::min_element(v.begin(), v.end()); };
    auto hi = [](const std::vector<float>& v) { return *std::max_element(v.begin(), v.end()); };
    std::printf("{\"designs\": %d, \"boundaries\": %d, \"state_MB\": %.1f, \"rounds\": %d, \"launches_per_round\": %d, "
                "\"two_launches_us\": {\"median\": %.2f, \"min\": %.2f, \"max\": %.2f}, \"one_launch_us\": {\"median\": %.2f, \"min\": %.2f, \"max\": %.2f}, "
                "\"bitwise_equal\": true}\n", B, nb, n * 4 / 1e6, rounds, per, med(t_two), lo(t_two), hi(t_two), med(t_one), lo(t_one), hi(t_one));
    return 0;
}
