// Kernels that the code object holds behind every other one.  cindm_hip.hip includes this file last, and a kernel here is a template
// whose first use is here too: the compiler emits plain kernels where they are defined and instantiations in the order of their
// first use, so what is added here leaves the offsets of all existing kernels alone.
#pragma once
#include "kernels.h"

namespace cindm {

// the guided update with the pair-distance objective (dz_mode 6; kMulti: its DDIM update under the multistep solver, which reads and
// writes hist): instantiations of compose_update_body of their own, launched as the quadratic ones are and never fused into
// ups_last_kernel
template <bool kMulti>
__global__ void compose_update_pair_kernel(const ComposeArgs a, float* hist) {
    compose_update_body<kObjPair, kMulti>(a, (int64_t)blockIdx.x * blockDim.x + threadIdx.x, hist);
}

void launch_compose_update_pair(const ComposeArgs& a, float* hist, int64_t n_elements, hipStream_t stream) {
    const dim3 grid((unsigned)((n_elements + 255) / 256));
    if (hist) hipLaunchKernelGGL(compose_update_pair_kernel<true>, grid, dim3(256), 0, stream, a, hist);
    else hipLaunchKernelGGL(compose_update_pair_kernel<false>, grid, dim3(256), 0, stream, a, (float*)nullptr);
}

// the unguided DDIM update under pred_x0 / pred_v with the clamp on (compose_update_body's kClampedEps; kMulti: under the multistep
// solver): the host launches it for that combination only, and never fused
template <bool kMulti>
__global__ void compose_update_clamped_kernel(const ComposeArgs a, float* hist) {
    compose_update_body<kObjPosition, kMulti, true>(a, (int64_t)blockIdx.x * blockDim.x + threadIdx.x, hist);
}

void launch_compose_update_clamped(const ComposeArgs& a, float* hist, int64_t n_elements, hipStream_t stream) {
    const dim3 grid((unsigned)((n_elements + 255) / 256));
    if (hist) hipLaunchKernelGGL(compose_update_clamped_kernel<true>, grid, dim3(256), 0, stream, a, hist);
    else hipLaunchKernelGGL(compose_update_clamped_kernel<false>, grid, dim3(256), 0, stream, a, (float*)nullptr);
}

// the guided update with the sum of the armed table objectives (dz_mode 7; kMulti: its DDIM update under the multistep
// solver): compose_update_body's kObjSum.  The tables' addresses and flags are the second by-value argument; never fused
template <bool kMulti>
__global__ void compose_update_sum_kernel(const ComposeArgs a, const DesignSum s, float* hist) {
    compose_update_body<kObjSum, kMulti>(a, (int64_t)blockIdx.x * blockDim.x + threadIdx.x, hist, &s);
}

void launch_compose_update_sum(const ComposeArgs& a, const DesignSum& sum, float* hist, int64_t n_elements, hipStream_t stream) {
    const dim3 grid((unsigned)((n_elements + 255) / 256));
    if (hist) hipLaunchKernelGGL(compose_update_sum_kernel<true>, grid, dim3(256), 0, stream, a, sum, hist);
    else hipLaunchKernelGGL(compose_update_sum_kernel<false>, grid, dim3(256), 0, stream, a, sum, (float*)nullptr);
}

}  // namespace cindm
