// GPS and magnetometer series (moved verbatim from mc_kernel.hip: the ISA of its kernels is unchanged).
#include <hip/hip_runtime.h>
#include "ginsim.h"
#include "ins_math.hpp"
#include "philox.hpp"
#include "mag_synth.hpp"
#include "gps_synth.hpp"
#include "launch.hpp"

namespace ginsim {

// ---------------------------------------------------------------------------------------------------
// Auxiliary sensors: one thread per (sample, run), run fastest.  gps_gen: pathgen.py:621-624; mag_gen: :658-661.
__global__ void __launch_bounds__(256) aux_gps_kernel(const ginsim_aux_params a) {
    __shared__ uint32_t ntab[kNormalLdsWords];
    const NormalTables tab = fill_normal_tables(ntab, threadIdx.x, blockDim.x);
    __syncthreads();

    MathConsts mk;
    mk.init<false>();
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= a.m * a.runs) return;
    const int64_t r = idx % a.runs, k = idx / a.runs;
    const uint64_t grun = a.run_offset + (uint64_t)r;
    const RngKey key{(uint32_t)a.seed, (uint32_t)(a.seed >> 32), (uint32_t)grun, (uint32_t)(grun >> 32)};
    double fix[6];
    gps_fix(a.ref_gps + 6 * k, a.gps_sigma, key, (uint32_t)k, tab, fix);     // ref + sigma * N  (gps_synth.hpp)
    const int64_t plane = a.m * a.runs;
#pragma unroll
    for (int c = 0; c < 6; ++c) a.out_gps[c * plane + idx] = fix[c];
}

__global__ void __launch_bounds__(256) aux_mag_kernel(const ginsim_aux_params a) {
    __shared__ uint32_t ntab[kNormalLdsWords];
    const NormalTables tab = fill_normal_tables(ntab, threadIdx.x, blockDim.x);
    __syncthreads();

    MathConsts mk;
    mk.init<false>();
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= a.n * a.runs) return;
    const int64_t r = idx % a.runs, j = idx / a.runs;
    const uint64_t grun = a.run_offset + (uint64_t)r;
    const RngKey key{(uint32_t)a.seed, (uint32_t)(a.seed >> 32), (uint32_t)grun, (uint32_t)(grun >> 32)};
    double z[3];
    mag_normals(key, (uint32_t)j, tab, z);
    const double v[3] = {a.ref_mag[3 * j] + a.mag_hi[0], a.ref_mag[3 * j + 1] + a.mag_hi[1], a.ref_mag[3 * j + 2] + a.mag_hi[2]};
    const int64_t plane = a.n * a.runs;
#pragma unroll
    for (int c = 0; c < 3; ++c)     // (ref + hi) . si^T  + std * N  (mag_synth.hpp)
        a.out_mag[c * plane + idx] = mag_axis(a.mag_si + 3 * c, v, a.mag_std[c], z[c]);
}

hipError_t launch_aux(const ginsim_aux_params& p, hipStream_t s) {
    if (p.out_gps && p.ref_gps && p.m > 0)
        hipLaunchKernelGGL(aux_gps_kernel, dim3((unsigned)((p.m * p.runs + 255) / 256)), dim3(256), 0, s, p);
    if (p.out_mag && p.ref_mag && p.n > 0)
        hipLaunchKernelGGL(aux_mag_kernel, dim3((unsigned)((p.n * p.runs + 255) / 256)), dim3(256), 0, s, p);
    return hipGetLastError();
}

}  // namespace ginsim
