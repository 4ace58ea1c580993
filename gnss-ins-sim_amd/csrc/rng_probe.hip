// Test hooks of the random-number path (moved verbatim from mc_kernel.hip: the ISA of its kernels is unchanged).
#include <hip/hip_runtime.h>
#include "ginsim.h"
#include "philox.hpp"
#include "launch.hpp"

namespace ginsim {

// ---------------------------------------------------------------------------------------------------
// RNG self-test: normals (and raw Philox words) of one (seed, run, stream), sample index = global lane.
__global__ void rng_probe_kernel(uint64_t seed, uint64_t run, uint32_t stream, int64_t count,
                                 double* __restrict__ z0, double* __restrict__ z1, uint32_t* __restrict__ words) {
    __shared__ uint32_t ntab[kNormalLdsWords];
    const NormalTables tab = fill_normal_tables(ntab, threadIdx.x, blockDim.x);
    __syncthreads();

    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= count) return;
    const RngKey key{(uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)run, (uint32_t)(run >> 32)};
    double a, b;
    normal_pair(key, stream, (uint32_t)j, a, b, tab);
    z0[j] = a;
    z1[j] = b;
    if (words) {
        const u32x4 w = philox4x32((uint32_t)j, stream, key.r0, key.r1, key.k0, key.k1);      // raw block (j, stream)
        words[4 * j + 0] = w.x; words[4 * j + 1] = w.y; words[4 * j + 2] = w.z; words[4 * j + 3] = w.w;
    }
}

hipError_t launch_rng_probe(uint64_t seed, uint64_t run, uint32_t stream, int64_t count, double* z0, double* z1,
                            uint32_t* words, hipStream_t stream_h) {
    const int tb = 256;
    hipLaunchKernelGGL(rng_probe_kernel, dim3((unsigned)((count + tb - 1) / tb)), dim3(tb), 0, stream_h, seed, run,
                       stream, count, z0, z1, words);
    return hipGetLastError();
}

// The normal transform on given words (test hook): words 0-1 are taken as one half block -- z0 from word 0, z1 from
// word 1 (words 2-3 unused).
__global__ void normal_transform_kernel(const uint32_t* __restrict__ words, int64_t count, double* __restrict__ z0, double* __restrict__ z1) {
    __shared__ uint32_t ntab[kNormalLdsWords];
    const NormalTables tab = fill_normal_tables(ntab, threadIdx.x, blockDim.x);
    __syncthreads();

    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const uint32_t ra[1] = {words[4 * i]}, ang[1] = {words[4 * i + 1]};
    float a[1], b[1];
    normal_transform<1>(ra, ang, a, b, tab);
    z0[i] = (double)a[0];
    z1[i] = (double)b[0];
}

hipError_t launch_normal_transform(const uint32_t* words, int64_t count, double* z0, double* z1, hipStream_t s) {
    hipLaunchKernelGGL(normal_transform_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, s, words, count, z0, z1);
    return hipGetLastError();
}

}  // namespace ginsim
