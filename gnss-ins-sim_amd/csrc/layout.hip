// Layout helpers of the host-buffer boundary (moved verbatim from mc_kernel.hip and mc_kernel_f32.hip: the ISA of their kernels
// is unchanged).
#include <hip/hip_runtime.h>
#include "ginsim.h"
#include "launch.hpp"

namespace ginsim {

// ---------------------------------------------------------------------------------------------------
// Layout helpers for the host-buffer boundary: [R][n][C] (reference per-run arrays) <-> [C][n][R].
__global__ void aos_to_soa_kernel(const double* __restrict__ src, double* __restrict__ dst, int64_t R, int64_t n, int C) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;   // over n*R, run fastest
    if (idx >= n * R) return;
    const int64_t r = idx % R, j = idx / R;
    for (int c = 0; c < C; ++c) dst[(c * n + j) * R + r] = src[(r * n + j) * C + c];
}

// gather selected runs: series [C][n][runs] -> out [nsel][n][C]
__global__ void gather_runs_kernel(const double* __restrict__ series, int C, int64_t n, int64_t runs,
                                   const int64_t* __restrict__ ids, int nsel, double* __restrict__ out) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;   // over nsel*n*C, component fastest
    const int64_t total = (int64_t)nsel * n * C;
    if (idx >= total) return;
    const int c = (int)(idx % C);
    const int64_t j = (idx / C) % n;
    const int64_t k = idx / (C * n);
    out[idx] = series[((int64_t)c * n + j) * runs + ids[k]];
}

// the same from a series-major buffer [runs][C][n] (sensor_layout 1): out [nsel][n][C]
__global__ void gather_series_kernel(const double* __restrict__ series, int C, int64_t n, const int64_t* __restrict__ ids, int nsel,
                                     double* __restrict__ out) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;   // over nsel*C*n, sample fastest (the reads coalesce)
    const int64_t total = (int64_t)nsel * n * C;
    if (idx >= total) return;
    const int64_t j = idx % n;
    const int c = (int)((idx / n) % C);
    const int64_t k = idx / (n * C);
    out[(k * n + j) * C + c] = series[(ids[k] * C + c) * n + j];
}

hipError_t launch_gather_series(const double* series, int C, int64_t n, const int64_t* ids, int nsel, double* out, hipStream_t s) {
    const int tb = 256;
    const int64_t total = (int64_t)nsel * n * C;
    hipLaunchKernelGGL(gather_series_kernel, dim3((unsigned)((total + tb - 1) / tb)), dim3(tb), 0, s, series, C, n, ids, nsel, out);
    return hipGetLastError();
}

// [C][n][R] -> [R][C][n]: per component a (n x R) -> (R x n) transpose through a padded LDS tile of 64 samples x up to 64 runs.
// The tile's source rows are read as ONE flat range when the tile spans whole rows (R <= 64: 64 x R contiguous doubles, every
// lane busy whatever R is -- with a lane per run, 32 runs left half of every wavefront idle and the re-layout of config 5's
// 2 x 1.1 GB ran at 2.6 TB/s; now 4.6); the writes are 512-byte rows of 64 samples, one per run of the tile.  (Tiles of 128
// samples for few runs -- 1 KiB rows on the write side -- measured no faster.)
__global__ void __launch_bounds__(256) runs_to_series_kernel(const double* __restrict__ in, double* __restrict__ out, int C,
                                                            int64_t n, int64_t R) {
    __shared__ double tile[64][65];
    const int c = blockIdx.z;
    const int64_t j0 = (int64_t)blockIdx.x * 64, r0 = (int64_t)blockIdx.y * 64;
    const int rt = (int)(R - r0 < 64 ? R - r0 : 64);            // runs in this tile
    const int jt = (int)(n - j0 < 64 ? n - j0 : 64);            // samples in this tile
    const double* src = in + (int64_t)c * n * R + j0 * R + r0;
    const bool pow2 = (rt & (rt - 1)) == 0;
    const int sh = 31 - __builtin_clz(rt);
    for (int e = threadIdx.x; e < jt * rt; e += 256) {
        const int j = pow2 ? (e >> sh) : e / rt;
        const int r = e - j * rt;
        tile[j][r] = __builtin_nontemporal_load(&src[(int64_t)j * R + r]);
    }
    __syncthreads();
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    if (tx < jt)
        for (int k = ty; k < rt; k += 4) __builtin_nontemporal_store(tile[tx][k], &out[((r0 + k) * C + c) * n + j0 + tx]);
}

hipError_t launch_runs_to_series(const double* in, double* out, int C, int64_t n, int64_t R, hipStream_t s) {
    hipLaunchKernelGGL(runs_to_series_kernel, dim3((unsigned)((n + 63) / 64), (unsigned)((R + 63) / 64), (unsigned)C), dim3(256), 0, s,
                       in, out, C, n, R);
    return hipGetLastError();
}

hipError_t launch_aos_to_soa(const double* src, double* dst, int64_t R, int64_t n, int C, hipStream_t s) {
    const int tb = 256;
    hipLaunchKernelGGL(aos_to_soa_kernel, dim3((unsigned)((n * R + tb - 1) / tb)), dim3(tb), 0, s, src, dst, R, n, C);
    return hipGetLastError();
}

hipError_t launch_gather_runs(const double* series, int C, int64_t n, int64_t runs, const int64_t* ids, int nsel,
                              double* out, hipStream_t s) {
    const int tb = 256;
    const int64_t total = (int64_t)nsel * n * C;
    hipLaunchKernelGGL(gather_runs_kernel, dim3((unsigned)((total + tb - 1) / tb)), dim3(tb), 0, s, series, C, n, runs,
                       ids, nsel, out);
    return hipGetLastError();
}

// gather selected runs of a float series: [C][n][runs] (float) -> out [nsel][n][C] (double), optional per-component origin
__global__ void gather_runs_f32_kernel(const float* __restrict__ series, int C, int64_t n, int64_t runs,
                                       const int64_t* __restrict__ ids, int nsel, double* __restrict__ out) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t total = (int64_t)nsel * n * C;
    if (idx >= total) return;
    const int c = (int)(idx % C);
    const int64_t j = (idx / C) % n;
    const int64_t k = idx / (C * n);
    out[idx] = (double)series[((int64_t)c * n + j) * runs + ids[k]];
}

hipError_t launch_gather_runs_f32(const float* series, int C, int64_t n, int64_t runs, const int64_t* ids, int nsel,
                                  double* out, hipStream_t s) {
    const int tb = 256;
    const int64_t total = (int64_t)nsel * n * C;
    hipLaunchKernelGGL(gather_runs_f32_kernel, dim3((unsigned)((total + tb - 1) / tb)), dim3(tb), 0, s, series, C, n, runs,
                       ids, nsel, out);
    return hipGetLastError();
}

}  // namespace ginsim
