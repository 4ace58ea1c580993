// End-point error statistics over Monte-Carlo runs: count, mean, M2 (sum of squared deviations) and
// max|e| for the 9 error components, reduced with wavefront shuffles (Chan/Welford merges).
//
// Restates InsDataMgr.__end_point_error_stats + __array_stats
// (gnss_ins_sim/sim/ins_data_manager.py:717-759, 797-808): {'max': max|e|, 'avg': mean, 'std': std(ddof=0)}.
// (count, mean, M2, max) partials are mergeable, so per-device results combine exactly across GPUs.
#include <hip/hip_runtime.h>
#include "ginsim.h"
#include "fastmath.hpp"
#include "ins_math.hpp"
#include "traj_error.hpp"

namespace ginsim {

constexpr int kStatBlock = 256;

// The end-point reduction runs on x - k, k = the component's first error (0 if that is not finite): a mean and its deviations
// of the size of the spread instead of the size of the offset.  Without it the running means of data at 1e6 +- 1e-6 are
// rounded to ulp(1e6) ~ 1e-10 at every update and merge, and the std came out 1e-5 relative off where np.std is 1e-9.
__device__ __forceinline__ double shift_of(const double* x) {
    const double k = x[0];
    return __builtin_isfinite(k) ? k : 0.0;
}

// grid = (blocks, 9); partial[(comp*blocks + block)] = moments of that block's strided slice
__global__ void __launch_bounds__(kStatBlock) stats_partial_kernel(const double* __restrict__ e, int64_t runs,
                                                                   Mom* __restrict__ partial) {
    const int comp = blockIdx.y;
    const double* x = e + (int64_t)comp * runs;
    const double k = shift_of(x);
    Mom m{0.0, 0.0, 0.0, 0.0};
    for (int64_t r = (int64_t)blockIdx.x * kStatBlock + threadIdx.x; r < runs; r += (int64_t)gridDim.x * kStatBlock) {
        const double v = x[r] - k;
        m.n += 1.0;
        if (__builtin_isfinite(v) && __builtin_isfinite(m.mean)) {
            const double d = v - m.mean;
            m.mean += d / m.n;
            m.m2 += d * (v - m.mean);
        } else {                        // see merge
            m.mean += v;
            m.m2 = __builtin_nan("");
        }
        m.mx = nan_max(fabs(x[r]), m.mx);
    }
#pragma unroll
    for (int mask = 32; mask >= 1; mask >>= 1) m = merge(m, shfl_xor(m, mask));
    __shared__ Mom wave_part[kStatBlock / 64];
    if ((threadIdx.x & 63) == 0) wave_part[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        Mom t = wave_part[0];
        for (int w = 1; w < kStatBlock / 64; ++w) t = merge(t, wave_part[w]);
        partial[comp * gridDim.x + blockIdx.x] = t;
    }
}

// one 64-lane block per component: lanes fold the block partials they own (stride 64, fixed order), then the same
// butterfly of Chan merges as above -- deterministic, and ~10x shorter than one lane walking all partials
__global__ void stats_final_kernel(const Mom* __restrict__ partial, int blocks, const double* __restrict__ e, int64_t runs,
                                   ginsim_stats* __restrict__ out) {
    const int c = blockIdx.x;
    Mom t{0.0, 0.0, 0.0, 0.0};
    for (int b = threadIdx.x; b < blocks; b += 64) t = merge(t, partial[c * blocks + b]);
#pragma unroll
    for (int mask = 32; mask >= 1; mask >>= 1) t = merge(t, shfl_xor(t, mask));
    if (threadIdx.x == 0) {
        if (c == 0) out->count = t.n;
        out->mean[c] = shift_of(e + (int64_t)c * runs) + t.mean;
        out->m2[c] = t.m2;
        out->maxabs[c] = t.mx;
    }
}

// Process-error statistics: the time axis of 64 runs is cut into kSeg segments, one wavefront each (coalesced across
// lanes, the truth row is wave-uniform -> scalar loads), a Welford accumulator per component; the segment records
// are Chan-merged in a fixed order through LDS.  HBM-bound: 72 B per sample*run read once; four wavefronts per SIMD
// at 65 536 runs hide the load latency a lone wavefront per run group would wait out every step.
// out = max|e|, mean, std (ddof = 0) as [runs][3][9] (run_major, what the host API returns) or [3][9][runs].
constexpr int kSeg = 4;

template <typename T>
__global__ void __launch_bounds__(64 * kSeg) process_stats_kernel(const T* __restrict__ traj, const double* __restrict__ ref,
                                                                 int64_t n, int64_t runs, int64_t j0, int pos_ned,
                                                                 int run_major, double* __restrict__ out, const ProcOrigin org) {
    __shared__ Mom part[kSeg][9][64];
    const int lane = threadIdx.x & 63, seg = threadIdx.x >> 6;
    const int64_t r = (int64_t)blockIdx.x * 64 + lane;
    const bool active = r < runs;
    const int64_t plane = n * runs;
    const uniform_ref truth = (uniform_ref)(uintptr_t)ref;
    const int64_t len = n - j0, per = (len + kSeg - 1) / kSeg;
    const int64_t jb = j0 + seg * per, je = (jb + per < n) ? jb + per : n;
    double mean[9], m2[9], mx[9];
#pragma unroll
    for (int c = 0; c < 9; ++c) { mean[c] = 0.0; m2[c] = 0.0; mx[c] = 0.0; }
    double cnt = 0.0;
    double o3[3] = {0.0, 0.0, 0.0};
    if (org.table && active) run_origin(org, r, o3);
    // the error of sample j against the truth
    auto error = [&](int64_t j, double (&e)[9]) {
        double x[9], t[9];
#pragma unroll
        for (int c = 0; c < 9; ++c) { x[c] = (double)traj[c * plane + j * runs + r]; t[c] = truth[9 * j + c]; }
        x[3] += o3[0]; x[4] += o3[1]; x[5] += o3[2];
        sample_error(x, t, pos_ned, e);
    };
    if (active) {
        for (int64_t j = jb; j < je; ++j) {
            double e[9];
            error(j, e);
            cnt += 1.0;
            const double icnt = rcp_nr(cnt);
#pragma unroll
            for (int c = 0; c < 9; ++c) {
                const double d = e[c] - mean[c];
                mean[c] = __builtin_fma(d, icnt, mean[c]);
                m2[c] = __builtin_fma(d, e[c] - mean[c], m2[c]);
                mx[c] = nan_max(fabs(e[c]), mx[c]);
            }
        }
        // a non-finite error (max|e| is inf or NaN) left the Welford mean NaN even where np.average is +-inf: that segment's
        // mean is formed again as a plain sum, and its M2 is NaN (see merge).  Once per segment, and only for such a run.
        bool bad = false;
#pragma unroll
        for (int c = 0; c < 9; ++c) bad |= !__builtin_isfinite(mx[c]);
        if (bad) {
            double sum[9];
#pragma unroll
            for (int c = 0; c < 9; ++c) sum[c] = 0.0;
            for (int64_t j = jb; j < je; ++j) {
                double e[9];
                error(j, e);
#pragma unroll
                for (int c = 0; c < 9; ++c) sum[c] += e[c];
            }
#pragma unroll
            for (int c = 0; c < 9; ++c)
                if (!__builtin_isfinite(mx[c])) { mean[c] = sum[c] / cnt; m2[c] = __builtin_nan(""); }
        }
    }
#pragma unroll
    for (int c = 0; c < 9; ++c) part[seg][c][lane] = Mom{cnt, mean[c], m2[c], mx[c]};
    __syncthreads();
    if (seg == 0 && active) {
#pragma unroll
        for (int c = 0; c < 9; ++c) {
            Mom t = part[0][c][lane];
#pragma unroll
            for (int k = 1; k < kSeg; ++k) t = merge(t, part[k][c][lane]);
            const double sd = t.n > 0.0 ? sqrt(t.m2 / t.n) : 0.0;
            if (run_major) {
                out[(r * 3 + 0) * 9 + c] = t.mx;
                out[(r * 3 + 1) * 9 + c] = t.mean;
                out[(r * 3 + 2) * 9 + c] = sd;
            } else {
                out[(0 * 9 + c) * runs + r] = t.mx;
                out[(1 * 9 + c) * runs + r] = t.mean;
                out[(2 * 9 + c) * runs + r] = sd;
            }
        }
    }
}

template <typename T>
static hipError_t launch_proc(const TrajView& v, int64_t j0, int pos_ned, int run_major, double* out, hipStream_t s) {
    hipLaunchKernelGGL((process_stats_kernel<T>), dim3((unsigned)((v.runs + 63) / 64)), dim3(64 * kSeg), 0, s,
                       static_cast<const T*>(v.traj), v.ref, v.n, v.runs, j0, pos_ned, run_major, out, v.org);
    return hipGetLastError();
}

hipError_t launch_process_stats(const TrajView& v, int64_t j0, int pos_ned, int run_major, double* out, hipStream_t s) {
    return v.f32 ? launch_proc<float>(v, j0, pos_ned, run_major, out, s) : launch_proc<double>(v, j0, pos_ned, run_major, out, s);
}

int stats_blocks(int64_t runs) {
    int64_t b = (runs + kStatBlock - 1) / kStatBlock;
    return (int)(b < 1 ? 1 : (b > 256 ? 256 : b));
}

size_t stats_scratch_bytes(int64_t runs) { return sizeof(Mom) * 9 * (size_t)stats_blocks(runs) + sizeof(ginsim_stats); }

hipError_t launch_end_stats(const double* end_err, int64_t runs, void* scratch, hipStream_t s) {
    const int blocks = stats_blocks(runs);
    Mom* partial = reinterpret_cast<Mom*>(scratch);
    ginsim_stats* out = reinterpret_cast<ginsim_stats*>(partial + 9 * blocks);
    hipLaunchKernelGGL(stats_partial_kernel, dim3(blocks, 9), dim3(kStatBlock), 0, s, end_err, runs, partial);
    hipLaunchKernelGGL(stats_final_kernel, dim3(9), dim3(64), 0, s, partial, blocks, end_err, runs, out);
    return hipGetLastError();
}

void stats_merge_host(const ginsim_stats* parts, int nparts, ginsim_stats* out) {
    for (int c = 0; c < 9; ++c) {
        Mom t{0.0, 0.0, 0.0, 0.0};
        for (int k = 0; k < nparts; ++k)
            t = merge(t, Mom{parts[k].count, parts[k].mean[c], parts[k].m2[c], parts[k].maxabs[c]});
        out->count = t.n;
        out->mean[c] = t.mean;
        out->m2[c] = t.m2;
        out->maxabs[c] = t.mx;
    }
}

}  // namespace ginsim
