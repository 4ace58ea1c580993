// Error-growth curves: count, mean, M2 and max|e| of the 9 error components ACROSS the runs, at every requested sample.
//
// At sample j this is InsDataMgr.__end_point_error_stats + __array_stats (gnss_ins_sim/sim/ins_data_manager.py:717-759,
// 797-808) applied to the series cut after j: calc_data_err / array_error (attitude wrapped, extra_opt='ned' included), then
// {'max': np.max(np.abs(x), 0), 'avg': np.average(x, 0), 'std': np.std(x, 0)} over the runs.  The records are the mergeable
// ones of stats.hip (moments.hpp), so the curves of blocks of runs, of devices and of ranks combine with the same Chan merge.
//
// The unit of work, the origin lookup and the cut of the run axis are traj_error.hpp's: a wavefront takes one sample and one slice
// of the run axis.  Here its lanes take two runs per load where the rows are 16-byte aligned, every lane keeps one Welford
// accumulator per component and the lanes are folded with the shuffle butterfly of stats.hip:
//   many samples, few runs   one wavefront per sample (parts = 1), the record is written directly
//   few samples, many runs   the run axis is cut into `parts` slices so that the launch still fills the device; the slice
//                            records are folded by curve_final_kernel in a fixed order (as stats_partial / stats_final do)
// HBM-bound: 72 B (fp64) per sample*run, read once.
#include <hip/hip_runtime.h>
#include "ginsim.h"
#include "traj_error.hpp"

namespace ginsim {

constexpr int kCurveMaxParts = 256;

// two runs per lane and load: rows of an even number of runs from a 16-byte aligned base, and enough runs to give every
// lane of a wavefront two of them
static int curve_vec(const void* traj, int64_t runs) {
    return (runs % 2 == 0 && runs >= 128 && (uintptr_t)traj % 16 == 0) ? 2 : 1;
}

template <typename T, int V> struct RunVec;
template <> struct RunVec<double, 1> { typedef double type; };
template <> struct RunVec<float, 1> { typedef float type; };
template <> struct RunVec<double, 2> { typedef double2 type; };
template <> struct RunVec<float, 2> { typedef float2 type; };

template <typename T> __device__ __forceinline__ double lane_of(const T& v, int) { return (double)v; }
__device__ __forceinline__ double lane_of(const double2& v, int k) { return k ? v.y : v.x; }
__device__ __forceinline__ double lane_of(const float2& v, int k) { return (double)(k ? v.y : v.x); }

// out: [m][9] records when parts == 1, else [m][parts][9] slice records (accumulated about `shift`, which is added by
// curve_final_kernel); shift: [m][9], the error of run 0 at the sample where it is finite, else 0 (stats.hip, shift_of)
// NED: the position error in local NED metres (lla_error_ned); a template parameter, so that the plain form does not carry the
// registers of the geodetic conversion
template <typename T, int V, bool NED>
__global__ void __launch_bounds__(kUnitBlock) curve_partial_kernel(const T* __restrict__ traj, const double* __restrict__ ref,
                                                                   int64_t n, int64_t runs, const int64_t* __restrict__ samples,
                                                                   int64_t m, int parts, Mom* __restrict__ out,
                                                                   double* __restrict__ shift, const ProcOrigin org) {
    constexpr int pos_ned = NED ? 1 : 0;
    typedef typename RunVec<T, V>::type Vec;
    const int lane = threadIdx.x & 63;
    const int64_t unit = wave_unit();
    if (unit >= m * parts) return;
    const WorkUnit w(unit, ref, n, runs, samples, parts);
    const int64_t s = w.s, j = w.j, plane = w.plane;
    const int part = (int)(unit - s * parts);
    const uniform_ref truth = w.truth;
    const T* row = traj + j * runs;
    double t[9];
#pragma unroll
    for (int c = 0; c < 9; ++c) t[c] = truth[9 * j + c];
    // the shift: the error of the launch's first run at this sample (every lane forms the same nine numbers)
    double k9[9];
    {
        double x[9], o3[3] = {0.0, 0.0, 0.0};
#pragma unroll
        for (int c = 0; c < 9; ++c) x[c] = (double)row[c * plane];
        if (org.table) run_origin(org, 0, o3);
        x[3] += o3[0]; x[4] += o3[1]; x[5] += o3[2];
        sample_error(x, t, pos_ned, k9);
#pragma unroll
        for (int c = 0; c < 9; ++c) k9[c] = __builtin_isfinite(k9[c]) ? k9[c] : 0.0;
    }
    double mean[9], m2[9], mx[9];
#pragma unroll
    for (int c = 0; c < 9; ++c) { mean[c] = 0.0; m2[c] = 0.0; mx[c] = 0.0; }
    double cnt = 0.0;
    for (int64_t r0 = ((int64_t)part * 64 + lane) * V; r0 < runs; r0 += (int64_t)parts * 64 * V) {     // r0 + V <= runs: V divides runs
        Vec v[9];
#pragma unroll
        for (int c = 0; c < 9; ++c) v[c] = *reinterpret_cast<const Vec*>(row + c * plane + r0);
#pragma unroll
        for (int u = 0; u < V; ++u) {
            double x[9], e[9], o3[3] = {0.0, 0.0, 0.0};
#pragma unroll
            for (int c = 0; c < 9; ++c) x[c] = lane_of(v[c], u);
            if (org.table) run_origin(org, r0 + u, o3);
            x[3] += o3[0]; x[4] += o3[1]; x[5] += o3[2];
            sample_error(x, t, pos_ned, e);
            cnt += 1.0;
            const double icnt = rcp_nr(cnt);
#pragma unroll
            for (int c = 0; c < 9; ++c) {
                const double w = e[c] - k9[c];
                const double d = w - mean[c];
                const double mean_ok = __builtin_fma(d, icnt, mean[c]);
                const double m2_ok = __builtin_fma(d, w - mean_ok, m2[c]);
                const bool ok = __builtin_isfinite(w) && __builtin_isfinite(mean[c]);        // else: see merge (moments.hpp)
                mean[c] = ok ? mean_ok : mean[c] + w;
                m2[c] = ok ? m2_ok : __builtin_nan("");
                mx[c] = nan_max(fabs(e[c]), mx[c]);
            }
        }
    }
#pragma unroll
    for (int c = 0; c < 9; ++c) {
        Mom a{cnt, mean[c], m2[c], mx[c]};
#pragma unroll
        for (int mask = 32; mask >= 1; mask >>= 1) a = merge(a, shfl_xor(a, mask));
        if (lane == 0) {
            if (parts == 1) a.mean += k9[c];
            else if (part == 0) shift[s * 9 + c] = k9[c];
            out[unit * 9 + c] = a;
        }
    }
}

// one wavefront per (sample, component): lanes fold the slice records they own (stride 64, fixed order), then the butterfly
__global__ void __launch_bounds__(64) curve_final_kernel(const Mom* __restrict__ partial, const double* __restrict__ shift, int parts,
                                                         Mom* __restrict__ out) {
    const int64_t rec = blockIdx.x;                 // s * 9 + c
    const int64_t s = rec / 9;
    const int c = (int)(rec - s * 9);
    Mom a{0.0, 0.0, 0.0, 0.0};
    for (int p = threadIdx.x; p < parts; p += 64) a = merge(a, partial[(s * parts + p) * 9 + c]);
#pragma unroll
    for (int mask = 32; mask >= 1; mask >>= 1) a = merge(a, shfl_xor(a, mask));
    if (threadIdx.x == 0) {
        a.mean += shift[rec];
        out[rec] = a;
    }
}

// scratch: [m][9] records, then (parts > 1) [m][parts][9] slice records and [m][9] shifts
size_t error_curve_scratch_bytes(const TrajView& v) {
    const int parts = run_slices(v.runs, v.m, 64 * curve_vec(v.traj, v.runs), kCurveMaxParts);
    size_t b = sizeof(Mom) * 9 * (size_t)v.m;
    if (parts > 1) b += sizeof(Mom) * 9 * (size_t)v.m * parts + sizeof(double) * 9 * (size_t)v.m;
    return b;
}

template <typename T>
static hipError_t launch_curve(const TrajView& v, int pos_ned, void* scratch, hipStream_t st) {
    const T* traj = static_cast<const T*>(v.traj);
    const int64_t m = v.m;
    const int V = curve_vec(traj, v.runs);
    const int parts = run_slices(v.runs, m, 64 * V, kCurveMaxParts);
    Mom* out = reinterpret_cast<Mom*>(scratch);
    Mom* partial = out + 9 * m;
    double* shift = reinterpret_cast<double*>(partial + 9 * m * parts);
    Mom* first = parts == 1 ? out : partial;
    void (*kernel)(const T*, const double*, int64_t, int64_t, const int64_t*, int64_t, int, Mom*, double*, const ProcOrigin) =
        V == 2 ? (pos_ned ? curve_partial_kernel<T, 2, true> : curve_partial_kernel<T, 2, false>)
               : (pos_ned ? curve_partial_kernel<T, 1, true> : curve_partial_kernel<T, 1, false>);
    hipLaunchKernelGGL(kernel, dim3(unit_blocks(m, parts)), dim3(kUnitBlock), 0, st, traj, v.ref, v.n, v.runs, v.samples, m, parts, first,
                       shift, v.org);
    if (parts > 1)
        hipLaunchKernelGGL(curve_final_kernel, dim3((unsigned)(9 * m)), dim3(64), 0, st, partial, shift, parts, out);
    return hipGetLastError();
}

hipError_t launch_error_curve(const TrajView& v, int pos_ned, void* scratch, hipStream_t st) {
    return v.f32 ? launch_curve<float>(v, pos_ned, scratch, st) : launch_curve<double>(v, pos_ned, scratch, st);
}

// host: the curves of `nparts` sets of runs, each [m][9] records, folded record by record in the order given
void curve_merge_host(const double* parts, int nparts, int64_t m, double* out) {
    const Mom* in = reinterpret_cast<const Mom*>(parts);
    Mom* o = reinterpret_cast<Mom*>(out);
    for (int64_t i = 0; i < 9 * m; ++i) {
        Mom t{0.0, 0.0, 0.0, 0.0};
        for (int k = 0; k < nparts; ++k) t = merge(t, in[(int64_t)k * 9 * m + i]);
        o[i] = t;
    }
}

}  // namespace ginsim
