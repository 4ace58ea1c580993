// Error-growth curves: count, mean, M2 and max|e| of the 9 error components ACROSS the runs, at every requested sample.
//
// At sample j this is InsDataMgr.__end_point_error_stats + __array_stats (gnss_ins_sim/sim/ins_data_manager.py:717-759,
// 797-808) applied to the series cut after j: calc_data_err / array_error (attitude wrapped, extra_opt='ned' included), then
// {'max': np.max(np.abs(x), 0), 'avg': np.average(x, 0), 'std': np.std(x, 0)} over the runs.  The records are the mergeable
// ones of stats.hip (moments.hpp), so the curves of blocks of runs, of devices and of ranks combine with the same Chan merge.
//
// Layout: the trajectories are [9][n][runs], so the row of one (component, sample) is contiguous across runs.  The unit of work
// is a WAVEFRONT: it takes one sample and one slice of the run axis, its lanes stride along the runs (two runs per lane and
// load where the rows are 16-byte aligned), the truth row is wave-uniform (scalar loads), every lane keeps one Welford
// accumulator per component and the lanes are folded with the shuffle butterfly of stats.hip.  No LDS, no barrier, no atomics:
//   many samples, few runs   one wavefront per sample (parts = 1), the record is written directly
//   few samples, many runs   the run axis is cut into `parts` slices so that the launch still fills the device; the slice
//                            records are folded by curve_final_kernel in a fixed order (as stats_partial / stats_final do)
// HBM-bound: 72 B (fp64) per sample*run, read once.
#include <hip/hip_runtime.h>
#include "ginsim.h"
#include "moments.hpp"
#include "launch.hpp"

namespace ginsim {

constexpr int kCurveBlock = 256;                    // four wavefronts, each with its own (sample, slice)
constexpr int kCurveWaves = kCurveBlock / 64;
constexpr int kCurveMaxParts = 256;
constexpr int64_t kCurveTargetWaves = 8192;         // 256 CUs x 4 SIMDs x 8 wavefronts

typedef const int64_t __attribute__((address_space(4))) * uniform_idx;

// the slices of the run axis for `m` samples of `runs` runs, V runs per lane and step
static int curve_parts(int64_t runs, int64_t m, int V) {
    const int64_t most = (runs + 64 * V - 1) / (64 * V);            // a slice holds at least one step of a wavefront
    int64_t want = (kCurveTargetWaves + m - 1) / m;
    if (want > most) want = most;
    if (want > kCurveMaxParts) want = kCurveMaxParts;
    return (int)(want < 1 ? 1 : want);
}

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

__device__ __forceinline__ void origin_of(const ProcOrigin& org, int64_t r, double (&o3)[3]) {
    const uint64_t call = org.ini_first + (uint64_t)r;
    const double* row = org.table + 3 * (call < (uint64_t)org.n_ini ? call : 0);
    o3[0] = row[0]; o3[1] = row[1]; o3[2] = row[2];
}

// out: [m][9] records when parts == 1, else [m][parts][9] slice records (accumulated about `shift`, which is added by
// curve_final_kernel); shift: [m][9], the error of run 0 at the sample where it is finite, else 0 (stats.hip, shift_of)
// NED: the position error in local NED metres (lla_error_ned); a template parameter, so that the plain form does not carry the
// registers of the geodetic conversion
template <typename T, int V, bool NED>
__global__ void __launch_bounds__(kCurveBlock) curve_partial_kernel(const T* __restrict__ traj, const double* __restrict__ ref,
                                                                   int64_t n, int64_t runs, const int64_t* __restrict__ samples,
                                                                   int64_t m, int parts, Mom* __restrict__ out,
                                                                   double* __restrict__ shift, const ProcOrigin org) {
    constexpr int pos_ned = NED ? 1 : 0;
    typedef typename RunVec<T, V>::type Vec;
    const int lane = threadIdx.x & 63;
    const int64_t unit = (int64_t)blockIdx.x * kCurveWaves + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (unit >= m * parts) return;                  // wave-uniform
    const int64_t s = unit / parts;
    const int part = (int)(unit - s * parts);
    const int64_t j = samples ? ((uniform_idx)(uintptr_t)samples)[s] : s;
    const int64_t plane = n * runs;
    const uniform_ref truth = (uniform_ref)(uintptr_t)ref;
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
        if (org.table) origin_of(org, 0, o3);
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
            if (org.table) origin_of(org, r0 + u, o3);
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
size_t error_curve_scratch_bytes(const void* traj, int64_t runs, int64_t m) {
    const int parts = curve_parts(runs, m, curve_vec(traj, runs));
    size_t b = sizeof(Mom) * 9 * (size_t)m;
    if (parts > 1) b += sizeof(Mom) * 9 * (size_t)m * parts + sizeof(double) * 9 * (size_t)m;
    return b;
}

template <typename T>
static hipError_t launch_curve(const T* traj, const double* ref, int64_t n, int64_t runs, const int64_t* samples, int64_t m,
                               int pos_ned, void* scratch, const ProcOrigin org, hipStream_t st) {
    const int V = curve_vec(traj, runs);
    const int parts = curve_parts(runs, m, V);
    Mom* out = reinterpret_cast<Mom*>(scratch);
    Mom* partial = out + 9 * m;
    double* shift = reinterpret_cast<double*>(partial + 9 * m * parts);
    const unsigned blocks = (unsigned)((m * parts + kCurveWaves - 1) / kCurveWaves);
    Mom* first = parts == 1 ? out : partial;
    void (*kernel)(const T*, const double*, int64_t, int64_t, const int64_t*, int64_t, int, Mom*, double*, const ProcOrigin) =
        V == 2 ? (pos_ned ? curve_partial_kernel<T, 2, true> : curve_partial_kernel<T, 2, false>)
               : (pos_ned ? curve_partial_kernel<T, 1, true> : curve_partial_kernel<T, 1, false>);
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(kCurveBlock), 0, st, traj, ref, n, runs, samples, m, parts, first, shift, org);
    if (parts > 1)
        hipLaunchKernelGGL(curve_final_kernel, dim3((unsigned)(9 * m)), dim3(64), 0, st, partial, shift, parts, out);
    return hipGetLastError();
}

hipError_t launch_error_curve(const double* traj, const double* ref, int64_t n, int64_t runs, const int64_t* samples, int64_t m,
                              int pos_ned, void* scratch, hipStream_t st) {
    return launch_curve<double>(traj, ref, n, runs, samples, m, pos_ned, scratch, ProcOrigin{nullptr, 0, 0}, st);
}

hipError_t launch_error_curve_f32(const float* traj, const double* ref, int64_t n, int64_t runs, const int64_t* samples, int64_t m,
                                  int pos_ned, void* scratch, const double* origin, int64_t n_ini, uint64_t ini_first, hipStream_t st) {
    return launch_curve<float>(traj, ref, n, runs, samples, m, pos_ned, scratch, ProcOrigin{origin, n_ini, ini_first}, st);
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
