// Error covariance across the runs: count, mean vector and the six co-moment sums of the position or the velocity error, at every
// requested sample (the record of cov_record.hpp).  The per-component moments of error_curve.hip do not say which way the error
// points; the cross moments do: rotated by the truth's yaw they are the along-track and cross-track variances, and their principal
// axes are the horizontal error ellipse (both on the host, ginsim/engine.py).
//
// Inputs as radial_keys_kernel (error_quantile.hip): which = 0 position (planes 3..5), 1 velocity (planes 6..8), the error formed by
// sample_error (moments.hpp), the fp32 form adds the origin table in fp64 as curve_partial_kernel does.  Only the three planes of
// the selected quantity are read: 24 B (fp64) or 12 B (fp32) per sample*run.
//
// Shape as error_curve.hip: the unit of work is a WAVEFRONT, one sample and one slice of the run axis, lanes stride along the runs,
// the truth row and the sample index are wave-uniform (scalar loads), `which` is a wave-uniform branch, every lane keeps one
// Welford accumulator and the lanes are folded with a shuffle butterfly.  No LDS, no barrier, no atomics:
//   many samples, few runs   one wavefront per sample (parts = 1), the record is written directly
//   few samples, many runs   the run axis is cut into `parts` slices so that the launch still fills the device; the slice
//                            records are folded by cov_final_kernel in a fixed order
// parts depends on (runs, m) alone: the same (n, runs, m) takes the same path and gives the same bytes at every launch.
//
// Conditioning: the lanes accumulate about a SHIFT, the error of the launch's first run at the sample (where finite, else 0), as
// curve_partial_kernel does.  Welford alone is not enough when |mean| >> sigma: the mean of the fold carries a rounding error of
// eps |mean|, which enters the next delta; about the shift every number is of the size of the spread.
//
// Non-finite values: a run with any of its three components not finite at the sample does not enter that sample's record; count is
// the number of runs that did.  The loop uses the same rule for the lanes past the end of the row: they hold NaN.
#include <hip/hip_runtime.h>
#include "ginsim.h"
#include "moments.hpp"
#include "cov_record.hpp"
#include "launch.hpp"

namespace ginsim {

constexpr int kCovBlock = 256;                      // four wavefronts, each with its own (sample, slice)
constexpr int kCovWaves = kCovBlock / 64;
constexpr int kCovMaxParts = 256;
constexpr int64_t kCovTargetWaves = 8192;           // 256 CUs x 4 SIMDs x 8 wavefronts
constexpr int kCovBatch = 2;                        // runs of a lane whose loads are in flight together

typedef const int64_t __attribute__((address_space(4))) * uniform_idx;

// the slices of the run axis for `m` samples of `runs` runs (a slice holds at least one step of a wavefront)
static int cov_parts(int64_t runs, int64_t m) {
    const int64_t most = (runs + 63) / 64;
    int64_t want = (kCovTargetWaves + m - 1) / m;
    if (want > most) want = most;
    if (want > kCovMaxParts) want = kCovMaxParts;
    return (int)(want < 1 ? 1 : want);
}

__device__ inline Cov shfl_xor(const Cov& a, int mask) {
    Cov o;
    o.n = __shfl_xor(a.n, mask, 64);
#pragma unroll
    for (int i = 0; i < 3; ++i) o.mean[i] = __shfl_xor(a.mean[i], mask, 64);
#pragma unroll
    for (int i = 0; i < 6; ++i) o.c[i] = __shfl_xor(a.c[i], mask, 64);
    return o;
}

// the error of run r against the truth (t0, t1, t2) of the selected quantity, from its three plane values
template <bool NED>
__device__ __forceinline__ void run_error(double a0, double a1, double a2, double t0, double t1, double t2, int which,
                                          const ProcOrigin& org, int64_t r, double (&e3)[3]) {
    double x[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, t[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, e[9];
    if (which) {                                    // wave-uniform
        x[6] = a0; x[7] = a1; x[8] = a2;
        t[6] = t0; t[7] = t1; t[8] = t2;
        sample_error(x, t, 0, e);
        e3[0] = e[6]; e3[1] = e[7]; e3[2] = e[8];
    } else {
        double o0 = 0.0, o1 = 0.0, o2 = 0.0;
        if (org.table) {                            // the run's initial state, as in the MC kernels (moments.hpp, ProcOrigin)
            const uint64_t call = org.ini_first + (uint64_t)r;
            const double* o = org.table + 3 * (call < (uint64_t)org.n_ini ? call : 0);
            o0 = o[0]; o1 = o[1]; o2 = o[2];
        }
        x[3] = a0 + o0; x[4] = a1 + o1; x[5] = a2 + o2;
        t[3] = t0; t[4] = t1; t[5] = t2;
        sample_error(x, t, NED ? 1 : 0, e);
        e3[0] = e[3]; e3[1] = e[4]; e3[2] = e[5];
    }
}

// out: [m] records when parts == 1, else [m][parts] slice records accumulated about `shift` ([m][3], written by slice 0 and added
// by cov_final_kernel)
template <typename T, bool NED>
__global__ void __launch_bounds__(kCovBlock) cov_partial_kernel(const T* __restrict__ traj, const double* __restrict__ ref, int64_t n,
                                                               int64_t runs, const int64_t* __restrict__ samples, int64_t m, int parts,
                                                               int which, Cov* __restrict__ out, double* __restrict__ shift,
                                                               const ProcOrigin org) {
    const int lane = threadIdx.x & 63;
    const int64_t unit = (int64_t)blockIdx.x * kCovWaves + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (unit >= m * parts) return;                  // wave-uniform
    const int64_t s = unit / parts;
    const int part = (int)(unit - s * parts);
    const int64_t j = samples ? ((uniform_idx)(uintptr_t)samples)[s] : s;
    const int64_t plane = n * runs;
    const int c0 = which ? 6 : 3;
    const uniform_ref truth = (uniform_ref)(uintptr_t)ref;
    const double t0 = truth[9 * j + c0], t1 = truth[9 * j + c0 + 1], t2 = truth[9 * j + c0 + 2];
    const T* row = traj + c0 * plane + j * runs;
    // the shift: the error of the launch's first run at this sample (every lane forms the same three numbers)
    double k3[3];
    run_error<NED>((double)row[0], (double)row[plane], (double)row[2 * plane], t0, t1, t2, which, org, 0, k3);
#pragma unroll
    for (int c = 0; c < 3; ++c) k3[c] = __builtin_isfinite(k3[c]) ? k3[c] : 0.0;
    Cov a{0.0, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}};
    const int64_t step = (int64_t)parts * 64;
    const T skip = (T)__builtin_nan("");
    for (int64_t r0 = (int64_t)part * 64 + lane; r0 < runs; r0 += kCovBatch * step) {
        T v[kCovBatch][3];
#pragma unroll
        for (int k = 0; k < kCovBatch; ++k) {
            const int64_t r = r0 + k * step;
            const bool in = r < runs;
            v[k][0] = in ? row[r] : skip;
            v[k][1] = in ? row[plane + r] : skip;
            v[k][2] = in ? row[2 * plane + r] : skip;
        }
#pragma unroll
        for (int k = 0; k < kCovBatch; ++k) {
            const int64_t r = r0 + k * step;
            double e[3];
            run_error<NED>((double)v[k][0], (double)v[k][1], (double)v[k][2], t0, t1, t2, which, org, r < runs ? r : 0, e);
            if (__builtin_isfinite(e[0]) && __builtin_isfinite(e[1]) && __builtin_isfinite(e[2])) {
                a.n += 1.0;
                const double icnt = rcp_nr(a.n);
                const double w0 = e[0] - k3[0], w1 = e[1] - k3[1], w2 = e[2] - k3[2];
                const double d0 = w0 - a.mean[0], d1 = w1 - a.mean[1], d2 = w2 - a.mean[2];
                a.mean[0] = __builtin_fma(d0, icnt, a.mean[0]);
                a.mean[1] = __builtin_fma(d1, icnt, a.mean[1]);
                a.mean[2] = __builtin_fma(d2, icnt, a.mean[2]);
                const double q0 = w0 - a.mean[0], q1 = w1 - a.mean[1], q2 = w2 - a.mean[2];
                a.c[0] = __builtin_fma(d0, q0, a.c[0]);
                a.c[1] = __builtin_fma(d0, q1, a.c[1]);
                a.c[2] = __builtin_fma(d0, q2, a.c[2]);
                a.c[3] = __builtin_fma(d1, q1, a.c[3]);
                a.c[4] = __builtin_fma(d1, q2, a.c[4]);
                a.c[5] = __builtin_fma(d2, q2, a.c[5]);
            }
        }
    }
#pragma unroll
    for (int mask = 32; mask >= 1; mask >>= 1) a = merge(a, shfl_xor(a, mask));
    if (lane == 0) {
        if (parts == 1) {
            out[unit] = finished(a, k3[0], k3[1], k3[2]);
        } else {
            if (part == 0) { shift[3 * s] = k3[0]; shift[3 * s + 1] = k3[1]; shift[3 * s + 2] = k3[2]; }
            out[unit] = a;
        }
    }
}

// one wavefront per sample: lanes fold the slice records they own (stride 64, fixed order), then the butterfly
__global__ void __launch_bounds__(64) cov_final_kernel(const Cov* __restrict__ partial, const double* __restrict__ shift, int parts,
                                                       Cov* __restrict__ out) {
    const int64_t s = blockIdx.x;
    Cov a{0.0, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}};
    for (int p = threadIdx.x; p < parts; p += 64) a = merge(a, partial[s * parts + p]);
#pragma unroll
    for (int mask = 32; mask >= 1; mask >>= 1) a = merge(a, shfl_xor(a, mask));
    if (threadIdx.x == 0) out[s] = finished(a, shift[3 * s], shift[3 * s + 1], shift[3 * s + 2]);
}

// scratch: [m] records, then (parts > 1) [m][parts] slice records and [m][3] shifts
size_t error_cov_scratch_bytes(int64_t runs, int64_t m) {
    const int parts = cov_parts(runs, m);
    size_t b = sizeof(Cov) * (size_t)m;
    if (parts > 1) b += sizeof(Cov) * (size_t)m * parts + sizeof(double) * 3 * (size_t)m;
    return b;
}

template <typename T>
static hipError_t launch_cov(const T* traj, const double* ref, int64_t n, int64_t runs, const int64_t* samples, int64_t m, int which,
                             int pos_ned, void* scratch, const ProcOrigin org, hipStream_t st) {
    const int parts = cov_parts(runs, m);
    Cov* out = reinterpret_cast<Cov*>(scratch);
    Cov* partial = out + m;
    double* shift = reinterpret_cast<double*>(partial + m * parts);
    const unsigned blocks = (unsigned)((m * parts + kCovWaves - 1) / kCovWaves);
    // the geodetic conversion only where the position is asked for in NED: the velocity takes the plain form
    hipLaunchKernelGGL((pos_ned && !which ? cov_partial_kernel<T, true> : cov_partial_kernel<T, false>), dim3(blocks), dim3(kCovBlock), 0,
                       st, traj, ref, n, runs, samples, m, parts, which, parts == 1 ? out : partial, shift, org);
    if (parts > 1) hipLaunchKernelGGL(cov_final_kernel, dim3((unsigned)m), dim3(64), 0, st, partial, shift, parts, out);
    return hipGetLastError();
}

hipError_t launch_error_cov(const double* traj, const double* ref, int64_t n, int64_t runs, const int64_t* samples, int64_t m,
                            int which, int pos_ned, void* scratch, hipStream_t st) {
    return launch_cov<double>(traj, ref, n, runs, samples, m, which, pos_ned, scratch, ProcOrigin{nullptr, 0, 0}, st);
}

hipError_t launch_error_cov_f32(const float* traj, const double* ref, int64_t n, int64_t runs, const int64_t* samples, int64_t m,
                                int which, int pos_ned, void* scratch, const double* origin, int64_t n_ini, uint64_t ini_first,
                                hipStream_t st) {
    return launch_cov<float>(traj, ref, n, runs, samples, m, which, pos_ned, scratch, ProcOrigin{origin, n_ini, ini_first}, st);
}

// host: the records of `nparts` sets of runs, each [m] records, folded record by record in the order given
void cov_merge_host(const double* parts, int nparts, int64_t m, double* out) {
    const Cov* in = reinterpret_cast<const Cov*>(parts);
    Cov* o = reinterpret_cast<Cov*>(out);
    for (int64_t i = 0; i < m; ++i) {
        Cov t{0.0, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}};
        for (int k = 0; k < nparts; ++k) t = merge(t, in[(int64_t)k * m + i]);
        o[i] = finished(t, 0.0, 0.0, 0.0);
    }
}

}  // namespace ginsim
