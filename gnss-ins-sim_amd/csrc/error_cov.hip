// Error covariance across the runs: count, mean vector and the six co-moment sums of the position or the velocity error, at every
// requested sample (the record of cov_record.hpp).  The per-component moments of error_curve.hip do not say which way the error
// points; the cross moments do: rotated by the truth's yaw they are the along-track and cross-track variances, and their principal
// axes are the horizontal error ellipse (both on the host, ginsim/engine.py).
//
// The unit of work, the error of the selected quantity (quantity_error: which = 0 position, 1 velocity) and the cut of the run
// axis are traj_error.hpp's.  Only the three planes of the selected quantity are read: 24 B (fp64) or 12 B (fp32) per sample*run.
// Every lane keeps one Welford accumulator and the lanes are folded with a shuffle butterfly:
//   many samples, few runs   one wavefront per sample (parts = 1), the record is written directly
//   few samples, many runs   the run axis is cut into `parts` slices so that the launch still fills the device; the slice
//                            records are folded by cov_final_kernel in a fixed order
//
// Conditioning: the lanes accumulate about a SHIFT, the error of the launch's first run at the sample (where finite, else 0), as
// curve_partial_kernel does.  Welford alone is not enough when |mean| >> sigma: the mean of the fold carries a rounding error of
// eps |mean|, which enters the next delta; about the shift every number is of the size of the spread.
//
// Non-finite values: a run with any of its three components not finite at the sample does not enter that sample's record; count is
// the number of runs that did.  The loop uses the same rule for the lanes past the end of the row: they hold NaN.
#include <hip/hip_runtime.h>
#include "ginsim.h"
#include "traj_error.hpp"
#include "cov_record.hpp"

namespace ginsim {

constexpr int kCovMaxParts = 256;
constexpr int kCovBatch = 2;                        // runs of a lane whose loads are in flight together

__device__ inline Cov shfl_xor(const Cov& a, int mask) {
    Cov o;
    o.n = __shfl_xor(a.n, mask, 64);
#pragma unroll
    for (int i = 0; i < 3; ++i) o.mean[i] = __shfl_xor(a.mean[i], mask, 64);
#pragma unroll
    for (int i = 0; i < 6; ++i) o.c[i] = __shfl_xor(a.c[i], mask, 64);
    return o;
}

// out: [m] records when parts == 1, else [m][parts] slice records accumulated about `shift` ([m][3], written by slice 0 and added
// by cov_final_kernel)
template <typename T, bool NED>
__global__ void __launch_bounds__(kUnitBlock) cov_partial_kernel(const T* __restrict__ traj, const double* __restrict__ ref, int64_t n,
                                                               int64_t runs, const int64_t* __restrict__ samples, int64_t m, int parts,
                                                               int which, Cov* __restrict__ out, double* __restrict__ shift,
                                                               const ProcOrigin org) {
    const int lane = threadIdx.x & 63;
    const int64_t unit = wave_unit();
    if (unit >= m * parts) return;
    const WorkUnit w(unit, ref, n, runs, samples, parts);
    const int64_t s = w.s, j = w.j, plane = w.plane;
    const int part = (int)(unit - s * parts), c0 = which ? 6 : 3;
    const uniform_ref truth = w.truth;
    const double t0 = truth[9 * j + c0], t1 = truth[9 * j + c0 + 1], t2 = truth[9 * j + c0 + 2];
    const T* row = traj + c0 * plane + j * runs;
    // the shift: the error of the launch's first run at this sample (every lane forms the same three numbers)
    double k3[3];
    quantity_error<NED>((double)row[0], (double)row[plane], (double)row[2 * plane], t0, t1, t2, which, org, 0, k3);
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
            quantity_error<NED>((double)v[k][0], (double)v[k][1], (double)v[k][2], t0, t1, t2, which, org, r < runs ? r : 0, e);
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
size_t error_cov_scratch_bytes(const TrajView& v) {
    const int parts = run_slices(v.runs, v.m, 64, kCovMaxParts);
    size_t b = sizeof(Cov) * (size_t)v.m;
    if (parts > 1) b += sizeof(Cov) * (size_t)v.m * parts + sizeof(double) * 3 * (size_t)v.m;
    return b;
}

template <typename T>
static hipError_t launch_cov(const TrajView& v, int which, int pos_ned, void* scratch, hipStream_t st) {
    const int64_t m = v.m;
    const int parts = run_slices(v.runs, m, 64, kCovMaxParts);
    Cov* out = reinterpret_cast<Cov*>(scratch);
    Cov* partial = out + m;
    double* shift = reinterpret_cast<double*>(partial + m * parts);
    // the geodetic conversion only where the position is asked for in NED: the velocity takes the plain form
    hipLaunchKernelGGL((pos_ned && !which ? cov_partial_kernel<T, true> : cov_partial_kernel<T, false>), dim3(unit_blocks(m, parts)),
                       dim3(kUnitBlock), 0, st, static_cast<const T*>(v.traj), v.ref, v.n, v.runs, v.samples, m, parts, which,
                       parts == 1 ? out : partial, shift, v.org);
    if (parts > 1) hipLaunchKernelGGL(cov_final_kernel, dim3((unsigned)m), dim3(64), 0, st, partial, shift, parts, out);
    return hipGetLastError();
}

hipError_t launch_error_cov(const TrajView& v, int which, int pos_ned, void* scratch, hipStream_t st) {
    return v.f32 ? launch_cov<float>(v, which, pos_ned, scratch, st) : launch_cov<double>(v, which, pos_ned, scratch, st);
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
