// What the error statistics share (stats.hip: over the runs at the last sample and over time per run; error_curve.hip: over the
// runs at every sample): the mergeable record (count, mean, M2, max|e|), its Chan merge with the non-finite rules of
// InsDataMgr.__array_stats, and the error of one sample of one run against the truth (array_error, ins_data_manager.py:519-553).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "fastmath.hpp"
#include "ins_math.hpp"

namespace ginsim {

struct Mom { double n, mean, m2, mx; };

// Non-finite errors follow __array_stats (np.max(np.abs(x)), np.average, np.std): a NaN anywhere makes all three NaN; an
// infinity makes the mean +-inf (NaN when both signs occur) and the std NaN.  The max of |e| keeps a NaN from either side.
__host__ __device__ inline double nan_max(double a, double b) { return (a > b || a != a) ? a : b; }

__host__ __device__ inline Mom merge(const Mom& a, const Mom& b) {
    const double n = a.n + b.n;
    if (n == 0.0) return Mom{0.0, 0.0, 0.0, 0.0};
    Mom o;
    o.n = n;
    if (__builtin_isfinite(a.mean) && __builtin_isfinite(b.mean)) {
        const double d = b.mean - a.mean;
        o.mean = a.mean + d * (b.n / n);
        o.m2 = a.m2 + b.m2 + d * d * (a.n * b.n / n);
    } else {                            // inf + finite = inf, inf - inf = NaN, NaN stays: the sign rule of np.average
        o.mean = a.mean + b.mean;
        o.m2 = __builtin_nan("");
    }
    o.mx = nan_max(a.mx, b.mx);
    return o;
}

__device__ inline Mom shfl_xor(const Mom& m, int mask) {
    return Mom{__shfl_xor(m.n, mask, 64), __shfl_xor(m.mean, mask, 64), __shfl_xor(m.m2, mask, 64),
               __shfl_xor(m.mx, mask, 64)};
}

// the truth row of a sample is the same for every lane of a wavefront: read through the constant address space it is a scalar load
typedef const double __attribute__((address_space(4))) * uniform_ref;

// attitude.angle_range_pi with the division by 2 pi replaced by a multiplication (same result: the two range
// fix-ups after the floor absorb a quotient that lands one ulp on the other side of an integer)
__device__ __forceinline__ double angle_range_pi_mul(double x) {
    double m = x - kTwoPi * floor(x * (1.0 / kTwoPi));
    if (m >= kTwoPi) m -= kTwoPi;
    if (m < 0.0) m += kTwoPi;
    return m > kPi ? m - kTwoPi : m;
}

// the error of a sample against its truth row t: x = the nine values of the run (position: origin already added)
__device__ __forceinline__ void sample_error(const double (&x)[9], const double (&t)[9], int pos_ned, double (&e)[9]) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {       // wrapped only when outside (-pi, pi), exactly as the online accumulator does (mc_kernel.hip wrap_pi3)
        const double d = x[c] - t[c];
        e[c] = fabs(d) < kPi ? d : angle_range_pi_mul(d);
    }
    if (pos_ned) {
        const Vec3 d = lla_error_ned(Vec3{x[3], x[4], x[5]}, Vec3{t[3], t[4], t[5]});
        e[3] = d.x; e[4] = d.y; e[5] = d.z;
    } else {
#pragma unroll
        for (int c = 3; c < 6; ++c) e[c] = x[c] - t[c];
    }
#pragma unroll
    for (int c = 6; c < 9; ++c) e[c] = x[c] - t[c];
}

}  // namespace ginsim
