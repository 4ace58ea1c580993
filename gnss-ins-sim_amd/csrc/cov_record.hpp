// The mergeable covariance record of error_cov.hip: count, mean[3] and the co-moment sums C[6] = sum (e_a - mean_a)(e_b - mean_b) of
// a 3-vector across a set of runs, in the order 00, 01, 02, 11, 12, 22 (GINSIM_COV_RECORD doubles).  Its Chan merge is written once
// for the device kernels and for the host merge of blocks, devices and ranks.  Unlike the record of moments.hpp it never holds a
// run with a non-finite component (such a run does not enter), so the merge has no non-finite rules: only the empty set is special.
#pragma once
#include <hip/hip_runtime.h>
#include "ginsim.h"

namespace ginsim {

struct Cov { double n, mean[3], c[6]; };
static_assert(sizeof(Cov) == sizeof(double) * GINSIM_COV_RECORD, "Cov is GINSIM_COV_RECORD doubles");

// C = C_a + C_b + dd^T n_a n_b / n, d = mean_b - mean_a.  An empty side (n = 0, whatever else it holds) leaves the other side's
// bits as they are: a set of one run keeps its exactly zero co-moments through every fold.
__host__ __device__ inline Cov merge(const Cov& a, const Cov& b) {
    if (b.n == 0.0) return a;
    if (a.n == 0.0) return b;
    const double n = a.n + b.n;
    const double wb = b.n / n, wab = a.n * b.n / n;
    const double d0 = b.mean[0] - a.mean[0], d1 = b.mean[1] - a.mean[1], d2 = b.mean[2] - a.mean[2];
    Cov o;
    o.n = n;
    o.mean[0] = a.mean[0] + d0 * wb;
    o.mean[1] = a.mean[1] + d1 * wb;
    o.mean[2] = a.mean[2] + d2 * wb;
    o.c[0] = a.c[0] + b.c[0] + d0 * d0 * wab;
    o.c[1] = a.c[1] + b.c[1] + d0 * d1 * wab;
    o.c[2] = a.c[2] + b.c[2] + d0 * d2 * wab;
    o.c[3] = a.c[3] + b.c[3] + d1 * d1 * wab;
    o.c[4] = a.c[4] + b.c[4] + d1 * d2 * wab;
    o.c[5] = a.c[5] + b.c[5] + d2 * d2 * wab;
    return o;
}

// the record as it leaves the library: a set without runs has no mean and no covariance (NaN, count 0); `shift` is what the
// kernels accumulated about (0 on the host)
__host__ __device__ inline Cov finished(Cov a, double s0, double s1, double s2) {
    if (a.n == 0.0) {
        const double q = __builtin_nan("");
        return Cov{0.0, {q, q, q}, {q, q, q, q, q, q}};
    }
    a.mean[0] += s0; a.mean[1] += s1; a.mean[2] += s2;
    return a;
}

}  // namespace ginsim
