// Soft / hard-iron magnetometer calibration, one lane per run.
//
// Restates, per run:
//   MagCal.run                      demo_algorithms/mag_calibrate.py:76-88 (the ranges replace its six prompts)
//   MagCalibrate, GetPointsNormal, GetMagOffset    demo_algorithms/mag_calibrate_src/src/MagCalibration.c:34-306
//   pathgen.mag_gen                 pathgen.py:658-661 (mag_synth.hpp: sample j of run r is the one aux_mag_kernel writes)
//
// Two passes over a run's samples, a third only when mag_cal is kept:
//   1. per range the normal equations M^T M v = M^T 1 (nine sums) -> v, sign and norm -> a row of orthMtx;
//   2. u = orthMtx . m for every row of the three ranges: the (max - min) of the columns the sensitivities take, and the moments
//      of degree <= 3 of u (sum u, sum u u^T, sum u_i u_k^2).  sens is diagonal, so the 4x4 normal equations of the sphere fit over
//      w = sens . u (H = [2w, 1], B = |w|^2) are those moments scaled afterwards;
//   3. (kept) w - centre, the three ranges stacked.
// In the generated form a pass makes the samples again from the counter RNG: the series is never stored.
//
// IEEE all the way: nothing is clamped or tested.  The reference multiplies by the FULL matrices diag(sens) and orthMtx, so a
// non-finite entry reaches every element of its row sum (0 * NaN); the products with the zeros are kept where that decides the
// non-finite pattern of an output (x + 0 * y == x for finite y: the finite values are the same).  max / min start from the first
// row and compare with > / <, as vecMax / vecMin do.
#include <hip/hip_runtime.h>
#include "ginsim.h"
#include "ins_math.hpp"
#include "philox.hpp"
#include "sensor_synth.hpp"
#include "mag_synth.hpp"
#include "launch.hpp"

namespace ginsim {

// A x = b by elimination without pivoting (the normal matrices are symmetric positive definite when the data are not degenerate;
// when they are, the divisions by zero give the non-finite answer).  Fully unrolled: A and b live in registers.
template <int N>
__device__ __forceinline__ void solve(double (&A)[N][N], double (&b)[N], double (&x)[N]) {
#pragma unroll
    for (int k = 0; k < N; ++k) {
#pragma unroll
        for (int i = k + 1; i < N; ++i) {
            const double f = A[i][k] / A[k][k];
#pragma unroll
            for (int j = k; j < N; ++j) A[i][j] = A[i][j] - f * A[k][j];
            b[i] = b[i] - f * b[k];
        }
    }
#pragma unroll
    for (int i = N - 1; i >= 0; --i) {
        double s = b[i];
#pragma unroll
        for (int j = i + 1; j < N; ++j) s = s - A[i][j] * x[j];
        x[i] = s / A[i][i];
    }
}

// everything a lane needs to read or make sample j of its run
template <bool GIVEN>
struct MagSource {
    const double* in;       // GIVEN: &in_mag[run]
    int64_t runs, plane;
    uniform_ptr ref;
    RngKey key;
    NormalTables tab;
    double si[9], hi[3], sd[3];

    __device__ __forceinline__ Vec3 sample(int64_t j) const {
        if (GIVEN) {
            const double* p = in + j * runs;
            return Vec3{__builtin_nontemporal_load(p), __builtin_nontemporal_load(p + plane), __builtin_nontemporal_load(p + 2 * plane)};
        }
        double z[3];
        mag_normals(key, (uint32_t)j, tab, z);
        const double v[3] = {ref[3 * j] + hi[0], ref[3 * j + 1] + hi[1], ref[3 * j + 2] + hi[2]};
        return Vec3{mag_axis(si, v, sd[0], z[0]), mag_axis(si + 3, v, sd[1], z[1]), mag_axis(si + 6, v, sd[2], z[2])};
    }
};

// GetPointsNormal over rows [j0, j1), then the sign and the norm MagCalibrate gives it (MagCalibration.c:45-71, 200-222)
template <bool GIVEN>
__device__ __forceinline__ void range_normal(const MagSource<GIVEN>& src, int64_t j0, int64_t j1, double (&v)[3]) {
    double a00 = 0.0, a01 = 0.0, a02 = 0.0, a11 = 0.0, a12 = 0.0, a22 = 0.0, b0 = 0.0, b1 = 0.0, b2 = 0.0;
    for (int64_t j = j0; j < j1; ++j) {
        const Vec3 m = src.sample(j);
        a00 = __builtin_fma(m.x, m.x, a00); a01 = __builtin_fma(m.x, m.y, a01); a02 = __builtin_fma(m.x, m.z, a02);
        a11 = __builtin_fma(m.y, m.y, a11); a12 = __builtin_fma(m.y, m.z, a12); a22 = __builtin_fma(m.z, m.z, a22);
        b0 += m.x; b1 += m.y; b2 += m.z;
    }
    double A[3][3] = {{a00, a01, a02}, {a01, a11, a12}, {a02, a12, a22}}, b[3] = {b0, b1, b2};
    solve<3>(A, b, v);
    // vecMax over |v|: the first largest; a NaN never wins a > comparison
    const double c0 = fabs(v[0]), c1 = fabs(v[1]), c2 = fabs(v[2]);
    double big = v[0], cb = c0;
    if (c1 > cb) { big = v[1]; cb = c1; }
    if (c2 > cb) { big = v[2]; }
    if (big < 0.0) { v[0] = -1.0 * v[0]; v[1] = -1.0 * v[1]; v[2] = -1.0 * v[2]; }
    const double nrm = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    v[0] = v[0] / nrm; v[1] = v[1] / nrm; v[2] = v[2] / nrm;
}

__device__ __forceinline__ void rotate(const double (&O)[3][3], const Vec3& m, double (&u)[3]) {
#pragma unroll
    for (int i = 0; i < 3; ++i) u[i] = O[i][0] * m.x + O[i][1] * m.y + O[i][2] * m.z;
}

// the moments of u over all three ranges the sphere fit is made of
struct Moments {
    double cnt, s1[3], s2[6], s3[3][3];     // s2: 00 01 02 11 12 22; s3[i][k] = sum u_i u_k^2
    __device__ __forceinline__ void clear() {
        cnt = 0.0;
        for (int i = 0; i < 3; ++i) { s1[i] = 0.0; for (int k = 0; k < 3; ++k) s3[i][k] = 0.0; }
        for (int i = 0; i < 6; ++i) s2[i] = 0.0;
    }
    __device__ __forceinline__ void add(const double (&u)[3]) {
        const double q[3] = {u[0] * u[0], u[1] * u[1], u[2] * u[2]};
        cnt += 1.0;
        s2[0] += q[0]; s2[3] += q[1]; s2[5] += q[2];
        s2[1] = __builtin_fma(u[0], u[1], s2[1]); s2[2] = __builtin_fma(u[0], u[2], s2[2]); s2[4] = __builtin_fma(u[1], u[2], s2[4]);
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            s1[i] += u[i];
#pragma unroll
            for (int k = 0; k < 3; ++k) s3[i][k] = __builtin_fma(u[i], q[k], s3[i][k]);
        }
    }
};

// second pass over rows [j0, j1): (max - min) of column CN over (max - min) of column CD, and the moments
template <bool GIVEN, int CN, int CD>
__device__ __forceinline__ double range_ratio(const MagSource<GIVEN>& src, int64_t j0, int64_t j1, const double (&O)[3][3], Moments& mo) {
    double nmax = 0.0, nmin = 0.0, dmax = 0.0, dmin = 0.0;
    for (int64_t j = j0; j < j1; ++j) {
        double u[3];
        rotate(O, src.sample(j), u);
        if (j == j0) {      // wave-uniform
            nmax = nmin = u[CN];
            dmax = dmin = u[CD];
        } else {
            nmax = u[CN] > nmax ? u[CN] : nmax;
            nmin = u[CN] < nmin ? u[CN] : nmin;
            dmax = u[CD] > dmax ? u[CD] : dmax;
            dmin = u[CD] < dmin ? u[CD] : dmin;
        }
        mo.add(u);
    }
    return (nmax - nmin) / (dmax - dmin);
}

// third pass over rows [j0, j1): mag_cal rows `at` onwards of this run
template <bool GIVEN>
__device__ __forceinline__ void range_calibrated(const MagSource<GIVEN>& src, int64_t j0, int64_t j1, const double (&O)[3][3],
                                                 const double (&s)[3], const double (&p)[4], double* out, int64_t at, int64_t total,
                                                 int64_t runs) {
    for (int64_t j = j0; j < j1; ++j, ++at) {
        double u[3];
        rotate(O, src.sample(j), u);
        // mtxMultiplyVec with the full diag(sens): the zeros multiply the other components
        const double w0 = s[0] * u[0] + 0.0 * u[1] + 0.0 * u[2];
        const double w1 = 0.0 * u[0] + s[1] * u[1] + 0.0 * u[2];
        const double w2 = 0.0 * u[0] + 0.0 * u[1] + s[2] * u[2];
        __builtin_nontemporal_store(w0 - p[0], out + at * runs);
        __builtin_nontemporal_store(w1 - p[1], out + (total + at) * runs);
        __builtin_nontemporal_store(w2 - p[2], out + (2 * total + at) * runs);
    }
}

template <bool GIVEN>
__global__ void __launch_bounds__(256) magcal_kernel(const ginsim_magcal_params a) {
    __shared__ uint32_t ntab[GIVEN ? 4 : kNormalLdsWords];
    NormalTables tab{};
    if (!GIVEN) {
        tab = fill_normal_tables(ntab, threadIdx.x, blockDim.x);
        __syncthreads();
    }
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= a.runs) return;
    const int64_t runs = a.runs;
    const uint64_t grun = a.run_offset + (uint64_t)r;
    MagSource<GIVEN> src;
    src.in = GIVEN ? a.in_mag + r : nullptr;
    src.runs = runs;
    src.plane = a.n * runs;
    src.ref = as_uniform(a.ref_mag);
    src.key = RngKey{(uint32_t)a.seed, (uint32_t)(a.seed >> 32), (uint32_t)grun, (uint32_t)(grun >> 32)};
    src.tab = tab;
    for (int i = 0; i < 9; ++i) src.si[i] = a.mag_si[i];
    for (int i = 0; i < 3; ++i) { src.hi[i] = a.mag_hi[i]; src.sd[i] = a.mag_std[i]; }

    // 1. the rotation axes: the rows of orthMtx
    double O[3][3];
    range_normal<GIVEN>(src, a.seg[0], a.seg[1], O[0]);
    range_normal<GIVEN>(src, a.seg[2], a.seg[3], O[1]);
    range_normal<GIVEN>(src, a.seg[4], a.seg[5], O[2]);

    // 2. relative sensitivities (MagCalibration.c:118-152) and the moments of the rotated rows
    Moments mo;
    mo.clear();
    const double sZ2Y = range_ratio<GIVEN, 2, 1>(src, a.seg[0], a.seg[1], O, mo);
    const double sZ2X = range_ratio<GIVEN, 2, 0>(src, a.seg[2], a.seg[3], O, mo);
    const double sY2X = range_ratio<GIVEN, 1, 0>(src, a.seg[4], a.seg[5], O, mo);
    const double s[3] = {1.0, 1.0 / sY2X, (1.0 + sY2X * sY2X) / (sY2X * sY2X * sZ2X + sY2X * sZ2Y)};
    // soft_iron = diag(sens) . orthMtx, the full product
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        a.out_si[(0 + k) * runs + r] = s[0] * O[0][k] + 0.0 * O[1][k] + 0.0 * O[2][k];
        a.out_si[(3 + k) * runs + r] = 0.0 * O[0][k] + s[1] * O[1][k] + 0.0 * O[2][k];
        a.out_si[(6 + k) * runs + r] = 0.0 * O[0][k] + 0.0 * O[1][k] + s[2] * O[2][k];
    }

    // 3. the sphere through w = sens . u (MagCalibration.c:224-283): H^T H p = H^T B from the moments
    const double q[3] = {s[0] * s[0], s[1] * s[1], s[2] * s[2]};
    const double m2[3][3] = {{mo.s2[0], mo.s2[1], mo.s2[2]}, {mo.s2[1], mo.s2[3], mo.s2[4]}, {mo.s2[2], mo.s2[4], mo.s2[5]}};
    double H[4][4], g[4], p[4];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int k = 0; k < 3; ++k) H[i][k] = 4.0 * (s[i] * s[k] * m2[i][k]);
        H[i][3] = H[3][i] = 2.0 * (s[i] * mo.s1[i]);
        g[i] = 2.0 * (s[i] * (q[0] * mo.s3[i][0] + q[1] * mo.s3[i][1] + q[2] * mo.s3[i][2]));
    }
    H[3][3] = mo.cnt;
    g[3] = q[0] * mo.s2[0] + q[1] * mo.s2[3] + q[2] * mo.s2[5];
    solve<4>(H, g, p);
    a.out_hi[r] = p[0];
    a.out_hi[runs + r] = p[1];
    a.out_hi[2 * runs + r] = p[2];
    a.out_hi[3 * runs + r] = sqrt(p[3] + (p[0] * p[0] + p[1] * p[1] + p[2] * p[2]));

    if (a.out_cal) {    // wave-uniform
        const int64_t nx = a.seg[1] - a.seg[0], ny = a.seg[3] - a.seg[2], nz = a.seg[5] - a.seg[4], total = nx + ny + nz;
        double* out = a.out_cal + r;
        range_calibrated<GIVEN>(src, a.seg[0], a.seg[1], O, s, p, out, 0, total, runs);
        range_calibrated<GIVEN>(src, a.seg[2], a.seg[3], O, s, p, out, nx, total, runs);
        range_calibrated<GIVEN>(src, a.seg[4], a.seg[5], O, s, p, out, nx + ny, total, runs);
    }
}

hipError_t launch_magcal(const ginsim_magcal_params& p, hipStream_t stream) {
    const dim3 grid((unsigned)((p.runs + 255) / 256)), block(256);
    if (p.in_mag) hipLaunchKernelGGL((magcal_kernel<true>), grid, block, 0, stream, p);
    else hipLaunchKernelGGL((magcal_kernel<false>), grid, block, 0, stream, p);
    return hipGetLastError();
}

}  // namespace ginsim
