// What the kernels of the loosely coupled GPS/INS filter share (ins_loose.hip: loose_kernel; ins_loose_aided.hip:
// loose_aided_kernel): the covariance in LDS (Cov), its propagation, the GPS correction, the odometer / non-holonomic aiding block,
// the feedback both end with, and the time loop (loose_body), whose AID = false form is loose_kernel as it was; and, for
// ins_loose_cons.hip's loose_cons_kernel, the consistency checkpoint (loose_checkpoint) behind the flag CONS.  The account of
// the register budget that put P into LDS is in ins_loose.hip's header; the aiding block's equations are in ins_loose_aided.hip's.
// For ins_loose_mag.hip's loose_mag_kernel: the magnetometer block (loose_mag) behind the flag MAG; its equations are in that file's header.
// The covariance and everything that touches it is generic in the number of states NS (CovT<NS>; Cov = CovT<15> is the filter of the
// four files above).  ins_loose_scale.hip's loose_scale_kernel is the lane with NS = 16: state 15 is the odometer's scale-factor
// error; what it adds is behind `NS == kLooseStates + 1` and compiles to nothing for NS = 15.
// For ins_loose_still.hip's loose_still_kernel: the standstill block (loose_still) behind the flag STILL; its equations are in that
// file's header.
// For ins_loose_all.hip's loose_all_kernel: the three blocks above in one lane, each gated at run time; what it adds is behind
// `TL == Tail::ALL` (the layout of the kernel's fifth argument) and compiles to nothing for the six files above.
// For ins_loose_all_cons.hip's loose_all_cons_kernel: that lane with the checkpoint, and the checkpoint's three values of the
// scale-factor state behind `NS == kLooseStates + 1`; CONS with Tail::ONE is loose_cons_kernel's lane as it was.
#pragma once
#include <hip/hip_runtime.h>
#include "ginsim.h"
#include "ginsim_loose_all.h"
#include "ins_math.hpp"
#include "philox.hpp"
#include "sensor_synth.hpp"
#include "gps_synth.hpp"
#include "mag_synth.hpp"
#include "nav.hpp"

namespace ginsim {

constexpr int kLooseStates = 15;                                    // dr, dv, psi, dbg, dba: the states every filter has
constexpr int kLooseScaleStates = kLooseStates + 1;                 // and the odometer's scale-factor error, state 15
__host__ __device__ constexpr int loose_tri(int ns) { return ns * (ns + 1) / 2; }
constexpr int kLooseTri = loose_tri(kLooseStates);

// index of element (i, j) of the symmetric NS x NS matrix in its upper triangle, row by row
template <int NS = kLooseStates>
__host__ __device__ constexpr int tri(int i, int j) {
    return i <= j ? i * NS - i * (i - 1) / 2 + (j - i) : j * NS - j * (j - 1) / 2 + (i - j);
}
__host__ __device__ constexpr bool in_block(int k, int b) { return k >= b && k < b + 3; }
// Between the fully unrolled phases of a step: without a fence the scheduler interleaves them for instruction-level parallelism,
// which lengthens live ranges.  Build report of the form below (P in LDS): 0 bytes of scratch with and without the fences,
// 2-110 AGPRs (values parked outside the 256 VGPRs arithmetic can address) with them, 70-230 without.
__device__ __forceinline__ void phase_fence() { __builtin_amdgcn_sched_barrier(0); }

constexpr int kLooseBlock = 64;                                     // lanes per workgroup

// P lives in LDS as [element][lane] doubles, 120 x 64 per wavefront (60 KB: two single-wavefront workgroups per CU): a lane's
// column, no bank conflict, every byte offset a 16-bit immediate.  See the register budget in ins_loose.hip's header.
// With 16 states: 136 x 64 (68 KB; with the 8 KB of normal tables two workgroups are 152 KB of the CU's 160 KB).
__host__ __device__ constexpr size_t loose_cov_lds(int ns) { return sizeof(double) * loose_tri(ns) * kLooseBlock; }
constexpr size_t kLooseCovLds = loose_cov_lds(kLooseStates);
__device__ __forceinline__ double* cov_lds() {
    extern __shared__ double loose_lds[];
    return loose_lds;
}

constexpr int kAidFirst = 3, kAidSupport = 6;       // an aiding row is non-zero on dv and psi (states 3-8) only

template <int NS>
struct CovT {
    __device__ __forceinline__ double& at(int i, int j) { return cov_lds()[tri<NS>(i, j) * kLooseBlock + threadIdx.x]; }
    __device__ __forceinline__ double get(int i, int j) const { return cov_lds()[tri<NS>(i, j) * kLooseBlock + threadIdx.x]; }

    // P <- T P T^T, T = I + B E(I, J): block row I gains B times block row J (I != J), B a 3x3 matrix
    template <int I, int J>
    __device__ __forceinline__ void congruence(const double (&B)[3][3]) {
        double W[3][3], Y[3][3];        // W = B P_JI, Y = B P_JJ, both of the matrix as it is now
#pragma unroll
        for (int a = 0; a < 3; ++a) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                W[a][c] = B[a][0] * get(J, I + c) + B[a][1] * get(J + 1, I + c) + B[a][2] * get(J + 2, I + c);
                Y[a][c] = B[a][0] * get(J, J + c) + B[a][1] * get(J + 1, J + c) + B[a][2] * get(J + 2, J + c);
            }
        }
#pragma unroll
        for (int k = 0; k < NS; ++k) {
            if (in_block(k, I)) continue;
            const double t0 = get(J, k), t1 = get(J + 1, k), t2 = get(J + 2, k);
#pragma unroll
            for (int a = 0; a < 3; ++a) at(I + a, k) += B[a][0] * t0 + B[a][1] * t1 + B[a][2] * t2;
        }
#pragma unroll
        for (int a = 0; a < 3; ++a) {
#pragma unroll
            for (int c = a; c < 3; ++c)
                at(I + a, I + c) += W[a][c] + W[c][a] + (Y[a][0] * B[c][0] + Y[a][1] * B[c][1] + Y[a][2] * B[c][2]);
        }
    }
    // the same with B = s I
    template <int I, int J>
    __device__ __forceinline__ void congruence(double s) {
        double W[3][3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
#pragma unroll
            for (int c = 0; c < 3; ++c) W[a][c] = s * get(J + a, I + c);
        }
#pragma unroll
        for (int k = 0; k < NS; ++k) {
            if (in_block(k, I)) continue;
#pragma unroll
            for (int a = 0; a < 3; ++a) at(I + a, k) += s * get(J + a, k);
        }
#pragma unroll
        for (int a = 0; a < 3; ++a) {
#pragma unroll
            for (int c = a; c < 3; ++c) at(I + a, I + c) += W[a][c] + W[c][a] + (s * s) * get(J + a, J + c);
        }
    }
    // P <- D P D with D = diag(d) on block I, identity elsewhere
    template <int I>
    __device__ __forceinline__ void scale(const double (&d)[3]) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
#pragma unroll
            for (int k = 0; k < NS; ++k) {
                if (in_block(k, I)) continue;
                at(I + a, k) *= d[a];
            }
#pragma unroll
            for (int c = a; c < 3; ++c) at(I + a, I + c) *= d[a] * d[c];
        }
    }
    // block I gains C diag(q) C^T
    template <int I>
    __device__ __forceinline__ void add_rotated(const double (&C)[3][3], const double (&q)[3]) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
#pragma unroll
            for (int c = a; c < 3; ++c) at(I + a, I + c) += C[a][0] * q[0] * C[c][0] + C[a][1] * q[1] * C[c][1] + C[a][2] * q[2] * C[c][2];
        }
    }
    // scalar measurement of state I with variance rv and innovation-before-state z: x and P updated
    template <int I>
    __device__ __forceinline__ void update(double z, double rv, double (&x)[NS]) {
        double col[NS];
#pragma unroll
        for (int k = 0; k < NS; ++k) col[k] = get(k, I);
        const double inv = 1.0 / (col[I] + rv);
        const double g = (z - x[I]) * inv;
#pragma unroll
        for (int k = 0; k < NS; ++k) x[k] += col[k] * g;
#pragma unroll
        for (int a = 0; a < NS; ++a) {
#pragma unroll
            for (int c = a; c < NS; ++c) at(a, c) -= col[a] * col[c] * inv;
        }
    }
    // scalar measurement with the row h on states kAidFirst .. kAidFirst + 5 (zero elsewhere), variance rv and
    // innovation-before-state z: Ph = P h, s = h.Ph + rv, g = (z - h.x) / s, x += Ph g, P -= Ph Ph^T / s
    // LAST: the row has a seventh entry hl on the last state, NS - 1 (the odometer row of the scale-factor filter)
    template <bool LAST>
    __device__ __forceinline__ void update_row_impl(const double (&h)[kAidSupport], double hl, double z, double rv, double (&x)[NS]) {
        double ph[NS];
#pragma unroll
        for (int k = 0; k < NS; ++k) {
            double t = get(k, kAidFirst) * h[0];
#pragma unroll
            for (int c = 1; c < kAidSupport; ++c) t += get(k, kAidFirst + c) * h[c];
            if (LAST) t += get(k, NS - 1) * hl;
            ph[k] = t;
        }
        double s = rv, hx = 0.0;
#pragma unroll
        for (int c = 0; c < kAidSupport; ++c) { s += h[c] * ph[kAidFirst + c]; hx += h[c] * x[kAidFirst + c]; }
        if (LAST) { s += hl * ph[NS - 1]; hx += hl * x[NS - 1]; }
        const double inv = 1.0 / s;
        const double g = (z - hx) * inv;
#pragma unroll
        for (int k = 0; k < NS; ++k) x[k] += ph[k] * g;
#pragma unroll
        for (int a = 0; a < NS; ++a) {
#pragma unroll
            for (int c = a; c < NS; ++c) at(a, c) -= ph[a] * ph[c] * inv;
        }
    }
    __device__ __forceinline__ void update_row(const double (&h)[kAidSupport], double z, double rv, double (&x)[NS]) {
        update_row_impl<false>(h, 0.0, z, rv, x);
    }
    __device__ __forceinline__ void update_row(const double (&h)[kAidSupport], double hl, double z, double rv, double (&x)[NS]) {
        update_row_impl<true>(h, hl, z, rv, x);
    }
    // the same with the row h on the psi states 6-8 only (the magnetometer rows): three products per element of Ph
    // (not update_row_impl with another first column and width: under -ffp-contract=on the one expression below rounds the
    // product with h[1] and fuses the other two, the loop there rounds the product with h[0]; the kernel's bits would move)
    __device__ __forceinline__ void update_row_psi(const double (&h)[3], double z, double rv, double (&x)[NS]) {
        double ph[NS];
#pragma unroll
        for (int k = 0; k < NS; ++k) ph[k] = get(k, 6) * h[0] + get(k, 7) * h[1] + get(k, 8) * h[2];
        double s = rv, hx = 0.0;
#pragma unroll
        for (int c = 0; c < 3; ++c) { s += h[c] * ph[6 + c]; hx += h[c] * x[6 + c]; }
        const double inv = 1.0 / s;
        const double g = (z - hx) * inv;
#pragma unroll
        for (int k = 0; k < NS; ++k) x[k] += ph[k] * g;
#pragma unroll
        for (int a = 0; a < NS; ++a) {
#pragma unroll
            for (int c = a; c < NS; ++c) at(a, c) -= ph[a] * ph[c] * inv;
        }
    }
};
using Cov = CovT<kLooseStates>;

// C = body -> navigation of the attitude (the matrix of Att::to_nav)
__device__ __forceinline__ void body_to_nav(const Att& t, double (&C)[3][3]) {
    C[0][0] = t.cp * t.cy; C[0][1] = t.sr * t.sp * t.cy - t.cr * t.sy; C[0][2] = t.sp * t.cr * t.cy + t.sy * t.sr;
    C[1][0] = t.cp * t.sy; C[1][1] = t.sr * t.sp * t.sy + t.cr * t.cy; C[1][2] = t.sp * t.cr * t.sy - t.cy * t.sr;
    C[2][0] = -t.sp;       C[2][1] = t.cp * t.sr;                      C[2][2] = t.cp * t.cr;
}

typedef const ginsim_loose_params __attribute__((address_space(4))) * loose_ptr;
// the second by-value block follows the first in the kernarg segment (8-byte aligned structs)
__device__ __forceinline__ loose_ptr loose_params() {
    typedef const char __attribute__((address_space(4))) * bytes_ptr;
    bytes_ptr p = (bytes_ptr)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(p));
    return (loose_ptr)(p + sizeof(ginsim_mc_params));
}

// What the kernel's fifth argument is.  ONE: the block of one family (loose_mag_kernel, loose_scale_kernel, loose_still_kernel): every
// accessor below reads at the tail's start, and a lane has at most one of the three blocks.  ALL: a ginsim_loose_all_params
// (loose_all_kernel): the three blocks one after the other, each accessor at its member's offset.
enum class Tail { ONE, ALL };
constexpr size_t kLooseTailOffset = sizeof(ginsim_mc_params) + sizeof(ginsim_loose_params) + 2 * sizeof(void*);
static_assert(offsetof(ginsim_loose_all_params, mag) == 0 && offsetof(ginsim_loose_all_params, scale) == sizeof(ginsim_loose_mag_params) &&
              offsetof(ginsim_loose_all_params, still) == sizeof(ginsim_loose_mag_params) + sizeof(ginsim_loose_scale_params) &&
              sizeof(ginsim_loose_all_params) == sizeof(ginsim_loose_mag_params) + sizeof(ginsim_loose_scale_params) + sizeof(ginsim_loose_still_params),
              "ginsim_loose_all_params: the three blocks one after the other, no padding");
static_assert(kLooseTailOffset + sizeof(ginsim_loose_all_params) <= 4096, "the kernarg segment of loose_all_kernel: HIP's limit of 4 KB");

// The fifth argument of loose_mag_kernel, loose_scale_kernel and loose_still_kernel, the family's block T by value: it follows the
// two parameter blocks and the two pointers (stamp, visible) in the kernarg segment.  OFFSET: where T lies inside the argument
template <class T, size_t OFFSET = 0>
__device__ __forceinline__ const T __attribute__((address_space(4))) * loose_tail_params() {
    static_assert(sizeof(ginsim_mc_params) % 8 == 0 && sizeof(ginsim_loose_params) % 8 == 0 && alignof(T) == 8 && OFFSET % 8 == 0,
                  "the kernarg offsets of loose_params() / loose_tail_params()");
    typedef const char __attribute__((address_space(4))) * bytes_ptr;
    bytes_ptr p = (bytes_ptr)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(p));
    return (const T __attribute__((address_space(4))) *)(p + sizeof(ginsim_mc_params) + sizeof(ginsim_loose_params) + 2 * sizeof(void*) + OFFSET);
}
typedef const ginsim_loose_mag_params __attribute__((address_space(4))) * loose_mag_ptr;
typedef const ginsim_loose_scale_params __attribute__((address_space(4))) * loose_scale_ptr;
typedef const ginsim_loose_still_params __attribute__((address_space(4))) * loose_still_ptr;
template <Tail TL = Tail::ONE>
__device__ __forceinline__ loose_mag_ptr loose_mag_params() {
    return loose_tail_params<ginsim_loose_mag_params, TL == Tail::ALL ? offsetof(ginsim_loose_all_params, mag) : 0>();
}
template <Tail TL = Tail::ONE>
__device__ __forceinline__ loose_scale_ptr loose_scale_params() {
    return loose_tail_params<ginsim_loose_scale_params, TL == Tail::ALL ? offsetof(ginsim_loose_all_params, scale) : 0>();
}
template <Tail TL = Tail::ONE>
__device__ __forceinline__ loose_still_ptr loose_still_params() {
    return loose_tail_params<ginsim_loose_still_params, TL == Tail::ALL ? offsetof(ginsim_loose_all_params, still) : 0>();
}

// the standstill signal of sample j (wave-uniform: a scalar load, as visible[kf])
__device__ __forceinline__ bool still_flag(const int32_t* flags, int64_t j) {
    typedef const int32_t __attribute__((address_space(4))) * flags_ptr;
    return ((flags_ptr)(uintptr_t)flags)[j] != 0;
}

// P <- Phi P Phi^T + Qd for the step from the attitude with body -> navigation matrix C and bias-corrected specific force f^n
// (NS = 16: Phi is the identity on state 15, whose row takes part in every congruence as a column; P[15][15] += q_k)
template <Tail TL = Tail::ONE, int NS>
__device__ __forceinline__ void loose_propagate(CovT<NS>& P, const double (&C)[3][3], double fx, double fy, double fz, double dt) {
    const double A[3][3] = {{0.0, -fz * dt, fy * dt}, {fz * dt, 0.0, -fx * dt}, {-fy * dt, fx * dt, 0.0}};      // [f^n x] dt
    double Cp[3][3], Cm[3][3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
#pragma unroll
        for (int c = 0; c < 3; ++c) { Cp[a][c] = C[a][c] * dt; Cm[a][c] = -Cp[a][c]; }
    }
    P.template congruence<0, 3>(dt); phase_fence();         // T_r
    P.template congruence<3, 6>(A); phase_fence();          // T_v
    P.template congruence<3, 12>(Cm); phase_fence();
    P.template congruence<6, 9>(Cp); phase_fence();         // T_psi
    const loose_ptr lp = loose_params();
    const double dg[3] = {lp->decay_g[0], lp->decay_g[1], lp->decay_g[2]}, da[3] = {lp->decay_a[0], lp->decay_a[1], lp->decay_a[2]};
    P.template scale<9>(dg); phase_fence();                 // D
    P.template scale<12>(da); phase_fence();
    const double qv[3] = {lp->q_v[0], lp->q_v[1], lp->q_v[2]}, qp[3] = {lp->q_psi[0], lp->q_psi[1], lp->q_psi[2]};
    P.template add_rotated<3>(C, qv); phase_fence();
    P.template add_rotated<6>(C, qp); phase_fence();
#pragma unroll
    for (int a = 0; a < 3; ++a) { P.at(9 + a, 9 + a) += lp->q_bg[a]; P.at(12 + a, 12 + a) += lp->q_ba[a]; }
    if (NS == kLooseScaleStates) P.at(kLooseStates, kLooseStates) += loose_scale_params<TL>()->q_k;
}

// The feedback of the error state x into the mechanisation and the bias estimates (truth = estimate - error).  mlat, mlon:
// metres per radian of latitude / longitude at the state before the feedback (ref_frame 0).  x[15] of the scale-factor filter is
// fed back by the caller (k_est -= x[15])
template <int RF, int NS>
__device__ __forceinline__ void loose_feedback(Nav& s, Vec3& bg, Vec3& ba, const double (&x)[NS], double mlat, double mlon) {
    if (RF == 0) {
        s.pos.x -= x[0] / mlat;
        s.pos.y -= x[1] / mlon;
        s.pos.z += x[2];
        sincos(s.pos.x, &s.sl, &s.cl);
    } else {
        s.pos.x -= x[0]; s.pos.y -= x[1]; s.pos.z -= x[2];
    }
    s.vel.x -= x[3]; s.vel.y -= x[4]; s.vel.z -= x[5];
    // C <- (I + [psi x]) C_est; the n -> b matrix D = C^T becomes D (I - [psi x]); Euler angles from its rows by atan2 (the
    // first-order rotation scales a row by 1 + O(psi^2), which the quotients do not see)
    double C[3][3];
    body_to_nav(s.att, C);
    const double px = x[6], py = x[7], pz = x[8];
    // rows of D' = columns of C' = (I + [psi x]) C:  C'[i][k] = C[i][k] + (psi x C[:,k])[i]
    const double d00 = C[0][0] + (py * C[2][0] - pz * C[1][0]);
    const double d01 = C[1][0] + (pz * C[0][0] - px * C[2][0]);
    const double d02 = C[2][0] + (px * C[1][0] - py * C[0][0]);
    const double d12 = C[2][1] + (px * C[1][1] - py * C[0][1]);
    const double d22 = C[2][2] + (px * C[1][2] - py * C[0][2]);
    s.att.set(atan2(d01, d00), atan2(-d02, sqrt(d00 * d00 + d01 * d01)), atan2(d12, d22));
    if (RF == 1) s.vb = s.att.to_body(s.vel);
    bg.x -= x[9]; bg.y -= x[10]; bg.z -= x[11];
    ba.x -= x[12]; ba.y -= x[13]; ba.z -= x[14];
}

// One fix: six scalar updates, then the feedback.  kest: the scale-factor estimate (NS = 16; not touched otherwise)
template <int RF, int NS>
__device__ __forceinline__ void loose_correct(CovT<NS>& P, Nav& s, Vec3& bg, Vec3& ba, const double (&fix)[6], double& kest) {
    const loose_ptr lp = loose_params();
    double z[6], mlat = 1.0, mlon = 1.0;
    if (RF == 0) {          // LLA difference -> NED metres
        const Geo e = geo_param_sc(s.sl, s.cl, s.pos.z);
        mlat = e.rm + s.pos.z;
        mlon = (e.rn + s.pos.z) * e.cl;
        z[0] = (s.pos.x - fix[0]) * mlat;
        z[1] = (s.pos.y - fix[1]) * mlon;
        z[2] = -(s.pos.z - fix[2]);
    } else {
        z[0] = s.pos.x - fix[0]; z[1] = s.pos.y - fix[1]; z[2] = s.pos.z - fix[2];
    }
    z[3] = s.vel.x - fix[3]; z[4] = s.vel.y - fix[4]; z[5] = s.vel.z - fix[5];
    double x[NS];
#pragma unroll
    for (int k = 0; k < NS; ++k) x[k] = 0.0;
    P.template update<0>(z[0], lp->r_diag[0], x); phase_fence();
    P.template update<1>(z[1], lp->r_diag[1], x); phase_fence();
    P.template update<2>(z[2], lp->r_diag[2], x); phase_fence();
    P.template update<3>(z[3], lp->r_diag[3], x); phase_fence();
    P.template update<4>(z[4], lp->r_diag[4], x); phase_fence();
    P.template update<5>(z[5], lp->r_diag[5], x); phase_fence();
    loose_feedback<RF>(s, bg, ba, x, mlat, mlon);
    if (NS == kLooseScaleStates) kest -= x[NS - 1];
}

// One aiding block (ins_loose_aided.hip's header): the rows `mask` selects, in ascending order, from x = 0; then the feedback.
// D = C^T, v_b = D v and every row are formed from the state before the first row.  mask is wave-uniform.
// NS = 16: the odometer is divided by the estimate kest, not by odo_scale_f, and its row has the seventh entry
// h[15] = v_b[0] / kest; the block ends with kest -= x[15].  kest is not touched otherwise.
template <int RF, int NS>
__device__ __forceinline__ void loose_aid(CovT<NS>& P, Nav& s, Vec3& bg, Vec3& ba, double odo, int mask, double& kest) {
    const loose_ptr lp = loose_params();
    double C[3][3];
    body_to_nav(s.att, C);
    const double v[3] = {s.vel.x, s.vel.y, s.vel.z};
    double h[3][kAidSupport], z[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {               // row i of D is column i of C; the psi part is -(D [v x])[i,:] = v x D[i,:]
        const double d0 = C[0][i], d1 = C[1][i], d2 = C[2][i];
        h[i][0] = d0; h[i][1] = d1; h[i][2] = d2;
        h[i][3] = v[1] * d2 - v[2] * d1;
        h[i][4] = v[2] * d0 - v[0] * d2;
        h[i][5] = v[0] * d1 - v[1] * d0;
        z[i] = d0 * v[0] + d1 * v[1] + d2 * v[2];
    }
    double hk = 0.0;
    if (NS == kLooseScaleStates) {
        hk = z[0] / kest;
        z[0] -= odo / kest;
    } else {
        z[0] -= odo / lp->odo_scale_f;
    }
    double mlat = 1.0, mlon = 1.0;
    if (RF == 0) {
        const Geo e = geo_param_sc(s.sl, s.cl, s.pos.z);
        mlat = e.rm + s.pos.z;
        mlon = (e.rn + s.pos.z) * e.cl;
    }
    double x[NS];
#pragma unroll
    for (int k = 0; k < NS; ++k) x[k] = 0.0;
    phase_fence();
    if (mask & 1) {
        if (NS == kLooseScaleStates) P.update_row(h[0], hk, z[0], lp->r_odo, x);
        else P.update_row(h[0], z[0], lp->r_odo, x);
        phase_fence();
    }
    if (mask & 2) { P.update_row(h[1], z[1], lp->r_nhc, x); phase_fence(); }
    if (mask & 4) { P.update_row(h[2], z[2], lp->r_nhc, x); phase_fence(); }
    loose_feedback<RF>(s, bg, ba, x, mlat, mlon);
    if (NS == kLooseScaleStates) kest -= x[NS - 1];
}

// One magnetometer block (ins_loose_mag.hip's header): the three rows in ascending order from x = 0; then the feedback.
// D = C^T, z and every row are formed from the state before the first row.  mag: the raw sample of this lane.
// NS = 16: the rows have h[15] = 0 (update_row_psi over 16 states) and the block ends with kest -= x[15], as loose_aid.
template <int RF, Tail TL = Tail::ONE, int NS>
__device__ __forceinline__ void loose_mag(CovT<NS>& P, Nav& s, Vec3& bg, Vec3& ba, const double (&mag)[3], double& kest) {
    const loose_mag_ptr mp = loose_mag_params<TL>();
    double C[3][3];
    body_to_nav(s.att, C);
    const double m[3] = {mp->mag_n[0], mp->mag_n[1], mp->mag_n[2]};
    double h[3][3], z[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {               // row i of D is column i of C; the psi part is -(D [m x])[i,:] = m x D[i,:]
        const double d0 = C[0][i], d1 = C[1][i], d2 = C[2][i];
        h[i][0] = m[1] * d2 - m[2] * d1;
        h[i][1] = m[2] * d0 - m[0] * d2;
        h[i][2] = m[0] * d1 - m[1] * d0;
        const double cal = mp->cal_si[3 * i] * mag[0] + mp->cal_si[3 * i + 1] * mag[1] + mp->cal_si[3 * i + 2] * mag[2] - mp->cal_hi[i];
        z[i] = (d0 * m[0] + d1 * m[1] + d2 * m[2]) - cal;
    }
    double mlat = 1.0, mlon = 1.0;
    if (RF == 0) {
        const Geo e = geo_param_sc(s.sl, s.cl, s.pos.z);
        mlat = e.rm + s.pos.z;
        mlon = (e.rn + s.pos.z) * e.cl;
    }
    double x[NS];
#pragma unroll
    for (int k = 0; k < NS; ++k) x[k] = 0.0;
    phase_fence();
    P.update_row_psi(h[0], z[0], loose_mag_params<TL>()->r_mag[0], x); phase_fence();
    P.update_row_psi(h[1], z[1], loose_mag_params<TL>()->r_mag[1], x); phase_fence();
    P.update_row_psi(h[2], z[2], loose_mag_params<TL>()->r_mag[2], x); phase_fence();
    loose_feedback<RF>(s, bg, ba, x, mlat, mlon);
    if (NS == kLooseScaleStates) kest -= x[NS - 1];
}

// One standstill block (ins_loose_still.hip's header): the rows `mask` selects (bit 0: dv, states 3-5; bit 1: dbg, states 9-11) in
// ascending state order from x = 0; then the feedback.  Every z is formed from the state before the first row.  gyro_prev: the raw
// gyro sample the lane integrated last (j - 1), before the bias was subtracted.  mask is wave-uniform.
// NS = 16: every row observes one of the first 15 states (h[15] = 0) and the block ends with kest -= x[15], as loose_aid.
template <int RF, Tail TL = Tail::ONE, int NS>
__device__ __forceinline__ void loose_still(CovT<NS>& P, Nav& s, Vec3& bg, Vec3& ba, const Vec3& gyro_prev, int mask, double& kest) {
    // the rate the mechanisation assumes of a body at rest (nav_step with v = 0): earth rate in the body axes of the estimate
    Vec3 wr{0.0, 0.0, 0.0};
    if (RF == 0) {
        if (kernarg_params()->earth_rot) wr = s.att.to_body(Vec3{kWie * s.cl, 0.0, -kWie * s.sl});
    }
    const double zv[3] = {s.vel.x, s.vel.y, s.vel.z};
    const double zg[3] = {bg.x + wr.x - gyro_prev.x, bg.y + wr.y - gyro_prev.y, bg.z + wr.z - gyro_prev.z};
    double mlat = 1.0, mlon = 1.0;
    if (RF == 0) {
        const Geo e = geo_param_sc(s.sl, s.cl, s.pos.z);
        mlat = e.rm + s.pos.z;
        mlon = (e.rn + s.pos.z) * e.cl;
    }
    double x[NS];
#pragma unroll
    for (int k = 0; k < NS; ++k) x[k] = 0.0;
    phase_fence();
    if (mask & 1) {
        P.template update<3>(zv[0], loose_still_params<TL>()->r_zupt, x); phase_fence();
        P.template update<4>(zv[1], loose_still_params<TL>()->r_zupt, x); phase_fence();
        P.template update<5>(zv[2], loose_still_params<TL>()->r_zupt, x); phase_fence();
    }
    if (mask & 2) {
        P.template update<9>(zg[0], loose_still_params<TL>()->r_zaru[0], x); phase_fence();
        P.template update<10>(zg[1], loose_still_params<TL>()->r_zaru[1], x); phase_fence();
        P.template update<11>(zg[2], loose_still_params<TL>()->r_zaru[2], x); phase_fence();
    }
    loose_feedback<RF>(s, bg, ba, x, mlat, mlon);
    if (NS == kLooseScaleStates) kest -= x[NS - 1];
}

// ---- consistency checkpoints (ins_loose_cons.hip)
// What loose_cons_kernel passes to the lane next to the two parameter blocks: the DEVICE copy of the checkpoint samples, their
// number and the wavefronts' partial records [wave][checkpoint][GINSIM_CONS_RECORD].  Not read unless CONS.
struct ConsArgs {
    const int64_t* sample = nullptr;
    int64_t m = 0;
    double* work = nullptr;
};

// the sum of v over the 64 lanes, in every lane: a 6-level butterfly whose order does not depend on the data
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int d = 1; d < kLooseBlock; d <<= 1) v += __shfl_xor(v, d, kLooseBlock);
    return v;
}

// e^T B^-1 e of the symmetric 3x3 block I of P by its adjugate and determinant; NaN unless the block is positive definite
// (Sylvester: the three leading minors)
template <int I, int NS>
__device__ __forceinline__ double block_nees(const CovT<NS>& P, const double* e) {
    const double a = P.get(I, I), b = P.get(I, I + 1), c = P.get(I, I + 2), d = P.get(I + 1, I + 1), f = P.get(I + 1, I + 2), g = P.get(I + 2, I + 2);
    const double a00 = d * g - f * f, a01 = c * f - b * g, a02 = b * f - c * d;
    const double a11 = a * g - c * c, a12 = b * c - a * f, a22 = a * d - b * b;
    const double det = a * a00 + b * a01 + c * a02;
    const double q = (e[0] * e[0] * a00 + e[1] * e[1] * a11 + e[2] * e[2] * a22) + 2.0 * (e[0] * e[1] * a01 + e[0] * e[2] * a02 + e[1] * e[2] * a12);
    return (a > 0.0 && a22 > 0.0 && det > 0.0) ? q / det : __builtin_nan("");
}

// One checkpoint: the lane's error state against the truth row t (att3, pos3, vel3) in the filter's own coordinates
// (tests/ins_loose_ref.py, error_state), the record's values of this lane, their sums over the wavefront, and lane 0's store of
// the partial record.  live: the lane carries a run of its own (a tail lane repeats the last run with weight 0).  Every lane of
// the wavefront arrives here together (the checkpoints are wave-uniform).
// NS = 16 (loose_all_cons_kernel): the record's slots 37-39 carry the scale state: P[15][15], and against the truth
// ktrue[r] of run r the error kest - ktrue[r], squared and over P[15][15].  ktrue == NULL (wave-uniform): the two error sums are
// written 0 and the scale error takes no part in a lane's inclusion.  NS = 15 is the checkpoint as it was.
template <int RF, int NS>
__device__ __forceinline__ void loose_checkpoint(const CovT<NS>& P, const Nav& s, uniform_ptr t, bool live, double* __restrict__ rec,
                                                 double kest = 0.0, const double* __restrict__ ktrue = nullptr, int64_t r = 0) {
    double e[9];
    if (RF == 0) {
        const Geo g = geo_param(t[3], t[5]);
        e[0] = (s.pos.x - t[3]) * (g.rm + t[5]);
        e[1] = (s.pos.y - t[4]) * (g.rn + t[5]) * g.cl;
        e[2] = -(s.pos.z - t[5]);
    } else {
        e[0] = s.pos.x - t[3]; e[1] = s.pos.y - t[4]; e[2] = s.pos.z - t[5];
    }
    e[3] = s.vel.x - t[6]; e[4] = s.vel.y - t[7]; e[5] = s.vel.z - t[8];
    {   // [psi x] = I - C_est C^T, both body -> navigation; psi from its antisymmetric part
        Att ta;
        ta.set(t[0], t[1], t[2]);
        double Ce[3][3], Ct[3][3];
        body_to_nav(s.att, Ce);
        body_to_nav(ta, Ct);
        const double m12 = Ce[1][0] * Ct[2][0] + Ce[1][1] * Ct[2][1] + Ce[1][2] * Ct[2][2];
        const double m21 = Ce[2][0] * Ct[1][0] + Ce[2][1] * Ct[1][1] + Ce[2][2] * Ct[1][2];
        const double m20 = Ce[2][0] * Ct[0][0] + Ce[2][1] * Ct[0][1] + Ce[2][2] * Ct[0][2];
        const double m02 = Ce[0][0] * Ct[2][0] + Ce[0][1] * Ct[2][1] + Ce[0][2] * Ct[2][2];
        const double m01 = Ce[0][0] * Ct[1][0] + Ce[0][1] * Ct[1][1] + Ce[0][2] * Ct[1][2];
        const double m10 = Ce[1][0] * Ct[0][0] + Ce[1][1] * Ct[0][1] + Ce[1][2] * Ct[0][2];
        e[6] = 0.5 * (m12 - m21);
        e[7] = 0.5 * (m20 - m02);
        e[8] = 0.5 * (m01 - m10);
    }
    phase_fence();
    const double nees[3] = {block_nees<0>(P, e), block_nees<3>(P, e + 3), block_nees<6>(P, e + 6)};
    // is the lane included?  every value finite, every P_kk > 0, every block positive definite (block_nees)
    bool ok = live;
#pragma unroll
    for (int k = 0; k < kLooseStates; ++k) {
        const double pk = P.get(k, k);
        ok = ok && pk > 0.0 && isfinite(pk);
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        const double e2 = e[k] * e[k], q = e2 / P.get(k, k);
        ok = ok && isfinite(e2) && isfinite(q);
    }
#pragma unroll
    for (int b = 0; b < 3; ++b) ok = ok && isfinite(nees[b]);
    double ek2 = 0.0;       // (kest - ktrue[r])^2, 0 without a truth (NS = 16 only)
    if constexpr (NS == kLooseScaleStates) {
        const double pk = P.get(kLooseStates, kLooseStates);
        ok = ok && pk > 0.0 && isfinite(pk);
        if (ktrue) {
            const double ek = kest - ktrue[r];
            ek2 = ek * ek;
            ok = ok && isfinite(ek2) && isfinite(ek2 / pk);
        }
    }
    phase_fence();
    // one value at a time: made again from e and the lane's column of P, summed, stored -- nothing of the record stays in registers
    const bool first = threadIdx.x == 0;
    const double cnt = wave_sum(ok ? 1.0 : 0.0);
    if (first) rec[0] = cnt;
#pragma unroll
    for (int k = 0; k < kLooseStates; ++k) {
        const double v = wave_sum(ok ? P.get(k, k) : 0.0);
        if (first) rec[1 + k] = v;
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        const double e2 = e[k] * e[k];
        const double v = wave_sum(ok ? e2 : 0.0), w = wave_sum(ok ? e2 / P.get(k, k) : 0.0);
        if (first) { rec[16 + k] = v; rec[25 + k] = w; }
    }
#pragma unroll
    for (int b = 0; b < 3; ++b) {
        const double v = wave_sum(ok ? nees[b] : 0.0);
        if (first) rec[34 + b] = v;
    }
    if constexpr (NS == kLooseScaleStates) {
        const double pk = P.get(kLooseStates, kLooseStates);
        const double u = wave_sum(ok ? pk : 0.0), v = wave_sum(ok ? ek2 : 0.0), w = wave_sum(ok && ktrue ? ek2 / pk : 0.0);
        if (first) { rec[37] = u; rec[38] = v; rec[39] = w; }
    }
    if (first) {
#pragma unroll
        for (int k = NS == kLooseScaleStates ? 40 : 37; k < GINSIM_CONS_RECORD; ++k) rec[k] = 0.0;
    }
}

__device__ __forceinline__ void put3(double* base, int64_t plane, int64_t off, const Vec3& v) {
    if (base) store3(base, plane, off, v);
}

// The whole lane: RF: ref_frame.  GIVEN: samples from in_accel / in_gyro (/ in_odo), fixes from in_gps.  VIB: the generated sensors
// carry a vibration term.  PS: online process-error statistics (out_proc).  AID: the aiding block (aid_mask != 0) at every sample
// j > 0 with j % aid_every == 0, after a fix of the same sample and before the row is stored.  ntab: the kernel's static LDS for
// the normal tables.  CONS: consistency checkpoints (loose_checkpoint) at the samples cq.sample[0 .. cq.m), on the state that row j reports:
// after a fix and an aiding block of the same sample, before the row is stored.  CONS = false is the lane as it was.
// MAG: the magnetometer block (loose_mag) at every sample j > 0 with j % mag_every == 0, after a fix and an aiding block of the same
// sample, before a checkpoint and before the row is stored; its numbers are the kernel's fifth argument (loose_mag_params).  With
// MAG an aid_mask of 0 fires no aiding block at all.  MAG = false is the lane as it was.
// NS: the number of states.  16 (with AID; without CONS and MAG unless TL is Tail::ALL): the odometer's scale factor is state 15 and its estimate kest a
// value of the lane; its numbers and outputs are the kernel's fifth argument (loose_scale_params).  NS = 15 is the lane as it was.
// STILL: the standstill block (loose_still) at every sample j > 0 with j % still_every == 0 and still_flags[j] != 0, after a fix and an
// aiding block of the same sample, before the row is stored (the magnetometer block's place; with AID, and unless TL is Tail::ALL without CONS and MAG, NS = 15);
// its numbers are the kernel's fifth argument (loose_still_params).  The lane carries the raw gyro sample it integrated last.  With
// STILL an aid_mask of 0 fires no aiding block at all.  STILL = false is the lane as it was.
// TL: the layout of the kernel's fifth argument (Tail).  ALL (loose_all_kernel, with AID, MAG and STILL, NS 15 or 16): the lane may have
// the three blocks together, each gated at run time: a magnetometer block with mag_every == 0 and a standstill block with
// still_mask == 0 never fire and none of their pointers is read.  TL = Tail::ONE is the lane as it was.
// CONS with Tail::ALL (loose_all_cons_kernel, ins_loose_all_cons.hpp): the checkpoint after the standstill block, on 15 or 16 states;
// ktrue: the scale factor's truth per run for the record's slots 38 and 39, or NULL (loose_checkpoint).  Not read otherwise.
template <int RF, bool GIVEN, bool VIB, bool PS, bool AID, bool CONS = false, bool MAG = false, int NS = kLooseStates, bool STILL = false,
          Tail TL = Tail::ONE>
__device__ __forceinline__ void loose_body(const ginsim_mc_params& a, const ginsim_loose_params& b, const int64_t* __restrict__ stamp,
                                           const int32_t* __restrict__ visible, uint32_t* ntab, const ConsArgs& cq = ConsArgs{},
                                           const double* __restrict__ ktrue = nullptr) {
    static_assert(NS == kLooseStates || (NS == kLooseScaleStates && AID && (!CONS || TL == Tail::ALL)),
                  "16 states: the aided lane, with checkpoints in the combined lane only");
    static_assert(!STILL || (AID && (!CONS || TL == Tail::ALL)), "the standstill block: the aided lane, with checkpoints in the combined lane only");
    static_assert(!CONS || (!MAG && !STILL && NS == kLooseStates && TL == Tail::ONE) || (AID && MAG && STILL && !PS && TL == Tail::ALL),
                  "checkpoints: no other block, or the combined lane with all of them");
    static_assert(TL == Tail::ALL || int(MAG) + int(STILL) + int(NS == kLooseScaleStates) <= 1,
                  "one family's block as the fifth argument: the lane has at most one of the three");
    NormalTables tab{};
    if (!GIVEN) {
        tab = fill_normal_tables(ntab, threadIdx.x, blockDim.x);
        __syncthreads();
    }
    int64_t lane = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = lane < b.n_list;
    if (CONS) {
        // the cross-lane sums of a checkpoint need all 64 lanes in the loop: a tail lane filters the last run of the list again
        // (it stores that run's own bits a second time) and enters every sum with weight 0
        if (!live) lane = b.n_list - 1;
    } else if (!live) {
        return;
    }
    const int64_t r = b.run_list ? b.run_list[lane] : lane;
    // Tail::ALL: n and runs through kernarg_params(), a load of their own.  Read from `a` they are part of one eight-dword scalar load
    // of the block's head that lives across the loop; in loose_all_kernel<0, false, true, false, NS> the allocator gave that octet a
    // spill slot before it chose to load it again instead, and the slot, never written, stayed as 36 bytes of scratch per lane
    const int64_t n = TL == Tail::ALL ? kernarg_params()->n : a.n, runs = TL == Tail::ALL ? kernarg_params()->runs : a.runs;
    const int64_t plane = n * runs, m = b.m;
    const double dt = 1.0 / a.fs;

    const uint64_t call = a.ini_first + (uint64_t)r;
    const double* ini = a.ini + 10 * (call < (uint64_t)a.n_ini ? call : 0);
    Nav s;
    nav_init<RF>(s, ini, a.ini_has_g);
    const uint64_t grun = a.run_offset + (uint64_t)r;
    const RngKey key{(uint32_t)a.seed, (uint32_t)(a.seed >> 32), (uint32_t)grun, (uint32_t)(grun >> 32)};
    Vec3 da{0.0, 0.0, 0.0}, dg{0.0, 0.0, 0.0}, vpa{0.0, 0.0, 0.0}, vpg{0.0, 0.0, 0.0};
    const Vec3 nopsd{0.0, 0.0, 0.0};
    if (VIB) {
        vpa = vibration_phase<S_ACC_VIB_PHASE>(&kernarg_params()->vib_accel, key);
        vpg = vibration_phase<S_GYR_VIB_PHASE>(&kernarg_params()->vib_gyro, key);
    }
    MathConsts mk;
    mk.init<false>();
    Vec3 bg{0.0, 0.0, 0.0}, ba{0.0, 0.0, 0.0};
    CovT<NS> P;
#pragma unroll
    for (int i = 0; i < kLooseStates; ++i) {
#pragma unroll
        for (int k = i; k < NS; ++k) P.at(i, k) = i == k ? b.p0[i / 3] * b.p0[i / 3] : 0.0;
    }
    double kest = 0.0;      // the scale-factor estimate (NS = 16 only)
    if (NS == kLooseScaleStates) {
        const loose_scale_ptr sp = loose_scale_params<TL>();
        kest = sp->scale0;
        P.at(kLooseStates, kLooseStates) = sp->p0_scale * sp->p0_scale;
    }
    Proc<1> ps;
    if (PS) ps.clear();
    const uniform_ptr nav_truth = as_uniform(a.ref_nav);
    const bool ned = a.proc_pos_ned != 0;
    int64_t kf = 0;         // the next fix (wave-uniform)
    // the next aiding block (wave-uniform); a period of n or more never fires
    const int64_t every = AID ? ((b.aid_every < n && !((MAG || STILL) && b.aid_mask == 0)) ? b.aid_every : n) : 0;
    int64_t ja = every;
    // the next magnetometer block (wave-uniform), a counter of its own; a period of n or more never fires
    // (the period is read again from the kernarg segment at every block: one wave-uniform counter is all the loop holds)
    int64_t jm = MAG ? (loose_mag_params<TL>()->mag_every < n ? loose_mag_params<TL>()->mag_every : n) : 0;
    if constexpr (MAG && TL == Tail::ALL) jm = jm < 1 ? n : jm;     // an absent block (mag_every == 0)
    int64_t kc = 0;         // the next checkpoint (wave-uniform)
    // the next sample at which a standstill block can fire (wave-uniform), a counter of its own as jm; and the raw gyro sample the
    // lane integrated last (STILL only: nothing reads it otherwise)
    int64_t js = STILL ? (loose_still_params<TL>()->still_every < n ? loose_still_params<TL>()->still_every : n) : 0;
    if constexpr (STILL && TL == Tail::ALL) js = loose_still_params<TL>()->still_mask == 0 ? n : js;        // an absent block
    Vec3 gyro_prev{0.0, 0.0, 0.0};

    for (int64_t j = 0; j < n; ++j) {
        const int64_t off = j * runs + r;
        // pointers and sizes are re-read from the kernarg segment where they are used (scalar loads): held in SGPRs for the whole
        // loop they overflow the SGPR file (sensor_synth.hpp, kernarg_params)
        const loose_ptr lb = loose_params();
        const params_ptr ka = kernarg_params();
        if (kf < m && stamp[kf] == j) {
            if (!visible || visible[kf] != 0) {
                double fix[6];
                if (GIVEN) {
#pragma unroll
                    for (int c = 0; c < 6; ++c) fix[c] = lb->in_gps[(c * m + kf) * runs + r];
                } else {
                    gps_fix(as_uniform(lb->ref_gps) + 6 * kf, loose_params()->gps_sigma, key, (uint32_t)kf, tab, fix);
                }
                loose_correct<RF>(P, s, bg, ba, fix, kest);
            }
            ++kf;
        }
        if (AID) {
            if (j == ja) {
                ja += every;
                const int mask = lb->aid_mask;
                double odo = 0.0;
                if (mask & 1) {
                    if (GIVEN) {
                        odo = ka->in_odo[off];
                    } else {            // the sample ginsim_mc_run stores in out_odo (mc_kernel.hip, pathgen.py:639-640)
                        double z0, z1;
                        normal_pair(key, S_ODO, (uint32_t)j, z0, z1, tab);
                        const params_ptr kq = kernarg_params();
                        odo = kq->odo_scale * as_uniform(kq->ref_odo)[j] + kq->odo_stdv * z0;
                    }
                }
                phase_fence();
                loose_aid<RF>(P, s, bg, ba, odo, mask, kest);
                phase_fence();
            }
        }
        if constexpr (MAG) {
            if (j == jm) {
                const loose_mag_ptr mp = loose_mag_params<TL>();
                jm += mp->mag_every < n ? mp->mag_every : n;
                double mag[3];
                if (GIVEN) {
#pragma unroll
                    for (int c = 0; c < 3; ++c) mag[c] = mp->in_mag[(c * n + j) * runs + r];
                } else {                // the sample ginsim_aux_sensors stores in out_mag (aux_sensors.hip, mag_synth.hpp)
                    double z[3];
                    mag_normals(key, (uint32_t)j, tab, z);
                    const uniform_ptr rm = as_uniform(mp->ref_mag);
                    const double v[3] = {rm[3 * j] + mp->mag_hi[0], rm[3 * j + 1] + mp->mag_hi[1], rm[3 * j + 2] + mp->mag_hi[2]};
#pragma unroll
                    for (int c = 0; c < 3; ++c) mag[c] = mag_axis(mp->mag_si + 3 * c, v, mp->mag_std[c], z[c]);
                }
                phase_fence();
                loose_mag<RF, TL>(P, s, bg, ba, mag, kest);
                phase_fence();
            }
        }
        if constexpr (STILL) {
            if (j == js) {
                const loose_still_ptr sp = loose_still_params<TL>();
                js += sp->still_every < n ? sp->still_every : n;
                if (still_flag(sp->still_flags, j)) {
                    phase_fence();
                    loose_still<RF, TL>(P, s, bg, ba, gyro_prev, sp->still_mask, kest);
                    phase_fence();
                }
            }
        }
        if constexpr (CONS) {
            if (kc < cq.m && cq.sample[kc] == j) {
                phase_fence();
                loose_checkpoint<RF>(P, s, nav_truth + 9 * j, live, cq.work + ((int64_t)blockIdx.x * cq.m + kc) * GINSIM_CONS_RECORD, kest, ktrue, r);
                phase_fence();
                ++kc;
            }
        }
        if (lb->out_traj) store9(lb->out_traj, plane, off, s);
        put3(lb->out_wb, plane, off, bg);
        put3(lb->out_ab, plane, off, ba);
        if (NS == kLooseScaleStates) {
            double* const ks = loose_scale_params<TL>()->out_scale;
            if (ks) ks[off] = kest;
        }
        if (PS) {
            if (j >= ka->proc_first) {
                const uniform_ptr q = nav_truth + 9 * j;
                const double t[9] = {q[0], q[1], q[2], q[3], q[4], q[5], q[6], q[7], q[8]};
                if (RF == 0 && ned) ps.template add<true>(s, t, j == ka->proc_first, nav_truth);
                else ps.template add<false>(s, t, j == ka->proc_first, nav_truth);
            }
        }
        if (j == n - 1) break;
        Vec3 acc, gyr;
        if (GIVEN) {
            acc = Vec3{ka->in_accel[off], ka->in_accel[plane + off], ka->in_accel[2 * plane + off]};
            gyr = Vec3{ka->in_gyro[off], ka->in_gyro[plane + off], ka->in_gyro[2 * plane + off]};
        } else {
            const uint32_t jj = (uint32_t)j;
            const Vec3 cur_a = load3(as_uniform(ka->ref_accel), j), cur_g = load3(as_uniform(ka->ref_gyro), j);
            // the six streams of mc_kernel's one batch in two halves (the same normals): half the registers in flight
            {
                double z0[3], z1[3];
                normal_pairs<S_ACC_D_XY, 3>(key, jj, z0, z1, tab);
                acc = sense3<true>(cur_a, &kernarg_params()->accel, da, Vec3{z0[0], z1[0], z0[1]}, Vec3{z1[1], z0[2], z1[2]});
            }
            phase_fence();
            {
                double z0[3], z1[3];
                normal_pairs<S_GYR_D_XY, 3>(key, jj, z0, z1, tab);
                gyr = sense3<true>(cur_g, &kernarg_params()->gyro, dg, Vec3{z0[0], z1[0], z0[1]}, Vec3{z1[1], z0[2], z1[2]});
            }
            phase_fence();
            if (VIB) {
                acc = add_vibration<S_ACC_VIB_XY>(acc, &kernarg_params()->vib_accel, key, jj, tab, vpa, nopsd);
                gyr = add_vibration<S_GYR_VIB_XY>(gyr, &kernarg_params()->vib_gyro, key, jj, tab, vpg, nopsd);
            }
        }
        if constexpr (STILL) gyro_prev = gyr;       // raw: before the bias is subtracted
        acc = Vec3{acc.x - ba.x, acc.y - ba.y, acc.z - ba.z};
        gyr = Vec3{gyr.x - bg.x, gyr.y - bg.y, gyr.z - bg.z};
        // what the propagation needs of the state BEFORE the step: C and f^n = C f
        double C[3][3];
        body_to_nav(s.att, C);
        const double fx = C[0][0] * acc.x + C[0][1] * acc.y + C[0][2] * acc.z;
        const double fy = C[1][0] * acc.x + C[1][1] * acc.y + C[1][2] * acc.z;
        const double fz = C[2][0] * acc.x + C[2][1] * acc.y + C[2][2] * acc.z;
        phase_fence();
        const bool resync = ((j + 1) & (kTrigResync - 1)) == 0;
        nav_step<RF, false>(s, gyr, acc, 0.0, dt, ka->earth_rot, resync, mk);
        loose_propagate<TL>(P, C, fx, fy, fz, dt);
    }
    if (b.out_end) store_end(b.out_end, runs, r, s);
    if (RF == 0 && b.out_end_ned) store_end_ned(b.out_end_ned, runs, r, s);
    if (PS) ps.store(b.out_proc, runs, r, (double)(n - a.proc_first), nav_truth);
    if (b.out_bias_end) {
        b.out_bias_end[0 * runs + r] = bg.x; b.out_bias_end[1 * runs + r] = bg.y; b.out_bias_end[2 * runs + r] = bg.z;
        b.out_bias_end[3 * runs + r] = ba.x; b.out_bias_end[4 * runs + r] = ba.y; b.out_bias_end[5 * runs + r] = ba.z;
    }
    if (b.out_pdiag_end) {
#pragma unroll
        for (int k = 0; k < kLooseStates; ++k) b.out_pdiag_end[k * runs + r] = P.get(k, k);
    }
    if (NS == kLooseScaleStates) {
        const loose_scale_ptr sp = loose_scale_params<TL>();
        double* const se = sp->out_scale_end;
        double* const pc = sp->out_pcross_end;
        if (se) { se[r] = kest; se[runs + r] = P.get(kLooseStates, kLooseStates); }
        if (pc) {
#pragma unroll
            for (int k = 0; k < kLooseStates; ++k) pc[k * runs + r] = P.get(k, kLooseStates);
        }
    }
}

}  // namespace ginsim
