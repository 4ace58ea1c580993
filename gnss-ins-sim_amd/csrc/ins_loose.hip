// Loosely coupled GPS/INS Kalman filter (InsLoose): sensor synthesis + free-integration mechanisation on bias-corrected
// samples + a 15-state closed-loop error-state filter, one lane per run.
//
// The reference declares the interface only (demo_algorithms/ins_loose.py: input fs, gyro, accel, time, gps_time, gps; output
// pos, vel, att_euler, wb, ab; prediction and correction are `pass`), so the arithmetic is specified here and restated in NumPy
// by tests/ins_loose_ref.py:
//   state order   dr(0-2) dv(3-5) psi(6-8) dbg(9-11) dba(12-14), error = estimate - truth, C_est = (I - [psi x]) C
//   propagation   P <- Phi P Phi^T + Qd, Phi = I + F dt; F: (r,v) = I, (v,psi) = [f^n x], (v,ba) = -C, (psi,bg) = C,
//                 (bg,bg) = -1/tau_g, (ba,ba) = -1/tau_a.  Phi is applied as the block congruences T_r, T_v, T_psi, D in that
//                 order (each reads rows the earlier ones left untouched: the product is exactly I + F dt), 3x3 blocks
//   correction    z = ins - gps, H = [I6 0], six sequential scalar updates, feedback, x = 0
// P is the upper triangle (120 doubles) per lane in LDS, [element][lane], 60 KB per single-wavefront workgroup (two per CU).
// Registers were tried first (one wavefront per SIMD: 256 VGPRs + 256 AGPRs per lane, but arithmetic takes its operands from the
// VGPRs only and a double needs an aligned pair).  The build's resource report with the 240 registers of P, per lane:
//   default flags                  100-700 bytes of scratch in every instantiation
//   machine-LICM off (build.py)    0 for the given-sensors ones without statistics, 12-430 for the others; scheduling fences
//                                  changed nothing; part of P in LDS (30, 60 elements, or 36 parked outside the covariance phases)
//                                  116-490
// With all of P in LDS: 0 bytes in all 12 instantiations (machine-LICM off; with it on the vibration variants keep a 36-byte
// private segment that no instruction addresses).  Every loop over P has compile-time bounds and is fully unrolled, so every LDS
// offset is an immediate.
//
// The sensor synthesis keeps mc_kernel.hip's -ffp-contract=on (same bits as ginsim_mc_run's sensors); a fix is gps_fix of
// gps_synth.hpp (same bits as ginsim_aux_sensors).  The generated and the given form share every line after the samples are in
// registers.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include "ginsim.h"
#include "ins_math.hpp"
#include "philox.hpp"
#include "device_once.hpp"
#include "sensor_synth.hpp"
#include "gps_synth.hpp"
#include "nav.hpp"
#include "launch.hpp"

namespace ginsim {

constexpr int kLooseStates = 15;
constexpr int kLooseTri = kLooseStates * (kLooseStates + 1) / 2;

// index of element (i, j) of the symmetric matrix in its upper triangle, row by row
__host__ __device__ constexpr int tri(int i, int j) {
    return i <= j ? i * kLooseStates - i * (i - 1) / 2 + (j - i) : j * kLooseStates - j * (j - 1) / 2 + (i - j);
}
__host__ __device__ constexpr bool in_block(int k, int b) { return k >= b && k < b + 3; }
// Between the fully unrolled phases of a step: without a fence the scheduler interleaves them for instruction-level parallelism,
// which lengthens live ranges.  Build report of the form below (P in LDS): 0 bytes of scratch with and without the fences,
// 2-110 AGPRs (values parked outside the 256 VGPRs arithmetic can address) with them, 70-230 without.
__device__ __forceinline__ void phase_fence() { __builtin_amdgcn_sched_barrier(0); }

constexpr int kLooseBlock = 64;                                     // lanes per workgroup

// P lives in LDS as [element][lane] doubles, 120 x 64 per wavefront (60 KB: two single-wavefront workgroups per CU): a lane's
// column, no bank conflict, every byte offset a 16-bit immediate.  See the register budget in the file header.
constexpr size_t kLooseCovLds = sizeof(double) * kLooseTri * kLooseBlock;
__device__ __forceinline__ double* cov_lds() {
    extern __shared__ double loose_lds[];
    return loose_lds;
}

struct Cov {
    __device__ __forceinline__ double& at(int i, int j) { return cov_lds()[tri(i, j) * kLooseBlock + threadIdx.x]; }
    __device__ __forceinline__ double get(int i, int j) const { return cov_lds()[tri(i, j) * kLooseBlock + threadIdx.x]; }

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
        for (int k = 0; k < kLooseStates; ++k) {
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
        for (int k = 0; k < kLooseStates; ++k) {
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
            for (int k = 0; k < kLooseStates; ++k) {
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
    __device__ __forceinline__ void update(double z, double rv, double (&x)[kLooseStates]) {
        double col[kLooseStates];
#pragma unroll
        for (int k = 0; k < kLooseStates; ++k) col[k] = get(k, I);
        const double inv = 1.0 / (col[I] + rv);
        const double g = (z - x[I]) * inv;
#pragma unroll
        for (int k = 0; k < kLooseStates; ++k) x[k] += col[k] * g;
#pragma unroll
        for (int a = 0; a < kLooseStates; ++a) {
#pragma unroll
            for (int c = a; c < kLooseStates; ++c) at(a, c) -= col[a] * col[c] * inv;
        }
    }
};

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

// P <- Phi P Phi^T + Qd for the step from the attitude with body -> navigation matrix C and bias-corrected specific force f^n
__device__ __forceinline__ void loose_propagate(Cov& P, const double (&C)[3][3], double fx, double fy, double fz, double dt) {
    const double A[3][3] = {{0.0, -fz * dt, fy * dt}, {fz * dt, 0.0, -fx * dt}, {-fy * dt, fx * dt, 0.0}};      // [f^n x] dt
    double Cp[3][3], Cm[3][3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
#pragma unroll
        for (int c = 0; c < 3; ++c) { Cp[a][c] = C[a][c] * dt; Cm[a][c] = -Cp[a][c]; }
    }
    P.congruence<0, 3>(dt); phase_fence();         // T_r
    P.congruence<3, 6>(A); phase_fence();          // T_v
    P.congruence<3, 12>(Cm); phase_fence();
    P.congruence<6, 9>(Cp); phase_fence();         // T_psi
    const loose_ptr lp = loose_params();
    const double dg[3] = {lp->decay_g[0], lp->decay_g[1], lp->decay_g[2]}, da[3] = {lp->decay_a[0], lp->decay_a[1], lp->decay_a[2]};
    P.scale<9>(dg); phase_fence();                 // D
    P.scale<12>(da); phase_fence();
    const double qv[3] = {lp->q_v[0], lp->q_v[1], lp->q_v[2]}, qp[3] = {lp->q_psi[0], lp->q_psi[1], lp->q_psi[2]};
    P.add_rotated<3>(C, qv); phase_fence();
    P.add_rotated<6>(C, qp); phase_fence();
#pragma unroll
    for (int a = 0; a < 3; ++a) { P.at(9 + a, 9 + a) += lp->q_bg[a]; P.at(12 + a, 12 + a) += lp->q_ba[a]; }
}

// One fix: six scalar updates, then the feedback into the mechanisation and the bias estimates
template <int RF>
__device__ __forceinline__ void loose_correct(Cov& P, Nav& s, Vec3& bg, Vec3& ba, const double (&fix)[6]) {
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
    double x[kLooseStates];
#pragma unroll
    for (int k = 0; k < kLooseStates; ++k) x[k] = 0.0;
    P.update<0>(z[0], lp->r_diag[0], x); phase_fence();
    P.update<1>(z[1], lp->r_diag[1], x); phase_fence();
    P.update<2>(z[2], lp->r_diag[2], x); phase_fence();
    P.update<3>(z[3], lp->r_diag[3], x); phase_fence();
    P.update<4>(z[4], lp->r_diag[4], x); phase_fence();
    P.update<5>(z[5], lp->r_diag[5], x); phase_fence();
    // feedback: truth = estimate - error
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

__device__ __forceinline__ void put3(double* base, int64_t plane, int64_t off, const Vec3& v) {
    if (base) store3(base, plane, off, v);
}

// RF: ref_frame.  GIVEN: samples from in_accel / in_gyro, fixes from in_gps.  VIB: the generated sensors carry a vibration term.
// PS: online process-error statistics (out_proc).
template <int RF, bool GIVEN, bool VIB, bool PS>
__global__ void __launch_bounds__(kLooseBlock)
loose_kernel(const ginsim_mc_params a, const ginsim_loose_params b, const int64_t* __restrict__ stamp, const int32_t* __restrict__ visible) {
    static_assert(!VIB || !GIVEN, "vibration: generate mode");
    __shared__ uint32_t ntab[GIVEN ? 4 : kNormalLdsWords];
    NormalTables tab{};
    if (!GIVEN) {
        tab = fill_normal_tables(ntab, threadIdx.x, blockDim.x);
        __syncthreads();
    }
    const int64_t lane = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (lane >= b.n_list) return;
    const int64_t r = b.run_list ? b.run_list[lane] : lane;
    const int64_t n = a.n, runs = a.runs, plane = n * runs, m = b.m;
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
    Cov P;
#pragma unroll
    for (int i = 0; i < kLooseStates; ++i) {
#pragma unroll
        for (int k = i; k < kLooseStates; ++k) P.at(i, k) = i == k ? b.p0[i / 3] * b.p0[i / 3] : 0.0;
    }
    Proc<1> ps;
    if (PS) ps.clear();
    const uniform_ptr nav_truth = as_uniform(a.ref_nav);
    const bool ned = a.proc_pos_ned != 0;
    int64_t kf = 0;         // the next fix (wave-uniform)

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
                loose_correct<RF>(P, s, bg, ba, fix);
            }
            ++kf;
        }
        if (lb->out_traj) store9(lb->out_traj, plane, off, s);
        put3(lb->out_wb, plane, off, bg);
        put3(lb->out_ab, plane, off, ba);
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
        loose_propagate(P, C, fx, fy, fz, dt);
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
}

int loose_variant(const ginsim_mc_params& p) { return p.given_sensors ? 1 : 0; }

template <int RF, bool PS>
static hipError_t launch_loose_a(const ginsim_mc_params& p, const ginsim_loose_params& b, const int64_t* stamp, const int32_t* visible,
                                 hipStream_t stream, char* name, size_t cap) {
    const int tb = kLooseBlock;
    const dim3 grid((unsigned)((b.n_list + tb - 1) / tb)), block((unsigned)tb);
    const bool given = p.given_sensors != 0, vib = any_vibration(p);
    if (name) {
        snprintf(name, cap, "ginsim::loose_kernel<%d, %s, %s, %s>", RF, given ? "true" : "false", vib ? "true" : "false", PS ? "true" : "false");
        return hipSuccess;
    }
    constexpr size_t kLooseLds = kLooseCovLds;
    static PerDeviceOnce once;          // more than 64 KB of dynamic LDS: the attribute, on every device that launches
    once.run([] {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&loose_kernel<RF, true, false, PS>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLooseLds);
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&loose_kernel<RF, false, true, PS>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLooseLds);
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&loose_kernel<RF, false, false, PS>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLooseLds);
    });
    if (given) hipLaunchKernelGGL((loose_kernel<RF, true, false, PS>), grid, block, kLooseLds, stream, p, b, stamp, visible);
    else if (vib) hipLaunchKernelGGL((loose_kernel<RF, false, true, PS>), grid, block, kLooseLds, stream, p, b, stamp, visible);
    else hipLaunchKernelGGL((loose_kernel<RF, false, false, PS>), grid, block, kLooseLds, stream, p, b, stamp, visible);
    return hipGetLastError();
}

// name != NULL: report the kernel's name, do not launch.  stamp / visible: DEVICE copies of b.gps_stamp / b.gps_visible
hipError_t launch_loose(const ginsim_mc_params& p, const ginsim_loose_params& b, const int64_t* stamp, const int32_t* visible,
                        hipStream_t stream, char* name, size_t cap) {
    if (b.n_list <= 0 && !name) return hipSuccess;
    const bool ps = b.out_proc != nullptr;
    if (p.ref_frame == 1) return ps ? launch_loose_a<1, true>(p, b, stamp, visible, stream, name, cap) : launch_loose_a<1, false>(p, b, stamp, visible, stream, name, cap);
    return ps ? launch_loose_a<0, true>(p, b, stamp, visible, stream, name, cap) : launch_loose_a<0, false>(p, b, stamp, visible, stream, name, cap);
}

}  // namespace ginsim
