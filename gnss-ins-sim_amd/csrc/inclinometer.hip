// Inclinometer kernel: sensor synthesis + MahonyFilter / TiltAcc + the att_euler error statistics, one lane per run.
//
// Restates, per run:
//   Sim.__gen_data_from_pathgen loop body      gnss_ins_sim/sim/ins_sim.py:490-506 (sense3 / add_vibration of sensor_synth.hpp:
//                                              the accel and gyro of run r are those of run r of a free-integration launch)
//   MahonyFilter.run / update / update_imu     demo_algorithms/inclinometer_mahony.py:50-151
//   TiltAcc.run                                demo_algorithms/inclinometer_acc.py:37-56
//   attitude.get_cn2b_acc_mag_ned, dcm2quat, rotation_quat, quat_multiply, quat_normalize   attitude.py:22-90, 294-342, 723-743
//   Sim.__quat2euler_zyx -> quat2euler zyx     ins_sim.py:750-764, attitude.py:91-107, 605-609
//   array_error (angle) + end-point / process statistics   ins_data_manager.py:519-553, 717-795
//
// The run chain (MahonyFilter.reset() clears `ini` only, so run r starts from the gyro_bias run r-1 ended with) is NOT solved
// here: the launch takes each run's initial bias as an input and writes its final bias; the host iterates whole-batch passes to
// the fixed point (ginsim/engine.py, InclinometerJob).  A pass may launch a compacted list of runs (run_list).
//
// The filter arithmetic is compiled without contraction (no fused multiply-add the reference's NumPy does not do); the sensor
// synthesis keeps the file's -ffp-contract=on, which is what mc_kernel.hip is compiled with -- the same bits.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include "ginsim.h"
#include "ins_math.hpp"
#include "philox.hpp"
#include "sensor_synth.hpp"
#include "launch.hpp"

namespace ginsim {

struct Quat { double q0, q1, q2, q3; };

// attitude.get_cn2b_acc_mag_ned then attitude.dcm2quat (attitude.py:22-45, 294-342); c[i][k] = cn2b[i][k]
// Both callers (TiltAcc's (1, 0, 0), Mahony's pseudo-magnetometer) give a DCM of zero yaw: c00 = cos(pitch) >= 0, c11 = cos(roll),
// c22 = c00 c11, so tr <= 0 needs c11 <= 0 and c00 is then the largest diagonal element: only the first and the last branch of
// dcm2quat are reachable through them (counted by tests/test_inclinometer_oracle.py).  The middle two restate the reference.
__device__ __forceinline__ Quat acc_mag_quat(double ax, double ay, double az, double mx, double my, double mz) {
#pragma clang fp contract(off)
    const double an = sqrt(ax * ax + ay * ay + az * az);
    const double zx = -ax / an, zy = -ay / an, zz = -az / an;
    const double cx = zy * mz - zz * my, cy = zz * mx - zx * mz, cz = zx * my - zy * mx;
    const double cn = sqrt(cx * cx + cy * cy + cz * cz);
    const double yx = cx / cn, yy = cy / cn, yz = cz / cn;
    const double xx = yy * zz - yz * zy, xy = yz * zx - yx * zz, xz = yx * zy - yy * zx;
    // columns x, y, z
    const double c00 = xx, c10 = xy, c20 = xz, c01 = yx, c11 = yy, c21 = yz, c02 = zx, c12 = zy, c22 = zz;
    const double tr = c00 + c11 + c22;
    double t0, t1, t2, t3;
    if (tr > 0.0) {
        t0 = 0.5 * sqrt(1.0 + tr);
        t1 = 0.25 / t0 * (c12 - c21);
        t2 = 0.25 / t0 * (c20 - c02);
        t3 = 0.25 / t0 * (c01 - c10);
    } else if (c11 > c00 && c11 > c22) {
        double s = sqrt(c11 - c00 - c22 + 1.0);
        t2 = 0.5 * s;
        if (s != 0.0) s = 0.5 / s;
        t0 = (c20 - c02) * s;
        t1 = (c01 + c10) * s;
        t3 = (c12 + c21) * s;
    } else if (c22 > c00) {
        double s = sqrt(c22 - c00 - c11 + 1.0);
        t3 = 0.5 * s;
        if (s != 0.0) s = 0.5 / s;
        t0 = (c01 - c10) * s;
        t1 = (c20 + c02) * s;
        t2 = (c12 + c21) * s;
    } else {
        double s = sqrt(c00 - c11 - c22 + 1.0);
        t1 = 0.5 * s;
        if (s != 0.0) s = 0.5 / s;
        t0 = (c12 - c21) * s;
        t2 = (c01 + c10) * s;
        t3 = (c20 + c02) * s;
    }
    if (t0 < 0) return Quat{-1.0 * t0, -1.0 * t1, -1.0 * t2, -1.0 * t3};
    return Quat{t0, t1, t2, t3};
}

// attitude.quat2euler zyx (attitude.py:101-107, three_axis_rot :605-609); x ** 2.0 is x * x.  asin is not clamped: an argument
// past 1 gives NaN where the reference raises
__device__ __forceinline__ void quat_euler(const Quat& q, double& yaw, double& pit, double& rol) {
#pragma clang fp contract(off)
    const double r11 = 2.0 * (q.q1 * q.q2 + q.q0 * q.q3);
    const double r12 = q.q0 * q.q0 + q.q1 * q.q1 - q.q2 * q.q2 - q.q3 * q.q3;
    const double r21 = -2.0 * (q.q1 * q.q3 - q.q0 * q.q2);
    const double r31 = 2.0 * (q.q2 * q.q3 + q.q0 * q.q1);
    const double r32 = q.q0 * q.q0 - q.q1 * q.q1 - q.q2 * q.q2 + q.q3 * q.q3;
    yaw = atan2(r11, r12);
    pit = asin(r21);
    rol = atan2(r31, r32);
}

struct MahonyGains { double kp_high, kp_low, ki_high, ki_low, limit, dt; };

// One MahonyFilter instance of one run: the state the reference keeps between samples
struct Mahony {
    Quat q;
    double ei[3];     // err_int
    double b[3];      // gyro_bias
    double t[3];      // tmp = the limited innovation (output 'ab')
    bool ini;

    // MahonyFilter.update + update_imu (inclinometer_mahony.py:74-151) with mag = 0 (the reference's default: update_imu always)
    __device__ __forceinline__ void step(double gx, double gy, double gz, double ax, double ay, double az, const MahonyGains& k) {
#pragma clang fp contract(off)
        const bool acc_valid = (ax != 0.0) || (ay != 0.0) || (az != 0.0);
        const double an = sqrt(ax * ax + ay * ay + az * az);
        const double kp = (fabs(an - 9.8) > 0.2 || sqrt(gx * gx + gy * gy + gz * gz) > 0.2) ? k.kp_low : k.kp_high;
        const double ki = (fabs(an - 9.8) > 0.2 || sqrt(gx * gx + gy * gy + gz * gz) > 0.2) ? k.ki_low : k.ki_high;
        if (acc_valid) { ax = ax / an; ay = ay / an; az = az / an; }
        if (!ini && acc_valid) {
            ini = true;
            ei[0] = 0.0; ei[1] = 0.0; ei[2] = 0.0;
            double m0, m1, m2;
            if (ax >= 1.0) { m0 = 0.0; m1 = 0.0; m2 = 1.0; }
            else if (ay <= -1.0) { m0 = 0.0; m1 = 0.0; m2 = -1.0; }          // acc[1], as the reference has it
            else {
                m0 = sqrt(1.0 - ax * ax);
                m1 = -ay * ax / m0;
                m2 = -ax * az / m0;
            }
            q = acc_mag_quat(ax, ay, az, m0, m1, m2);
        }
        // update_imu
        const double v0 = -2.0 * (q.q1 * q.q3 - q.q0 * q.q2);
        const double v1 = -2.0 * (q.q0 * q.q1 + q.q2 * q.q3);
        const double v2 = -q.q0 * q.q0 + q.q1 * q.q1 + q.q2 * q.q2 - q.q3 * q.q3;
        double e0 = ay * v2 - az * v1, e1 = az * v0 - ax * v2, e2 = ax * v1 - ay * v0;
        const double en = sqrt(e0 * e0 + e1 * e1 + e2 * e2);
        if (en > k.limit) { e0 = e0 / en * k.limit; e1 = e1 / en * k.limit; e2 = e2 / en * k.limit; }
        ei[0] = ei[0] + ki * e0 * k.dt; ei[1] = ei[1] + ki * e1 * k.dt; ei[2] = ei[2] + ki * e2 * k.dt;
        constexpr double kk = 0.9, k1 = 1.0 - 0.9;          // (1-k) as Python evaluates it: 0.09999999999999998
        b[0] = kk * b[0] + k1 * (kp * e0 + ei[0]);
        b[1] = kk * b[1] + k1 * (kp * e1 + ei[1]);
        b[2] = kk * b[2] + k1 * (kp * e2 + ei[2]);
        t[0] = e0; t[1] = e1; t[2] = e2;
        // attitude.quat_update = rotation_quat, quat_multiply, quat_normalize (attitude.py:665-677, 723-743, 75-89, 47-59)
        const double rx = (gx + b[0]) * k.dt, ry = (gy + b[1]) * k.dt, rz = (gz + b[2]) * k.dt;
        const double th = sqrt(rx * rx + ry * ry + rz * rz);
        const double h = 0.5 * th;
        const double s = sin(h), c = cos(h);
        double w0 = 1.0, w1 = 0.0, w2 = 0.0, w3 = 0.0;
        if (th != 0.0) {
            const double tt = c >= 0 ? s / th : -s / th;
            w0 = c >= 0 ? c : -c;
            w1 = tt * rx; w2 = tt * ry; w3 = tt * rz;
        }
        double p0 = q.q0 * w0 - q.q1 * w1 - q.q2 * w2 - q.q3 * w3;
        double p1 = q.q0 * w1 + q.q1 * w0 + q.q2 * w3 - q.q3 * w2;
        double p2 = q.q0 * w2 - q.q1 * w3 + q.q2 * w0 + q.q3 * w1;
        double p3 = q.q0 * w3 + q.q1 * w2 - q.q2 * w1 + q.q3 * w0;
        if (p0 < 0) { p0 = -p0; p1 = -p1; p2 = -p2; p3 = -p3; }
        const double pn = sqrt(p0 * p0 + p1 * p1 + p2 * p2 + p3 * p3);
        q = Quat{p0 / pn, p1 / pn, p2 / pn, p3 / pn};
    }
};

// Online statistics of the att_euler error of one algorithm of one run: the end point and, over samples >= proc_first, max|e|,
// mean and std (ddof 0) about the first in-window error (Proc<1> of mc_kernel.hip, the same non-finite rules)
struct EulerStats {
    double s1[3], s2[3], mx[3], e0[3], last[3];
    __device__ __forceinline__ void clear() {
        for (int c = 0; c < 3; ++c) { s1[c] = 0.0; s2[c] = 0.0; mx[c] = 0.0; e0[c] = 0.0; last[c] = 0.0; }
    }
    __device__ __forceinline__ void add(const double (&eul)[3], uniform_ptr truth, bool in_window, bool first) {
        double e[3];
        for (int c = 0; c < 3; ++c) {
            e[c] = eul[c] - truth[c];
            e[c] = fabs(e[c]) < kPi ? e[c] : angle_range_pi_mul(e[c]);
            last[c] = e[c];
        }
        if (!in_window) return;
        if (first) { e0[0] = e[0]; e0[1] = e[1]; e0[2] = e[2]; }
        for (int c = 0; c < 3; ++c) {
            const double d = e[c] - e0[c];
            s1[c] += d;
            s2[c] = __builtin_fma(d, d, s2[c]);
            mx[c] = fmax(mx[c], fabs(e[c]));
        }
    }
    __device__ __forceinline__ void store(double* end, double* proc, int64_t runs, int64_t r, double cnt) const {
        if (end) for (int c = 0; c < 3; ++c) end[c * runs + r] = last[c];
        if (!proc) return;
        for (int c = 0; c < 3; ++c) {
            const double md = cnt > 0.0 ? s1[c] / cnt : 0.0;
            const double var = cnt > 0.0 ? s2[c] / cnt - md * md : 0.0;
            proc[(0 * 3 + c) * runs + r] = s2[c] != s2[c] ? s2[c] : mx[c];
            proc[(1 * 3 + c) * runs + r] = e0[c] + md;
            proc[(2 * 3 + c) * runs + r] = var < 0.0 ? 0.0 : sqrt(var);
        }
    }
};

__device__ __forceinline__ void put(double* base, int64_t plane, int64_t off, int k, double v) {
    if (base) __builtin_nontemporal_store(v, base + k * plane + off);
}

// ALGOS: GINSIM_INCL_* bits.  GIVEN: sensors read from a.in_accel / a.in_gyro.  VIB: the sensors carry a vibration term.
template <int ALGOS, bool GIVEN, bool VIB>
__global__ void __launch_bounds__(256) incl_kernel(const ginsim_mc_params a, const ginsim_incl_params b) {
    constexpr bool MAH = (ALGOS & GINSIM_INCL_MAHONY) != 0, TILT = (ALGOS & GINSIM_INCL_TILT) != 0;
    __shared__ uint32_t ntab[GIVEN ? 4 : kNormalLdsWords];
    NormalTables tab{};
    if (!GIVEN) {
        tab = fill_normal_tables(ntab, threadIdx.x, blockDim.x);
        __syncthreads();
    }
    const int64_t lane = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (lane >= b.n_list) return;
    const int64_t r = b.run_list ? b.run_list[lane] : lane;
    const int64_t n = a.n, runs = a.runs, plane = n * runs;
    const MahonyGains gk{b.kp_high, b.kp_low, b.ki_high, b.ki_low, b.innovation_limit, b.dt};

    const uint64_t grun = a.run_offset + (uint64_t)r;
    const RngKey key{(uint32_t)a.seed, (uint32_t)(a.seed >> 32), (uint32_t)grun, (uint32_t)(grun >> 32)};
    Vec3 da{0.0, 0.0, 0.0}, dg{0.0, 0.0, 0.0}, vpa{0.0, 0.0, 0.0}, vpg{0.0, 0.0, 0.0};
    const Vec3 nopsd{0.0, 0.0, 0.0};
    if (VIB) {
        vpa = vibration_phase<S_ACC_VIB_PHASE>(&kernarg_params()->vib_accel, key);
        vpg = vibration_phase<S_GYR_VIB_PHASE>(&kernarg_params()->vib_gyro, key);
    }
    Mahony m;
    m.q = Quat{1.0, 0.0, 0.0, 0.0};
    m.ei[0] = m.ei[1] = m.ei[2] = 0.0;
    m.t[0] = m.t[1] = m.t[2] = 0.0;
    m.b[0] = b.bias_in[r]; m.b[1] = b.bias_in[runs + r]; m.b[2] = b.bias_in[2 * runs + r];
    m.ini = false;
    const bool stats = b.out_end[0] || b.out_end[1] || b.out_proc[0] || b.out_proc[1];      // wave-uniform
    EulerStats sm, st;
    sm.clear();
    st.clear();
    const uniform_ptr nav = as_uniform(a.ref_nav);

    for (int64_t j = 0; j < n; ++j) {
        const int64_t off = j * runs + r;
        Vec3 acc, gyr;
        if (GIVEN) {
            acc = Vec3{a.in_accel[off], a.in_accel[plane + off], a.in_accel[2 * plane + off]};
            gyr = Vec3{a.in_gyro[off], a.in_gyro[plane + off], a.in_gyro[2 * plane + off]};
        } else {
            const uint32_t jj = (uint32_t)j;
            const Vec3 cur_a = load3(as_uniform(a.ref_accel), j), cur_g = load3(as_uniform(a.ref_gyro), j);
            double z0[6], z1[6];
            normal_pairs<S_ACC_D_XY, 6>(key, jj, z0, z1, tab);
            const params_ptr kp = kernarg_params();
            acc = sense3<true>(cur_a, &kp->accel, da, Vec3{z0[0], z1[0], z0[1]}, Vec3{z1[1], z0[2], z1[2]});
            gyr = sense3<true>(cur_g, &kp->gyro, dg, Vec3{z0[3], z1[3], z0[4]}, Vec3{z1[4], z0[5], z1[5]});
            if (VIB) {
                acc = add_vibration<S_ACC_VIB_XY>(acc, &kernarg_params()->vib_accel, key, jj, tab, vpa, nopsd);
                gyr = add_vibration<S_GYR_VIB_XY>(gyr, &kernarg_params()->vib_gyro, key, jj, tab, vpg, nopsd);
            }
        }
        const bool in_win = j >= a.proc_first;
        const bool first = j == (a.proc_first > 0 ? a.proc_first : 0);
        if (MAH) {
            m.step(gyr.x, gyr.y, gyr.z, acc.x, acc.y, acc.z, gk);
            double* q = b.out_quat[0];
            put(q, plane, off, 0, m.q.q0); put(q, plane, off, 1, m.q.q1); put(q, plane, off, 2, m.q.q2); put(q, plane, off, 3, m.q.q3);
            for (int c = 0; c < 3; ++c) { put(b.out_wb, plane, off, c, m.b[c]); put(b.out_ab, plane, off, c, m.t[c]); }
            if (stats || b.out_euler[0]) {
                double e[3];
                quat_euler(m.q, e[0], e[1], e[2]);
                for (int c = 0; c < 3; ++c) put(b.out_euler[0], plane, off, c, e[c]);
                if (stats) sm.add(e, nav + 9 * j, in_win, first);
            }
        }
        if (TILT) {
            const Quat tq = acc_mag_quat(acc.x, acc.y, acc.z, 1.0, 0.0, 0.0);
            double* q = b.out_quat[1];
            put(q, plane, off, 0, tq.q0); put(q, plane, off, 1, tq.q1); put(q, plane, off, 2, tq.q2); put(q, plane, off, 3, tq.q3);
            if (stats || b.out_euler[1]) {
                double e[3];
                quat_euler(tq, e[0], e[1], e[2]);
                for (int c = 0; c < 3; ++c) put(b.out_euler[1], plane, off, c, e[c]);
                if (stats) st.add(e, nav + 9 * j, in_win, first);
            }
        }
    }
    if (MAH) {
        if (b.bias_out) { b.bias_out[r] = m.b[0]; b.bias_out[runs + r] = m.b[1]; b.bias_out[2 * runs + r] = m.b[2]; }
    }
    const double cnt = (double)(n - (a.proc_first > 0 ? a.proc_first : 0));
    if (stats && MAH) sm.store(b.out_end[0], b.out_proc[0], runs, r, cnt);
    if (stats && TILT) st.store(b.out_end[1], b.out_proc[1], runs, r, cnt);
}

static bool incl_vibration(const ginsim_mc_params& p) { return p.vib_accel.type != GINSIM_VIB_NONE || p.vib_gyro.type != GINSIM_VIB_NONE; }

int incl_variant(const ginsim_mc_params& p) { return p.given_sensors ? 1 : 0; }

template <int ALGOS>
static hipError_t launch_incl_a(const ginsim_mc_params& p, const ginsim_incl_params& b, hipStream_t stream, char* name, size_t cap) {
    const int tb = p.block_threads > 0 ? p.block_threads : 256;
    const dim3 grid((unsigned)((b.n_list + tb - 1) / tb)), block((unsigned)tb);
    const bool given = p.given_sensors != 0, vib = incl_vibration(p);
    if (name) {
        snprintf(name, cap, "ginsim::incl_kernel<%d, %s, %s>", ALGOS, given ? "true" : "false", vib ? "true" : "false");
        return hipSuccess;
    }
    if (given) hipLaunchKernelGGL((incl_kernel<ALGOS, true, false>), grid, block, 0, stream, p, b);
    else if (vib) hipLaunchKernelGGL((incl_kernel<ALGOS, false, true>), grid, block, 0, stream, p, b);
    else hipLaunchKernelGGL((incl_kernel<ALGOS, false, false>), grid, block, 0, stream, p, b);
    return hipGetLastError();
}

// name != NULL: report the kernel's name, do not launch
hipError_t launch_incl(const ginsim_mc_params& p, const ginsim_incl_params& b, hipStream_t stream, char* name, size_t cap) {
    if (b.n_list <= 0 && !name) return hipSuccess;
    switch (b.algo_mask) {
        case GINSIM_INCL_MAHONY: return launch_incl_a<GINSIM_INCL_MAHONY>(p, b, stream, name, cap);
        case GINSIM_INCL_TILT: return launch_incl_a<GINSIM_INCL_TILT>(p, b, stream, name, cap);
        default: return launch_incl_a<GINSIM_INCL_MAHONY | GINSIM_INCL_TILT>(p, b, stream, name, cap);
    }
}

}  // namespace ginsim
