// The strapdown solution of one run and what the lane-per-run kernels do with it: Nav / nav_init / nav_step (free integration with
// and without the odometer), the trajectory and end-point stores, and the online process-error statistics (Proc).  Moved here
// verbatim from mc_kernel.hip so that ins_loose.hip mechanises with the same code: the ISA of mc_kernel.hip's kernels is unchanged.
// Kernels that include it take a ginsim_mc_params BY VALUE as their FIRST argument (kernarg_params of sensor_synth.hpp).
#pragma once
#include <hip/hip_runtime.h>
#include "ginsim.h"
#include "ins_math.hpp"
#include "sensor_synth.hpp"

namespace ginsim {

// One strapdown solution (one algorithm instance of one run).
struct Nav {
    Att  att;
    Vec3 vb;    // body velocity (ref_frame 1, free integration)
    Vec3 vel;   // navigation-frame velocity of the previous sample
    Vec3 pos;   // ECEF+displacement (ref_frame 1) or LLA (ref_frame 0)
    double g;   // gravity: constant (ref_frame 1) or the external override of ref_frame 0
    double sl, cl;  // ref_frame 0: cached sin/cos of the latitude pos.x
    bool ext_g; // ref_frame 0: use g instead of the WGS-84 model (free_integration.py:143-146)
};

template <int RF>
__device__ __forceinline__ void nav_init(Nav& s, const double* __restrict__ ini, int has_g) {
    // free_integration.py:96-102 / :127-131
    s.att.set(ini[6], ini[7], ini[8]);
    s.vb = Vec3{ini[3], ini[4], ini[5]};
    s.vel = s.att.to_nav(s.vb);
    if (RF == 1) {
        s.pos = lla2ecef(ini[0], ini[1], ini[2]);
        s.g = has_g ? ini[9] : geo_param(ini[0], ini[2]).g;     // free_integration.py:89-93
    } else {
        s.pos = Vec3{ini[0], ini[1], ini[2]};
        s.g = has_g ? ini[9] : 0.0;
        sincos(ini[0], &s.sl, &s.cl);
    }
    s.ext_g = has_g != 0;
}

// One time step.  ODO == false: free_integration.py:104-116 (RF 1) / :134-172 (RF 0);
//                 ODO == true : free_integration_odo.py:96-105 (RF 1) / :118-152 (RF 0).
template <int RF, bool ODO, bool EASY = false>
__device__ __forceinline__ void nav_step(Nav& s, const Vec3& gyro, const Vec3& accel, double odo, double dt,
                                         int earth_rot, bool resync, const MathConsts& mk) {
    if (RF == 1) {
        const Vec3 v_prev = s.vel;
        if (!ODO) {
            const Vec3 gb = s.att.down_in_body();          // C(att[i-1]) . [0,0,g]
            const Vec3 wxv = cross3(gyro, s.vb);
            s.vb.x += (accel.x + gb.x * s.g) * dt - wxv.x * dt;
            s.vb.y += (accel.y + gb.y * s.g) * dt - wxv.y * dt;
            s.vb.z += (accel.z + gb.z * s.g) * dt - wxv.z * dt;
        }
        s.att.template step<EASY>(gyro, dt, resync, mk);
        if (ODO) {
            const Vec3 f = s.att.fwd_in_nav();
            s.vel = Vec3{f.x * odo, f.y * odo, f.z * odo};
        } else {
            s.vel = s.att.to_nav(s.vb);
        }
        s.pos.x += v_prev.x * dt;
        s.pos.y += v_prev.y * dt;
        s.pos.z += v_prev.z * dt;
    } else {
        const Geo e = geo_param_sc(s.sl, s.cl, s.pos.z);
        const double irm = rcp_n1(e.rm + s.pos.z);     // one Newton step (2^-46): these scale rates of ~1e-6 rad/s
        const double irn = rcp_n1(e.rn + s.pos.z);
        const double icl = rcp_n1(e.cl);
        const Vec3 v = s.vel;
        const Vec3 w_en{v.y * irn, -v.x * irm, -v.y * e.sl * icl * irn};
        Vec3 w_ie{0.0, 0.0, 0.0};
        if (earth_rot) { w_ie.x = kWie * e.cl; w_ie.z = -kWie * e.sl; }
        const Vec3 wb = s.att.to_body(Vec3{w_en.x + w_ie.x, w_en.y + w_ie.y, w_en.z + w_ie.z});
        const Vec3 w_nb{gyro.x - wb.x, gyro.y - wb.y, gyro.z - wb.z};
        Vec3 v_new;
        if (!ODO) {
            const Vec3 an = s.att.to_nav(accel);            // C(att[i-1])^T accel
            const double g = s.ext_g ? s.g : e.g;
            const Vec3 cor = cross3(Vec3{2.0 * w_ie.x + w_en.x, 2.0 * w_ie.y + w_en.y, 2.0 * w_ie.z + w_en.z}, v);
            v_new = Vec3{v.x + (an.x - cor.x) * dt, v.y + (an.y - cor.y) * dt, v.z + (an.z + g - cor.z) * dt};
        }
        s.att.template step<EASY>(w_nb, dt, resync, mk);
        if (ODO) {
            const Vec3 f = s.att.fwd_in_nav();
            v_new = Vec3{f.x * odo, f.y * odo, f.z * odo};
        }
        const double dlat = v.x * irm * dt;
        if (EASY && __builtin_amdgcn_ballot_w64(resync || !(fabs(dlat) <= 0x1.0p-6)) == 0) rotate_sincos_small(dlat, s.sl, s.cl, mk);
        else if (resync || !(fabs(dlat) <= 0.25)) sincos(s.pos.x + dlat, &s.sl, &s.cl);
        else if (fabs(dlat) <= 0x1.0p-6) rotate_sincos_small(dlat, s.sl, s.cl, mk);      // per lane: see Att::step
        else rotate_sincos(dlat, s.sl, s.cl, mk);
        s.pos.x += dlat;
        s.pos.y += v.y * irn * icl * dt;
        s.pos.z += -v.z * dt;
        s.vel = v_new;
    }
}

__device__ __forceinline__ void store9(double* __restrict__ base, int64_t plane, int64_t off, const Nav& s) {
    st(base + 0 * plane + off, s.att.yaw);
    st(base + 1 * plane + off, s.att.pit);
    st(base + 2 * plane + off, s.att.rol);
    st(base + 3 * plane + off, s.pos.x);
    st(base + 4 * plane + off, s.pos.y);
    st(base + 5 * plane + off, s.pos.z);
    st(base + 6 * plane + off, s.vel.x);
    st(base + 7 * plane + off, s.vel.y);
    st(base + 8 * plane + off, s.vel.z);
}

__device__ __forceinline__ void store3(double* __restrict__ base, int64_t plane, int64_t off, const Vec3& v) {
    st(base + off, v.x);
    st(base + plane + off, v.y);
    st(base + 2 * plane + off, v.z);
}

// the second end-point record of ref_frame 0 launches: same attitude / velocity errors, position error in NED metres
__device__ __forceinline__ void store_end_ned(double* __restrict__ out, int64_t runs, int64_t r, const Nav& s) {
    const params_ptr kp = kernarg_params();
    const double ref_end[9] = {kp->ref_end[0], kp->ref_end[1], kp->ref_end[2], kp->ref_end[3], kp->ref_end[4],
                               kp->ref_end[5], kp->ref_end[6], kp->ref_end[7], kp->ref_end[8]};
    out[0 * runs + r] = angle_range_pi(s.att.yaw - ref_end[0]);
    out[1 * runs + r] = angle_range_pi(s.att.pit - ref_end[1]);
    out[2 * runs + r] = angle_range_pi(s.att.rol - ref_end[2]);
    const Vec3 ep = lla_error_ned(s.pos, Vec3{ref_end[3], ref_end[4], ref_end[5]});
    out[3 * runs + r] = ep.x;
    out[4 * runs + r] = ep.y;
    out[5 * runs + r] = ep.z;
    out[6 * runs + r] = s.vel.x - ref_end[6];
    out[7 * runs + r] = s.vel.y - ref_end[7];
    out[8 * runs + r] = s.vel.z - ref_end[8];
}

__device__ __forceinline__ void store_end(double* __restrict__ out, int64_t runs, int64_t r, const Nav& s) {
    const params_ptr kp = kernarg_params();
    const double ref_end[9] = {kp->ref_end[0], kp->ref_end[1], kp->ref_end[2], kp->ref_end[3], kp->ref_end[4],
                               kp->ref_end[5], kp->ref_end[6], kp->ref_end[7], kp->ref_end[8]};
    // array_error(angle=True) on the last sample: ins_data_manager.py:537-541
    out[0 * runs + r] = angle_range_pi(s.att.yaw - ref_end[0]);
    out[1 * runs + r] = angle_range_pi(s.att.pit - ref_end[1]);
    out[2 * runs + r] = angle_range_pi(s.att.rol - ref_end[2]);
    Vec3 ep{s.pos.x - ref_end[3], s.pos.y - ref_end[4], s.pos.z - ref_end[5]};
    if (kp->end_pos_ned && kp->ref_frame == 0) ep = lla_error_ned(s.pos, Vec3{ref_end[3], ref_end[4], ref_end[5]});
    out[3 * runs + r] = ep.x;
    out[4 * runs + r] = ep.y;
    out[5 * runs + r] = ep.z;
    out[6 * runs + r] = s.vel.x - ref_end[6];
    out[7 * runs + r] = s.vel.y - ref_end[7];
    out[8 * runs + r] = s.vel.z - ref_end[8];
}


// Online process-error statistics of one run (InsDataMgr.__process_error_stats, ins_data_manager.py:761-795, on
// array_error :519-553): max|e|, mean and std(ddof=0) of the nine error components over the samples >= proc_first, without
// the samples ever leaving the registers -- which is what makes the statistics available when the trajectories are not kept.
//
// Round 3: RAW sums (sum e, sum e^2) instead of round 2's Welford recurrence (a Newton reciprocal and five dependent fp64
// operations per component and step; now one add, one fused multiply-add, one max).  Conditioning: every run starts on the
// truth, so e is the drift accumulated since sample 0 and |mean| is of the order of the std; the variance comes out as
// sum e^2 / n - mean^2 with a relative rounding error of ~ 2^-53 (1 + mean^2 / var) sqrt(n) -- 1e-12 for mean^2 / var up
// to 1e3 at n = 2e5.  process_stats_kernel (stats.hip), which reads kept trajectories, keeps the Welford / Chan-merge form
// and is the checker: the two agree to 1e-9 relative (tests/test_process_stats.py), the online form to 1e-7 with the oracle.
// The floor of the raw form: an error that is (nearly) CONSTANT over the window -- a noise-free or ideal IMU with an initial
// offset, a deterministic bias -- has var << mean^2, and what sum e^2 / n - mean^2 leaves of a std below ~1.5e-8 |mean| is
// rounding (clamped at 0 here).  No variant runs the raw form any more: the sums are kept about an error close to the mean,
// per lane where the registers are there, per launch where they are not (see Proc;
// tests/test_process_stats.py::test_online_statistics_floor_for_a_constant_error).
// The attitude error is wrapped to (-pi, pi] only when some lane of the wavefront is outside (-pi, pi) (wrap_pi3); exactly -pi
// takes the wrap, which returns +pi as angle_range_pi does.
__device__ __forceinline__ double wrap_pi_lane(double x) { return fabs(x) < kPi ? x : angle_range_pi_mul(x); }

__device__ __forceinline__ void wrap_pi3(double (&e)[9]) {
    const bool out = !(fabs(e[0]) < kPi) || !(fabs(e[1]) < kPi) || !(fabs(e[2]) < kPi);
    if (__builtin_amdgcn_ballot_w64(out) != 0) {
        e[0] = wrap_pi_lane(e[0]); e[1] = wrap_pi_lane(e[1]); e[2] = wrap_pi_lane(e[2]);
    }
}


// SHIFT 1 (round 5): the sums are kept about the FIRST in-window error of the run (sum (e - e0), sum (e - e0)^2): a (nearly)
// constant error then leaves var = sum d^2 / n - (sum d / n)^2 with d of the size of the error's VARIATION, and the floor of the
// raw form (~1.5e-8 |mean| on the std) is gone.  Nine more doubles per lane: every process-statistics variant that has them.
// SHIFT 2 (round 6): the ref_frame 0 free-integration variants (245-251 VGPRs: C3's kernel) and the vibration variants do not.
// Their sums are kept about ONE error for the whole launch: that of the first run's initial state against the truth at sample 0
// (proc_shift_kernel writes the nine numbers before the launch; proc_first > 0 keeps sample 0's, the errors grow from it).  It is
// the same for every lane, so it costs no vector register: it is re-read with scalar loads next to the nine subtractions, the way
// the truth sample is.  What is left under the sums is the error's growth plus what the runs' initial states differ by.
// The nine subtractions cost C3 2.3 %; a caller whose runs start ON the truth (nine zero shifts: the same sums either way) may say
// so (ginsim_mc_params.proc_plain_sums, which ginsim.MonteCarloJob works out from the initial state and the truth it uploads) and
// gets SHIFT 0 in these variants.
template <int SHIFT>
struct Proc {
    double s1[9], s2[9], mx[9], e0[SHIFT == 1 ? 9 : 1];
    __device__ __forceinline__ void clear() {
#pragma unroll
        for (int c = 0; c < 9; ++c) { s1[c] = 0.0; s2[c] = 0.0; mx[c] = 0.0; }
#pragma unroll
        for (int c = 0; c < (SHIFT == 1 ? 9 : 1); ++c) e0[c] = 0.0;
    }
    // the process error of one state against the truth sample t = att3, pos3, vel3 (ins_data_manager.py:761-795); NED: the
    // position error in local NED metres (:542-552)
    template <bool NED>
    static __device__ __forceinline__ void error(const Nav& s, const double (&t)[9], double (&e)[9]) {
        e[0] = s.att.yaw - t[0]; e[1] = s.att.pit - t[1]; e[2] = s.att.rol - t[2];
        wrap_pi3(e);
        if (NED) {
            const Vec3 d = lla_error_ned(s.pos, Vec3{t[3], t[4], t[5]});
            e[3] = d.x; e[4] = d.y; e[5] = d.z;
        } else {
            e[3] = s.pos.x - t[3]; e[4] = s.pos.y - t[4]; e[5] = s.pos.z - t[5];
        }
        e[6] = s.vel.x - t[6]; e[7] = s.vel.y - t[7]; e[8] = s.vel.z - t[8];
    }
    // t (wave-uniform): the truth of this sample; first (wave-uniform): this is the first sample of the window;
    // about (SHIFT 2): the launch's nine shifts, wave-uniform
    template <bool NED>
    __device__ __forceinline__ void add(const Nav& s, const double (&t)[9], bool first, uniform_ptr about) {
        double e[9];
        error<NED>(s, t, e);
        if (SHIFT == 1 && first) {
#pragma unroll
            for (int c = 0; c < 9; ++c) e0[c] = e[c];
        }
#pragma unroll
        for (int c = 0; c < 9; ++c) {
            const double d = SHIFT == 1 ? e[c] - e0[c] : (SHIFT == 2 ? e[c] - about[c] : e[c]);
            s1[c] += d;
            s2[c] = __builtin_fma(d, d, s2[c]);
            mx[c] = fmax(mx[c], fabs(e[c]));
        }
    }
    // Non-finite errors as __array_stats has them (np.max / np.average / np.std): add's fmax drops a NaN, but s2 (a sum of
    // squares) is NaN exactly when some d was, so max|e| is NaN then; s1 carries an infinity into the mean and s2 / cnt - md^2
    // makes the std NaN.  The std keeps a NaN and clamps a rounding negative to 0.
    __device__ __forceinline__ void store(double* __restrict__ out, int64_t runs, int64_t r, double cnt, uniform_ptr about) const {
#pragma unroll
        for (int c = 0; c < 9; ++c) {
            const double md = cnt > 0.0 ? s1[c] / cnt : 0.0;
            const double var = cnt > 0.0 ? s2[c] / cnt - md * md : 0.0;
            out[(0 * 9 + c) * runs + r] = s2[c] != s2[c] ? s2[c] : mx[c];
            out[(1 * 9 + c) * runs + r] = SHIFT == 1 ? e0[c] + md : (SHIFT == 2 ? about[c] + md : md);
            out[(2 * 9 + c) * runs + r] = var < 0.0 ? 0.0 : sqrt(var);
        }
    }
};

}  // namespace ginsim
