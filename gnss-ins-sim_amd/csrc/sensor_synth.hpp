// Sensor synthesis shared by the kernels of the fp64 path (mc_kernel.hip, series.hip, inclinometer.hip): one run's
// accelerometer and gyroscope samples from the truth, the Gauss-Markov drift, the white noise and the vibration term, and
// the helpers they read their inputs through.  Kernels that include it take a ginsim_mc_params BY VALUE as their FIRST
// argument (kernarg_params).  Moved here verbatim from mc_kernel.hip: the ISA of its kernels is unchanged.
#pragma once
#include <hip/hip_runtime.h>
#include "ginsim.h"
#include "ins_math.hpp"
#include "philox.hpp"

namespace ginsim {


// The by-value parameter block sits at offset 0 of the kernarg segment.  Its bulky members (two sensor models,
// ref_end) are re-read from there with scalar loads where they are used: kept in SGPRs for the whole time loop
// they overflow the SGPR file and the compiler parks them in VGPR lanes (v_readlane/v_writelane = VALU issue
// slots, ~14 % of the loop in the first build).  The empty asm makes the pointer opaque per iteration so the
// loads are not hoisted back out of the loop.
typedef const ginsim_mc_params __attribute__((address_space(4))) * params_ptr;
__device__ __forceinline__ params_ptr kernarg_params() {
    params_ptr p = (params_ptr)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(p));
    return p;
}
typedef const ginsim_sensor_model __attribute__((address_space(4))) * model_ptr;

// attitude.angle_range_pi with the division by 2 pi replaced by a multiplication, exactly as process_stats_kernel
// (stats.hip) evaluates it: the two statistics paths agree to the bit
__device__ __forceinline__ double angle_range_pi_mul(double x) {
    double m = x - kTwoPi * floor(x * (1.0 / kTwoPi));
    if (m >= kTwoPi) m -= kTwoPi;
    if (m < 0.0) m += kTwoPi;
    return m > kPi ? m - kTwoPi : m;
}

// Truth samples are the same for every lane.  Reading them through the constant address space tells the
// compiler the data are invariant, so a wave-uniform index becomes an s_load (scalar cache, lgkmcnt) instead
// of a per-lane global_load -- which matters beyond the 64x fewer bytes: vector loads share the vmcnt counter
// with the trajectory stores, and the s_waitcnt vmcnt(0) guarding them drained every outstanding store once
// per step (measured: +0.45 ms at 65 536 runs).
typedef const double __attribute__((address_space(4))) * uniform_ptr;
__device__ __forceinline__ uniform_ptr as_uniform(const double* p) {
    return (uniform_ptr)(uintptr_t)p;
}

// The nine coefficients of the simple sensor model as values, all asked for at once (one batch of scalar loads), for a caller that
// wants them due at one point instead of where sense3 uses them.  The bias and the white-drift flags of the general model (WD) stay
// behind the pointer and are read where they are used, as through model_ptr.
struct ModelBatch {
    double gm_a[3], gm_b[3], white[3];
    struct Bias {
        model_ptr m;
        __device__ __forceinline__ double operator[](int k) const { return m->bias[k]; }
    } bias;
    struct WhiteDrift {
        model_ptr m;
        __device__ __forceinline__ int32_t operator[](int k) const { return m->white_drift[k]; }
    } white_drift;
};
__device__ __forceinline__ ModelBatch load_model(model_ptr m) {
    return ModelBatch{{m->gm_a[0], m->gm_a[1], m->gm_a[2]}, {m->gm_b[0], m->gm_b[1], m->gm_b[2]}, {m->white[0], m->white[1], m->white[2]}, {m}, {m}};
}

// Sensor sample j of one 3-axis sensor: truth + bias + drift + white  (pathgen.py:500, 562), and the
// Gauss-Markov update d[j+1] = a d[j] + b N[j] (pathgen.py:589-590).
__device__ __forceinline__ Vec3 load3(uniform_ptr ref, int64_t j) { return Vec3{ref[3 * j], ref[3 * j + 1], ref[3 * j + 2]}; }

// WD = false: the launcher saw no axis with an infinite correlation time (white_drift) and no constant bias in either
// sensor -- every standard IMU grade of imu_model.py -- so the six wave-uniform selects and the three bias additions
// per sensor are compiled out (x + 0.0 == x: the values are the same).
// M: where the model is read from -- model_ptr (the kernarg segment, scalar loads at each use) or a pointer to a ModelBatch the caller
// loaded itself (the consumer of mc_kernel_split); the same expressions on the same values either way.
template <bool WD = true, class M = model_ptr>
__device__ __forceinline__ Vec3 sense3(const Vec3& truth, M m, Vec3& drift, const Vec3& zd,
                                       const Vec3& zw) {
    const double bx = m->gm_b[0] * zd.x, by = m->gm_b[1] * zd.y, bz = m->gm_b[2] * zd.z;
    const double dx = (WD && m->white_drift[0]) ? bx : drift.x;
    const double dy = (WD && m->white_drift[1]) ? by : drift.y;
    const double dz = (WD && m->white_drift[2]) ? bz : drift.z;
    Vec3 o;
    if (WD) {
        o.x = truth.x + m->bias[0] + dx + m->white[0] * zw.x;
        o.y = truth.y + m->bias[1] + dy + m->white[1] * zw.y;
        o.z = truth.z + m->bias[2] + dz + m->white[2] * zw.z;
    } else {
        o.x = truth.x + dx + m->white[0] * zw.x;
        o.y = truth.y + dy + m->white[1] * zw.y;
        o.z = truth.z + dz + m->white[2] * zw.z;
    }
    drift.x = __builtin_fma(m->gm_a[0], drift.x, bx);
    drift.y = __builtin_fma(m->gm_a[1], drift.y, by);
    drift.z = __builtin_fma(m->gm_a[2], drift.z, bz);
    return o;
}

// The vibration term of a sensor sample (ABI 5; pathgen.py:476-492, 538-556), added LAST as the reference's sum does
// (a_mea = ref + bias + drift + noise + vib).  Everything wave-uniform except the normals and the per-run phases.
typedef const ginsim_vibration __attribute__((address_space(4))) * vib_ptr;

template <uint32_t PHASE_STREAM>
__device__ __forceinline__ Vec3 vibration_phase(vib_ptr v, const RngKey& key) {
    if (v->type != GINSIM_VIB_SINUSOIDAL || !v->random_phase) return Vec3{0.0, 0.0, 0.0};
    const u32x4 w = philox4x32(0u, PHASE_STREAM >> 1, key.r0, key.r1, key.k0, key.k1);
    // np.random.rand(1)*2*math.pi (pathgen.py:553-555), u = word 2^-32
    return Vec3{((double)w.x * 0x1p-32 * 2.0) * kPi, ((double)w.y * 0x1p-32 * 2.0) * kPi, ((double)w.z * 0x1p-32 * 2.0) * kPi};
}

// the term itself, the three normals of a 'random' vibration given (zx, zy, zz: whoever generated them -- this wavefront, or the
// producers of the wave-specialised kernel through the LDS ring)
__device__ __forceinline__ Vec3 vibration_term(const Vec3& o, vib_ptr v, double zx, double zy, double zz, uint32_t j, const Vec3& phase) {
    Vec3 r = o;
    if (v->type == GINSIM_VIB_RANDOM) {
        r.x = o.x + v->amp[0] * zx;
        r.y = o.y + v->amp[1] * zy;
        r.z = o.z + v->amp[2] * zz;
    } else if (v->type == GINSIM_VIB_SINUSOIDAL) {
        const double cj = v->omega_dt * (double)j;          // (2 pi f dt) * arange(n), rounded before the phase is added
        if (v->random_phase) {
            const double ax = cj + phase.x, ay = cj + phase.y, az = cj + phase.z;
            r.x = o.x + v->amp[0] * sin(ax);
            r.y = o.y + v->amp[1] * sin(ay);
            r.z = o.z + v->amp[2] * sin(az);
        } else {
            const double s = sin(cj);
            r.x = o.x + v->amp[0] * s;
            r.y = o.y + v->amp[1] * s;
            r.z = o.z + v->amp[2] * s;
        }
    }
    return r;
}

// The three values of sample j of a 'psd' vibration (ABI 8): the series were made before the launch (vib_psd.hip), [axis][sample mod
// period][run], tiled to n (time_series_from_psd.py:58-63).  Zero for every other type.  Called at the TOP of a step, ~800
// instructions before the sum that takes the values: asked for next to the sum, the loads cost their whole latency every step.
__device__ __forceinline__ Vec3 psd_vibration(vib_ptr v, uint32_t j, int64_t run, int64_t runs) {
    if (v->type != GINSIM_VIB_PSD) return Vec3{0.0, 0.0, 0.0};
    const int64_t period = v->period;
    const double* s = v->series + (int64_t)(j % (uint32_t)period) * runs + run;
    const int64_t pl = period * runs;
    return Vec3{__builtin_nontemporal_load(s), __builtin_nontemporal_load(s + pl), __builtin_nontemporal_load(s + 2 * pl)};
}

// psd: psd_vibration() of this sensor and sample
template <uint32_t STREAM>
__device__ __forceinline__ Vec3 add_vibration(const Vec3& o, vib_ptr v, const RngKey& key, uint32_t j, const NormalTables& tab,
                                              const Vec3& phase, const Vec3& psd) {
    Vec3 r = o;
    if (v->type == GINSIM_VIB_PSD) {
        r.x = o.x + psd.x;
        r.y = o.y + psd.y;
        r.z = o.z + psd.z;
    } else if (v->type == GINSIM_VIB_RANDOM) {
        double z0[2], z1[2];
        normal_pairs<STREAM, 2>(key, j, z0, z1, tab);
        r.x = o.x + v->amp[0] * z0[0];
        r.y = o.y + v->amp[1] * z1[0];
        r.z = o.z + v->amp[2] * z0[1];
    } else if (v->type == GINSIM_VIB_SINUSOIDAL) {
        const double cj = v->omega_dt * (double)j;          // (2 pi f dt) * arange(n), rounded before the phase is added
        if (v->random_phase) {
            const double ax = cj + phase.x, ay = cj + phase.y, az = cj + phase.z;
            r.x = o.x + v->amp[0] * sin(ax);
            r.y = o.y + v->amp[1] * sin(ay);
            r.z = o.z + v->amp[2] * sin(az);
        } else {
            const double s = sin(cj);
            r.x = o.x + v->amp[0] * s;
            r.y = o.y + v->amp[1] * s;
            r.z = o.z + v->amp[2] * s;
        }
    }
    return r;
}

// Series are written once and not read back by the kernel: non-temporal stores keep them from displacing the L2.
__device__ __forceinline__ void st(double* p, double v) { __builtin_nontemporal_store(v, p); }

}  // namespace ginsim
