// Time-parallel sensor series for few runs: series_kernel<0..3>, series_scan_kernel and their launch (moved verbatim from
// mc_kernel.hip: the ISA of its kernels is unchanged).
#include <hip/hip_runtime.h>
#include <type_traits>
#include "ginsim.h"
#include "ins_math.hpp"
#include "philox.hpp"
#include "sensor_synth.hpp"
#include "launch.hpp"

namespace ginsim {

// ---------------------------------------------------------------------------------------------------
// Sensor series for FEW runs (Sim.run(1) as a data generator, the Allan flow of BASELINE config 5): with one lane per
// run the time loop of mc_kernel is a single sequential chain (n = 1 440 000 samples -> 2.8 s on one lane), and there are
// no runs to fill the chip with.  Here the TIME axis is the parallel one: a lane holds TWO CONSECUTIVE samples (kSpan), a
// wavefront covers 128 consecutive samples of one run per step and walks a chunk of L samples, so
//   * the Philox counter (sample, block, run) makes the twelve normals of a sample a per-lane computation;
//   * a lane writes 16 contiguous bytes of ONE series per step, a wavefront 1 KB -- in the series-major layout
//     [run][axis][n] (sensor_layout 1), which is what ginsim_allan reads: the Allan flow needs no re-layout;
//   * the one sequential thing, the Gauss-Markov recurrence d[j+1] = a d[j] + b w[j] (pathgen.py:583-590), is linear:
//     inside a lane it is evaluated as written, across the lanes of a step it is a weighted inclusive scan of the lanes'
//     two-sample sums with ratio a^2 (Hillis-Steele in DPP: row_shr 1/2/4/8 with the wave-uniform weights a^2, a^4, a^8,
//     a^16, then row_bcast:15 / :31 with the per-lane weights), ONE scan per 128 samples and axis (round 4 had a lane = a
//     sample and scanned every 64: 166 of the 560 vector instructions of a step went into it; the kernels are bound by
//     instruction issue, 1.24 ns per instruction and wave-step in either form), the carry of the previous 128 samples enters
//     at lane 0, and across chunks it is three launches:
//       pass A  chunk-end value of every chunk integrated from zero (drift normals only; a lane accumulates its
//               steps with weight a^128, one weighted wave reduction at the end of the chunk)
//       pass S  chunk-end values -> chunk-START values, start[k+1] = a^L start[k] + end[k]: the same scan, one
//               wavefront per (run, axis)
//       pass B  regenerates the normals (counter-based RNG: no state to carry) and emits
//               truth + bias + drift + white (pathgen.py:500, 562) with the recurrence started from start[k].
// Same normals and the same recurrence as the lane-per-run kernels; only the association of its sums differs (powers of
// a instead of repeated multiplication: a relative 1e-16 on a drift of ~1e-5, far below the 1e-12 / 1e-14 sensor
// tolerances and inside "an ulp of the terms" of the emitted sums, tests/test_gpu_edge_cases.py).
// Round 3's version gave a THREAD a chunk of up to 4096 samples: 44 workgroups for config 5's 32 x 1 440 000 samples
// (17 % of the chip), run-fastest stores 256 B apart, 6.0 ms + a 1.0 ms re-layout in front of a 0.5 ms Allan call.
// wave-uniform weights of the weighted scan with ratio q (ScanWeights below)
struct ScanQ { double q1, q2, q4, q8, q16; };
typedef const ScanQ __attribute__((address_space(4))) * scanq_ptr;

struct SeriesPlan {
    double* carry;          // [runs][nchunks][6]: pass A chunk-end values, pass S overwrites them with chunk-start values
    double a_pow[6];        // gm_a ^ L for accel xyz, gyro xyz
    int64_t nchunks;
    int64_t sr, sc;         // element (run r, axis c, sample j) of a 3-axis sensor lives at r sr + c sc + j
    int64_t odo_sr;         // and of the odometer at r odo_sr + j
    int32_t L;              // samples per chunk, a multiple of 64 kSpan (one step of a wavefront)
    int32_t pad;
    ScanQ   qs[6];          // powers of gm_a ^ kSpan (the scan over the lanes of a step: a lane holds kSpan consecutive samples)
    ScanQ   qL[6];          // powers of gm_a ^ L (pass S)
    double  a_step[6];      // gm_a ^ (64 kSpan) (pass A: the same lane, one step later)
};
typedef const SeriesPlan __attribute__((address_space(4))) * plan_ptr;
// the plan is the second kernel argument: it follows the parameter block in the kernarg segment
__device__ __forceinline__ plan_ptr kernarg_plan(size_t offset) {
    auto p = (const char __attribute__((address_space(4)))*)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(p));
    return (plan_ptr)(p + offset);
}

// Lanes the control cannot serve (the first lanes of a row for row_shr, row 0 for row_bcast) read 0.0 (bound_ctrl); every
// row is written (row_mask 0xf), so the instruction needs no defined previous value of its destination -- with a row mask
// the compiler had to zero the destination first: 84 v_mov per step.  The rows a broadcast must not reach get weight 0.
template <int CTRL>
__device__ __forceinline__ double dpp_or_zero(double x) {
    const int xl = __double2loint(x), xh = __double2hiint(x);
    const int lo = __builtin_amdgcn_update_dpp(xl, xl, CTRL, 0xf, 0xf, true);
    const int hi = __builtin_amdgcn_update_dpp(xh, xh, CTRL, 0xf, 0xf, true);
    return __hiloint2double(hi, lo);
}

// lane l <- lane l-1, lane 0 <- first
__device__ __forceinline__ double wave_shift_up(double x, double first) {
    const int lo = __builtin_amdgcn_update_dpp(__double2loint(first), __double2loint(x), 0x138 /* wave_shr:1 */, 0xf, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(__double2hiint(first), __double2hiint(x), 0x138, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
}

__device__ __forceinline__ double wave_lane63(double x) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(x), 63), hi = __builtin_amdgcn_readlane(__double2hiint(x), 63);
    return __hiloint2double(hi, lo);
}

// Weights of the weighted scan with ratio q: wave-uniform q, q^2, q^4, q^8, q^16 (host-computed, read from the kernarg
// segment where they are used: SGPR pairs, re-loaded per use instead of 48 VGPRs) and, per lane, q^((l & 15) + 1),
// q^((l & 31) + 1) -- zero in the rows that broadcast does not feed.

struct ScanWeights {
    double w15, w31;
    __device__ __forceinline__ void init(scanq_ptr q, int lane) {
        const int p = (lane & 15) + 1;                  // 1 .. 16
        double w = (p & 1) ? q->q1 : 1.0;
        w = (p & 2) ? w * q->q2 : w;
        w = (p & 4) ? w * q->q4 : w;
        w = (p & 8) ? w * q->q8 : w;
        w = (p & 16) ? q->q16 : w;
        w15 = (lane & 16) ? w : 0.0;                                    // rows 1 and 3 take the row before them
        w31 = (lane & 32) ? ((lane & 16) ? w * q->q16 : w) : 0.0;       // rows 2 and 3 take lane 31
    }
    // e[l] = sum_{i <= l} q^(l - i) u[i]
    __device__ __forceinline__ double inclusive(double e, scanq_ptr q) const {
        e = __builtin_fma(q->q1, dpp_or_zero<0x111>(e), e);        // row_shr:1
        e = __builtin_fma(q->q2, dpp_or_zero<0x112>(e), e);        // row_shr:2
        e = __builtin_fma(q->q4, dpp_or_zero<0x114>(e), e);        // row_shr:4
        e = __builtin_fma(q->q8, dpp_or_zero<0x118>(e), e);        // row_shr:8   -> scans of the four rows of 16
        e = __builtin_fma(w15, dpp_or_zero<0x142>(e), e);          // row_bcast:15: lane 15 of a row to the next row
        e = __builtin_fma(w31, dpp_or_zero<0x143>(e), e);          // row_bcast:31: lane 31 to rows 2 and 3
        return e;
    }
};

static void scanq_host(double q, ScanQ* out) {
    out->q1 = q; out->q2 = q * q; out->q4 = out->q2 * out->q2; out->q8 = out->q4 * out->q4; out->q16 = out->q8 * out->q8;
}

constexpr int kSeriesBlock = 256;       // four wavefronts = four chunks per workgroup
// Samples per lane: measured on config 5 (32 x 1 440 000; pass B alone, rocprofv3): 1 -> 601 us, 2 -> 516 us, 4 -> 673 us.  Four halve
// the scan's share again (335 vector instructions per 64 samples against 410) but need 168 registers (three wavefronts per
// SIMD) and read the truth rows with 96-byte lane strides: 48 cache lines per load instruction.
constexpr int kSpan = 2;                // consecutive samples of a lane
constexpr int kSeriesWaves = 4;         // wavefronts per SIMD the register allocator is held to (128 registers; the vibration
                                        // variant, with its sines: three)
constexpr int kGroup = 64 * kSpan;      // samples of one step of a wavefront

// the consecutive doubles of a lane in one series: 16-byte streaming stores (a series starts on an 8-byte boundary only)
typedef double f64x2 __attribute__((ext_vector_type(2)));
typedef f64x2 f64x2_a8 __attribute__((aligned(8)));
__device__ __forceinline__ void st_span(double* p, const double (&v)[kSpan]) {
    if (kSpan == 1) st(p, v[0]);
#pragma unroll
    for (int i = 0; i + 1 < kSpan; i += 2) __builtin_nontemporal_store(f64x2{v[i], v[i + 1]}, reinterpret_cast<f64x2_a8*>(p + i));
}

// PASS 0: pass A; 1: pass B; 2: pass B with the vibration term of Sim(env=...) (a per-sample term: nothing to scan); 3: pass B for
// the simple sensor model (no white-drift axis, no constant bias -- every standard IMU grade of imu_model.py: the six wave-uniform
// selects and the bias additions are compiled out, x + 0.0 == x)
template <int PASS>
__global__ void __launch_bounds__(kSeriesBlock, PASS == 2 ? kSeriesWaves - 1 : kSeriesWaves) series_kernel(const ginsim_mc_params a, const SeriesPlan pl) {
    constexpr bool VIB = PASS == 2;
    constexpr bool WD = PASS != 3;
    __shared__ uint32_t ntab[kNormalLdsWords];
    const NormalTables tab = fill_normal_tables(ntab, threadIdx.x, blockDim.x);
    __syncthreads();

    const int lane = threadIdx.x & 63;
    // grid: x = groups of four chunks, y = run; everything below is wave-uniform (SGPRs) except `lane`
    const int64_t c = (int64_t)blockIdx.x * (kSeriesBlock / 64) + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t r = blockIdx.y;
    if (c >= pl.nchunks) return;
    const int64_t j0 = c * pl.L, j1 = (j0 + pl.L < a.n) ? j0 + pl.L : a.n;
    const uint64_t grun = a.run_offset + (uint64_t)r;
    const RngKey key{(uint32_t)a.seed, (uint32_t)(a.seed >> 32), (uint32_t)grun, (uint32_t)(grun >> 32)};
    double* cb = pl.carry + (r * pl.nchunks + c) * 6;
    const params_ptr kp = kernarg_params();
    double ga[6], gb[6];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        ga[k] = kp->accel.gm_a[k]; gb[k] = kp->accel.gm_b[k];
        ga[3 + k] = kp->gyro.gm_a[k]; gb[3 + k] = kp->gyro.gm_b[k];
    }
    const plan_ptr kq = kernarg_plan(sizeof(ginsim_mc_params));
    if (PASS == 0) {
        // chunk-end value from zero: a lane folds its samples of every step (weight a), its steps with weight a^(64 kSpan),
        // then one scan over the lanes
        double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        auto fold = [&](const int64_t jg, auto full_tag) {
            constexpr bool FULL = decltype(full_tag)::value;        // every sample of the step inside the series: no masks
            double e[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int i = 0; i < kSpan; ++i) {
                const int64_t j = jg + kSpan * lane + i;
                const bool on = FULL || j < j1;
                double z0[6], z1[6];
                normal_pairs<S_ACC_D_XY, 6>(key, (uint32_t)(on ? j : j1 - 1), z0, z1, tab);
                const double zd[6] = {z0[0], z1[0], z0[1], z0[3], z1[3], z0[4]};
#pragma unroll
                for (int k = 0; k < 6; ++k) e[k] = __builtin_fma(ga[k], e[k], on ? gb[k] * zd[k] : 0.0);
            }
#pragma unroll
            for (int k = 0; k < 6; ++k) acc[k] = __builtin_fma(kernarg_plan(sizeof(ginsim_mc_params))->a_step[k], acc[k], e[k]);
        };
        int64_t jg = j0;
        for (; jg + kGroup <= j1; jg += kGroup) fold(jg, std::true_type{});
        if (jg < j1) fold(jg, std::false_type{});
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            ScanWeights sw;                     // of the scan over the LANES: ratio a^kSpan
            sw.init(&kq->qs[k], lane);
            const double e = sw.inclusive(acc[k], &kq->qs[k]);
            if (lane == 63) cb[k] = e;
        }
        return;
    }
    ScanWeights sw[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) sw[k].init(&kq->qs[k], lane);

    // ---- pass B
    const model_ptr ma = &kp->accel, mg = &kp->gyro;
    double carry[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) carry[k] = as_uniform(cb)[k];
    double* const oa = a.out_accel ? a.out_accel + r * pl.sr : nullptr;
    double* const og = a.out_gyro ? a.out_gyro + r * pl.sr : nullptr;
    double* const oo = a.out_odo ? a.out_odo + r * pl.odo_sr : nullptr;
    Vec3 vpa{0.0, 0.0, 0.0}, vpg{0.0, 0.0, 0.0};
    if (VIB) {
        vpa = vibration_phase<S_ACC_VIB_PHASE>(&kp->vib_accel, key);
        vpg = vibration_phase<S_GYR_VIB_PHASE>(&kp->vib_gyro, key);
    }
    // one step = 64 kSpan consecutive samples; FULL: all of them inside the series (every step but the last of a ragged series).
    // The words of the three Philox blocks of the lane's samples first (12 registers each), then one sensor after the other:
    // transform, recurrence, sums, stores -- the scheduling barriers keep the two sensors' working sets apart.
    auto step = [&](const int64_t jg, auto full_tag) {
        constexpr bool FULL = decltype(full_tag)::value;
        const int64_t jl = jg + kSpan * lane;
        bool on[kSpan];
        uint32_t wa[kSpan][6], wb[kSpan][6];
#pragma unroll
        for (int i = 0; i < kSpan; ++i) {
            const int64_t j = jl + i;
            on[i] = FULL || j < j1;
            draw_streams<S_ACC_D_XY, 6>(key, (uint32_t)(on[i] ? j : j1 - 1), wa[i], wb[i]);
        }
        __builtin_amdgcn_sched_barrier(0);
        auto sensor = [&](auto sensor_tag) {
            constexpr int S = decltype(sensor_tag)::value;          // 0: accelerometer (streams 0..2), 1: gyroscope (3..5)
            const model_ptr m = S ? mg : ma;
            const double* const truth = S ? a.ref_gyro : a.ref_accel;
            double* const out = S ? og : oa;
            // the recurrence d[j+1] = a d[j] + b w[j]: inside a lane as written, across the lanes the weighted scan of the
            // lanes' sums (ratio a^kSpan); the drift at the step's first sample enters at lane 0
            double u[kSpan][3], d[kSpan][3], o[kSpan][3];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const int K = 3 * S + k;
#pragma unroll
                for (int i = 0; i < kSpan; ++i) {
                    const uint32_t w = k == 0 ? wa[i][3 * S] : (k == 1 ? wb[i][3 * S] : wa[i][3 * S + 1]);
                    u[i][k] = on[i] ? gb[K] * (double)normal_icdf(w, tab) : 0.0;
                }
                double e = u[0][k];
#pragma unroll
                for (int i = 1; i < kSpan; ++i) e = __builtin_fma(ga[K], e, u[i][k]);
                e = lane == 0 ? __builtin_fma(kernarg_plan(sizeof(ginsim_mc_params))->qs[K].q1, carry[K], e) : e;
                const double inc = sw[K].inclusive(e, &kernarg_plan(sizeof(ginsim_mc_params))->qs[K]);   // drift at the next lane's first sample
                d[0][k] = wave_shift_up(inc, carry[K]);                                                    // at this lane's
                carry[K] = wave_lane63(inc);
#pragma unroll
                for (int i = 1; i < kSpan; ++i) d[i][k] = __builtin_fma(ga[K], d[i - 1][k], u[i - 1][k]);
            }
            // the sums of sense3 (pathgen.py:500, 562), same order of operations
#pragma unroll
            for (int i = 0; i < kSpan; ++i) {
                if (FULL || on[i]) {
                    const int64_t j = jl + i;
#pragma unroll
                    for (int k = 0; k < 3; ++k) {
                        const uint32_t w = k == 0 ? wb[i][3 * S + 1] : (k == 1 ? wa[i][3 * S + 2] : wb[i][3 * S + 2]);
                        const double ud = (WD && m->white_drift[k]) ? u[i][k] : d[i][k];
                        const double tb = WD ? truth[3 * j + k] + m->bias[k] : truth[3 * j + k];
                        o[i][k] = tb + ud + m->white[k] * (double)normal_icdf(w, tab);
                    }
                    if (VIB) {          // added last, as pathgen.py:500, 562 do
                        const Vec3 v = S ? add_vibration<S_GYR_VIB_XY>(Vec3{o[i][0], o[i][1], o[i][2]}, &kernarg_params()->vib_gyro, key, (uint32_t)j, tab, vpg, Vec3{0.0, 0.0, 0.0})
                                         : add_vibration<S_ACC_VIB_XY>(Vec3{o[i][0], o[i][1], o[i][2]}, &kernarg_params()->vib_accel, key, (uint32_t)j, tab, vpa, Vec3{0.0, 0.0, 0.0});
                        o[i][0] = v.x; o[i][1] = v.y; o[i][2] = v.z;
                    }
                    if (!FULL && out) { st(out + j, o[i][0]); st(out + pl.sc + j, o[i][1]); st(out + 2 * pl.sc + j, o[i][2]); }
                }
            }
            if (FULL && out) {
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    double v[kSpan];
#pragma unroll
                    for (int i = 0; i < kSpan; ++i) v[i] = o[i][k];
                    st_span(out + k * pl.sc + jl, v);
                }
            }
            __builtin_amdgcn_sched_barrier(0);
        };
        sensor(std::integral_constant<int, 0>{});
        sensor(std::integral_constant<int, 1>{});
        if (oo) {
            double od[kSpan];
#pragma unroll
            for (int i = 0; i < kSpan; ++i) {
                if (FULL || on[i]) {
                    const int64_t j = jl + i;
                    double y0, y1;
                    normal_pair(key, S_ODO, (uint32_t)j, y0, y1, tab);
                    od[i] = kp->odo_scale * a.ref_odo[j] + kp->odo_stdv * y0;     // pathgen.py:639-640
                    if (!FULL) st(oo + j, od[i]);
                }
            }
            if (FULL) st_span(oo + jl, od);
        }
    };
    int64_t jg = j0;
    for (; jg + kGroup <= j1; jg += kGroup) step(jg, std::true_type{});
    if (jg < j1) step(jg, std::false_type{});
}

// chunk-end values -> chunk-start values, one wavefront per (run, axis): start[0] = 0, start[k+1] = a^L start[k] + end[k]
// is the weighted scan again (ratio a^L), 64 chunks per step
__global__ void __launch_bounds__(64) series_scan_kernel(const SeriesPlan pl, int64_t runs) {
    const int lane = threadIdx.x;
    const int64_t id = blockIdx.x;
    if (id >= runs * 6) return;
    const int64_t r = id / 6;
    const int k = (int)(id % 6);
    double* cb = pl.carry + r * pl.nchunks * 6 + k;
    const scanq_ptr q = &kernarg_plan(0)->qL[k];
    ScanWeights sw;
    sw.init(q, lane);
    double carry = 0.0;                                  // start value of chunk cbase
    for (int64_t cbase = 0; cbase < pl.nchunks; cbase += 64) {
        const int64_t c = cbase + lane;
        const bool on = c < pl.nchunks;
        double u = on ? cb[c * 6] : 0.0;
        u = lane == 0 ? __builtin_fma(pl.a_pow[k], carry, u) : u;
        const double e = sw.inclusive(u, q);             // start of chunk c + 1
        const double s = wave_shift_up(e, carry);        // start of chunk c
        carry = wave_lane63(e);
        if (on) cb[c * 6] = s;
    }
}

// which pass B a launch takes (ginsim_mc_kernel_name reports it)
int series_pass_b(const ginsim_mc_params& p) { return any_vibration(p) ? 2 : (any_white_drift(p) ? 1 : 3); }

// sensors only, few runs, long series
bool series_path_applies(const ginsim_mc_params& p) {
    return p.algo_mask == 0 && !p.given_sensors && p.precision == 0 && !p.wave_trace && p.block_threads == 0 && !any_psd_vibration(p) &&
           p.runs <= 1024 && p.n >= 2048 && (p.sensor_layout == 1 || p.runs == 1);
}

int64_t series_chunks(const ginsim_mc_params& p, int32_t* L_out) {
    // ~16 384 wavefronts over the chip (1024 SIMDs, several rounds of a few wavefronts each), chunks of 256 .. 8192 samples in
    // whole wave-steps, and at most 1024 chunks per run where that fits (pass S walks them 64 at a time)
    int64_t L = (p.n * p.runs + 16383) / 16384;
    const int64_t lmin = (p.n + 1023) / 1024;
    if (L < lmin) L = lmin;
    if (L < 256) L = 256;
    if (L > 8192) L = 8192;
    L = (L + kGroup - 1) / kGroup * kGroup;
    *L_out = (int32_t)L;
    return (p.n + L - 1) / L;
}

hipError_t launch_series(const ginsim_mc_params& p, double* carry, hipStream_t stream) {
    SeriesPlan pl;
    pl.carry = carry;
    pl.nchunks = series_chunks(p, &pl.L);
    for (int k = 0; k < 6; ++k) {
        const double aa = k < 3 ? p.accel.gm_a[k] : p.gyro.gm_a[k - 3];
        double v = 1.0;
        for (int i = 0; i < pl.L; ++i) v *= aa;
        pl.a_pow[k] = v;
        static_assert(kSpan == 2, "the host's powers of gm_a");
        scanq_host(aa * aa, &pl.qs[k]);
        scanq_host(v, &pl.qL[k]);
        const double a16s = pl.qs[k].q16, a32s = a16s * a16s;     // gm_a ^ (16 span), ^ (32 span)
        pl.a_step[k] = a32s * a32s;                                  // gm_a ^ (64 span): one step of a wavefront
    }
    pl.pad = 0;
    // the sample index is the contiguous one in both layouts the path serves (series_path_applies: layout 1, or one run)
    if (p.sensor_layout == 1) { pl.sr = 3 * p.n; pl.sc = p.n; pl.odo_sr = p.n; }
    else { pl.sr = 0; pl.sc = p.n; pl.odo_sr = 0; }
    const dim3 grid((unsigned)((pl.nchunks + kSeriesBlock / 64 - 1) / (kSeriesBlock / 64)), (unsigned)p.runs), block(kSeriesBlock);
    hipLaunchKernelGGL((series_kernel<0>), grid, block, 0, stream, p, pl);
    hipLaunchKernelGGL(series_scan_kernel, dim3((unsigned)(p.runs * 6)), dim3(64), 0, stream, pl, p.runs);
    if (any_vibration(p)) hipLaunchKernelGGL((series_kernel<2>), grid, block, 0, stream, p, pl);
    else if (any_white_drift(p)) hipLaunchKernelGGL((series_kernel<1>), grid, block, 0, stream, p, pl);
    else hipLaunchKernelGGL((series_kernel<3>), grid, block, 0, stream, p, pl);
    return hipGetLastError();
}

}  // namespace ginsim
