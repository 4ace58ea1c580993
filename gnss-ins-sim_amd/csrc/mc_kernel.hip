// Fused Monte-Carlo kernel: sensor-error injection + strapdown mechanisation + end-point error.
//
// One lane = one Monte-Carlo run (no inter-lane traffic in the time loop; workgroups of 256 or 512 threads only
// shape the placement on the SIMDs and share the coefficient table (8 KB of LDS) of the normal transform).  Per-run state (Euler attitude + cached
// trig, body/NED velocity, position, the six Gauss-Markov bias states) lives in VGPRs for the whole time loop.
// Truth samples are wave-uniform and come in through the scalar cache.  Everything that leaves the lane is SoA [component][sample][run]
// (run fastest) so that every store instruction of a wavefront writes 64 x 8 B contiguous bytes.
//
// Restates, per run:
//   Sim.__gen_data_from_pathgen loop body      gnss_ins_sim/sim/ins_sim.py:490-506
//   pathgen.acc_gen / gyro_gen / bias_drift    gnss_ins_sim/pathgen/pathgen.py:441-594
//   pathgen.odo_gen                            gnss_ins_sim/pathgen/pathgen.py:627-641
//   FreeIntegration.run                        demo_algorithms/free_integration.py:63-174
//   FreeIntegration.run (odometer variant)     demo_algorithms/free_integration_odo.py:63-160
//   array_error + end-point pick               gnss_ins_sim/sim/ins_data_manager.py:519-541, 737
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <type_traits>
#include "ginsim.h"
#include "ins_math.hpp"
#include "philox.hpp"
#include "device_once.hpp"
#include "sensor_synth.hpp"
#include "nav.hpp"
#include "launch.hpp"

namespace ginsim {

constexpr int kWave = 64;


// Two workgroups per CU is what the launch geometry below counts on: tell the register allocator (variants had grown
// to 256 VGPRs + a few AGPRs = one wavefront per SIMD, 30 % slower at 262 144 runs, with no functional symptom;
// tests/test_host_cpu.py now reads the compiler's resource report).
// PS: 0 = no process statistics; 1 = online process-error statistics of the (single) algorithm; 2 = the same with the
// position error in NED metres (ref_frame 0); 3 / 4 = 1 / 2 with the sums taken as they are (ginsim_mc_params.proc_plain_sums:
// the caller states that the runs start ON the truth, so the launch's shift would be nine zeros -- the same sums without the
// nine subtractions per step; only the variants whose shift is per launch have the form, see Proc).
// VIB: the sensors carry a vibration term (vib_accel / vib_gyro; general sensor model, generate mode).
template <int RF, int ALGOS, bool GIVEN, bool WD, int PS = 0, bool VIB = false>
__global__ void __launch_bounds__(256, 2) mc_kernel(const ginsim_mc_params a, const double* __restrict__ proc_about) {
    static_assert(PS == 0 || (!GIVEN && (ALGOS == GINSIM_ALGO_FREE || ALGOS == GINSIM_ALGO_ODO)), "process statistics: one algorithm, generate mode");
    static_assert(!VIB || (!GIVEN && WD), "vibration: generate mode, general sensor model");
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint64_t* trace = nullptr;
    if (a.wave_trace && (threadIdx.x & 63) == 0) {
        trace = a.wave_trace + 4 * (((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6);
        trace[0] = __builtin_amdgcn_s_getreg((31 << 11) | 4);     // HW_REG_HW_ID
        trace[1] = __builtin_amdgcn_s_getreg((31 << 11) | 20);    // HW_REG_XCC_ID
        trace[2] = __builtin_amdgcn_s_memtime();
    }
    __shared__ uint32_t ntab[GIVEN ? 4 : kNormalLdsWords];
    NormalTables tab{};
    if (!GIVEN) {
        tab = fill_normal_tables(ntab, threadIdx.x, blockDim.x);
        __syncthreads();
    }
    if (r >= a.runs) return;
    constexpr bool FREE = (ALGOS & GINSIM_ALGO_FREE) != 0;
    constexpr bool ODO = (ALGOS & GINSIM_ALGO_ODO) != 0;
    const int64_t n = a.n;
    const int64_t runs = a.runs;
    const int64_t plane = n * runs;
    const double dt = 1.0 / a.fs;

    // which set of initial states: free_integration.py:85-87 (run_times counts calls since construction)
    const uint64_t call = a.ini_first + (uint64_t)r;
    const double* ini = a.ini + 10 * (call < (uint64_t)a.n_ini ? call : 0);
    Nav fi, od;
    if (FREE) nav_init<RF>(fi, ini, a.ini_has_g);
    if (ODO) nav_init<RF>(od, ini, a.ini_has_g);

    const uint64_t grun = a.run_offset + (uint64_t)r;
    const RngKey key{(uint32_t)a.seed, (uint32_t)(a.seed >> 32), (uint32_t)grun, (uint32_t)(grun >> 32)};
    Vec3 da{0.0, 0.0, 0.0}, dg{0.0, 0.0, 0.0};
    Vec3 vpa{0.0, 0.0, 0.0}, vpg{0.0, 0.0, 0.0};
    if (VIB) {
        vpa = vibration_phase<S_ACC_VIB_PHASE>(&kernarg_params()->vib_accel, key);
        vpg = vibration_phase<S_GYR_VIB_PHASE>(&kernarg_params()->vib_gyro, key);
    }
    MathConsts mk;
    // constants pinned in VGPRs except where that variant would spill to scratch (measured per variant)
    mk.init<(ALGOS != (GINSIM_ALGO_FREE | GINSIM_ALGO_ODO)) && PS == 0 && !VIB>();

    if (FREE && a.out_traj[0]) store9(a.out_traj[0], plane, r, fi);
    if (ODO && a.out_traj[1]) store9(a.out_traj[1], plane, r, od);
    // the sums shifted per lane wherever the registers are there, per launch elsewhere (see Proc)
    constexpr bool PNED = PS == 2 || PS == 4, PPLAIN = PS >= 3;
    static_assert(!PPLAIN || (RF == 0 && ALGOS == GINSIM_ALGO_FREE && !VIB), "plain sums: only where the shift is per launch and optional");
    constexpr int PSHIFT = PS == 0 ? 0 : ((!VIB && !(RF == 0 && ALGOS == GINSIM_ALGO_FREE)) ? 1 : (PPLAIN ? 0 : 2));
    const uniform_ptr nav_truth = as_uniform(a.ref_nav);
    // opaque per use: hoisted out of the time loop the nine shifts would sit in 18 SGPRs the loop does not have
    auto about = [&]() -> uniform_ptr {
        uniform_ptr q = as_uniform(proc_about);
        if (PSHIFT == 2) asm volatile("" : "+s"(q));
        return q;
    };
    Proc<PSHIFT> ps;
    if (PS) {
        ps.clear();
        if (a.proc_first <= 0) {                    // sample 0 is the initial state (free_integration.py:96-102)
            const double t[9] = {nav_truth[0], nav_truth[1], nav_truth[2], nav_truth[3], nav_truth[4], nav_truth[5],
                                 nav_truth[6], nav_truth[7], nav_truth[8]};
            ps.template add<PNED>(FREE ? fi : od, t, true, about());
        }
    }

    for (int64_t j = 0; j < n; ++j) {
        const int64_t off = j * runs + r;
        Vec3 acc, gyr;
        double odo = 0.0;
        if (GIVEN) {
            if (j == n - 1) break;
            gyr = Vec3{a.in_gyro[off], a.in_gyro[plane + off], a.in_gyro[2 * plane + off]};
            if (FREE) acc = Vec3{a.in_accel[off], a.in_accel[plane + off], a.in_accel[2 * plane + off]};
            if (ODO) odo = a.in_odo[off];
        } else {
            const bool last = (j == n - 1);
            // the last sample only exists as sensor output; skip it when nothing stores it
            if (last && !a.out_accel && !a.out_gyro && !a.out_odo) break;
            const uint32_t jj = (uint32_t)j;
            // wave-uniform truth of this step: requested here, ~800 instructions before the sensor sums use it
            const Vec3 cur_a = load3(as_uniform(a.ref_accel), j), cur_g = load3(as_uniform(a.ref_gyro), j);
            Vec3 psd_a{0.0, 0.0, 0.0}, psd_g{0.0, 0.0, 0.0};
            if (VIB) {
                psd_a = psd_vibration(&kernarg_params()->vib_accel, jj, r, runs);
                psd_g = psd_vibration(&kernarg_params()->vib_gyro, jj, r, runs);
            }
            const bool need_acc = FREE || a.out_accel;
            const bool need_gyr = FREE || ODO || a.out_gyro;
            const bool need_odo = ODO || a.out_odo;
            if (need_acc && need_gyr) {             // the common case: six streams in one phased batch
                double z0[6], z1[6];
                normal_pairs<S_ACC_D_XY, 6>(key, jj, z0, z1, tab);
                const params_ptr kp = kernarg_params();
                acc = sense3<WD>(cur_a, &kp->accel, da, Vec3{z0[0], z1[0], z0[1]}, Vec3{z1[1], z0[2], z1[2]});
                gyr = sense3<WD>(cur_g, &kp->gyro, dg, Vec3{z0[3], z1[3], z0[4]}, Vec3{z1[4], z0[5], z1[5]});
            } else if (need_acc) {
                double z0[3], z1[3];
                normal_pairs<S_ACC_D_XY, 3>(key, jj, z0, z1, tab);
                acc = sense3<WD>(cur_a, &kernarg_params()->accel, da, Vec3{z0[0], z1[0], z0[1]}, Vec3{z1[1], z0[2], z1[2]});
            } else if (need_gyr) {
                double z0[3], z1[3];
                normal_pairs<S_GYR_D_XY, 3>(key, jj, z0, z1, tab);
                gyr = sense3<WD>(cur_g, &kernarg_params()->gyro, dg, Vec3{z0[0], z1[0], z0[1]}, Vec3{z1[1], z0[2], z1[2]});
            }
            if (VIB) {
                if (need_acc) acc = add_vibration<S_ACC_VIB_XY>(acc, &kernarg_params()->vib_accel, key, jj, tab, vpa, psd_a);
                if (need_gyr) gyr = add_vibration<S_GYR_VIB_XY>(gyr, &kernarg_params()->vib_gyro, key, jj, tab, vpg, psd_g);
            }
            if (need_acc && a.out_accel) store3(a.out_accel, plane, off, acc);
            if (need_gyr && a.out_gyro) store3(a.out_gyro, plane, off, gyr);
            if (need_odo) {
                double z0, z1;
                normal_pair(key, S_ODO, jj, z0, z1, tab);
                const params_ptr kq = kernarg_params();
                odo = kq->odo_scale * as_uniform(a.ref_odo)[j] + kq->odo_stdv * z0;     // pathgen.py:639-640
                if (a.out_odo) a.out_odo[off] = odo;
            }
            if (last) break;
        }
        const bool resync = ((j + 1) & (kTrigResync - 1)) == 0;
        if (FREE) {
            nav_step<RF, false, !GIVEN>(fi, gyr, acc, 0.0, dt, a.earth_rot, resync, mk);
            if (a.out_traj[0]) store9(a.out_traj[0], plane, off + runs, fi);
        }
        if (ODO) {
            nav_step<RF, true, !GIVEN>(od, gyr, acc, odo, dt, a.earth_rot, resync, mk);
            if (a.out_traj[1]) store9(a.out_traj[1], plane, off + runs, od);
        }
        if (PS) {
            if (j + 1 >= a.proc_first) {            // wave-uniform
                const uniform_ptr q = nav_truth + 9 * (j + 1);
                const double t[9] = {q[0], q[1], q[2], q[3], q[4], q[5], q[6], q[7], q[8]};
                ps.template add<PNED>(FREE ? fi : od, t, a.proc_first > 0 && j + 1 == a.proc_first, about());
            }
        }
    }
    if (FREE && a.out_end[0]) store_end(a.out_end[0], runs, r, fi);
    if (ODO && a.out_end[1]) store_end(a.out_end[1], runs, r, od);
    if (RF == 0) {
        if (FREE && a.out_end_ned[0]) store_end_ned(a.out_end_ned[0], runs, r, fi);
        if (ODO && a.out_end_ned[1]) store_end_ned(a.out_end_ned[1], runs, r, od);
    }
    if (PS) ps.store(a.out_proc[FREE ? 0 : 1], runs, r, (double)(n - (a.proc_first > 0 ? a.proc_first : 0)), about());
    if (trace) trace[3] = __builtin_amdgcn_s_memtime();
}

// The launch-wide shift of the process statistics (Proc, SHIFT 2): the process error of the FIRST run's initial state against
// the truth at sample 0, nine doubles.  One lane, before the launch, on its stream.
template <int RF, bool NED>
__global__ void proc_shift_kernel(const ginsim_mc_params a, double* __restrict__ about) {
    const double* ini = a.ini + 10 * (a.ini_first < (uint64_t)a.n_ini ? a.ini_first : 0);
    Nav z;
    nav_init<RF>(z, ini, a.ini_has_g);
    const double t[9] = {a.ref_nav[0], a.ref_nav[1], a.ref_nav[2], a.ref_nav[3], a.ref_nav[4], a.ref_nav[5],
                         a.ref_nav[6], a.ref_nav[7], a.ref_nav[8]};
    double e[9];
    Proc<0>::error<NED>(z, t, e);
    for (int c = 0; c < 9; ++c) about[c] = e[c];
}

// ---------------------------------------------------------------------------------------------------
// Wave-specialised variant, written for SMALL batches (<= 1024 wavefronts of runs, i.e. one wavefront per SIMD with the
// kernel above -- BASELINE config 2) and, with two producer groups, the faster one at every size (mc_variant).  A lone wavefront cannot hide its own dependent-instruction and s_waitcnt latencies
// and there are no more runs to give the SIMD a second wavefront.  So the work of one step is split across TWO
// wavefronts per 64 runs, at the point where the normal generator changes character:
//
//   waves 4-7 of a 512-thread workgroup (producers): the three Philox blocks of a step and the twelve single-precision
//                                                    normal transforms -> LDS ring, per step and run the twelve
//                                                    normals as floats (48 B)
//   waves 0-3 (consumers)                          : read tile i-1 from LDS, widen, sensor sums, mechanisation, all stores
//
// One __syncthreads() per tile of T = kSplitTile (6) steps; the instruction total is unchanged, the SIMD just always has a second
// wavefront to issue from.  Results are bit-identical to mc_kernel (same functions in the same order on the same values).
constexpr int kSplitRuns = 256;
#ifndef GINSIM_SPLIT_TILE
#define GINSIM_SPLIT_TILE 6
#endif
constexpr int kSplitTile = GINSIM_SPLIT_TILE;
constexpr int kSplitStep = 12 * 4;                      // bytes per step and run in the ring
// 96 KiB of ring + the tables, padded to more than half of the LDS so that a CU takes ONE workgroup (eight wavefronts, two
// per SIMD: a producer and a consumer)
constexpr size_t kSplitRing = (size_t)2 * kSplitTile * kSplitStep * kSplitRuns;
constexpr size_t kSplitLds = kSplitRing > 100 * 1024 ? kSplitRing : 100 * 1024;

// The inputs of a step of the consumer besides the normals (DESIGN_EXPERIMENTS "The consumer's four scalar waits").
// The truth rows of a tile are fetched by the producers, which idle most of a tile, into `truth` while they fill the tile's normals
// (one lane per number, NOT gated on the lane's run: the last workgroup may have no active lane in a producer wavefront; no row at
// or beyond n_noise <= n is read); the consumer reads its step's row with uniform-address LDS loads next to its ring reads.  The
// tile barrier orders these writes and reads exactly as it orders the normals.
struct SplitInputs {
    double truth[2][ginsim::kSplitTile][8];     // [stage][step of the tile][accel x y z, gyro x y z, forward speed, -]
};
typedef const SplitInputs __attribute__((address_space(3))) * split_inputs_ptr;

// -DGINSIM_STEP_TIMING (experiment builds only, build.py tag=): consumer wave 0 of every workgroup sums s_memtime deltas from the top
// of a step to the finished sensor sums (every memory wait of the step's inputs lies before that point) and over the whole step, and
// writes {input cycles, step cycles} once at its end; ginsim_step_timing copies the table out.
#ifdef GINSIM_STEP_TIMING
constexpr int kTimingGroups = 1024;
__device__ unsigned long long g_step_timing[kTimingGroups][2];
#define GINSIM_TIMING(...) __VA_ARGS__
#else
#define GINSIM_TIMING(...)
#endif

// PROD producer wavefronts per consumer wavefront: with two (768 threads, three wavefronts per SIMD, <= 168 registers) the
// steps of a tile alternate between the two producer groups.
// KEEP = false: a statistics-only launch (no series pointer set): the store code and its address registers are compiled out,
// which is what lets the ref_frame 0 consumer fit the 168 registers of three wavefronts per SIMD.
// VIB (round 5): the vibration term of Sim(env=...) in the wave-specialised kernel, for the batches where the plain vibration kernel
// runs with ONE wavefront per SIMD (<= 1024 wavefronts of runs: C2).  The three normals per sensor of a 'random' vibration are one
// more Philox block each and come from the producers -- the ring carries 18 floats per step and run instead of 12, in tiles of 4
// steps instead of 6 (the same 144 KB) --, a sinusoidal term is evaluated by the consumer; same operations on the same values as
// mc_kernel<..., VIB = true> (vibration_term), so the two kernels agree to the bit.
template <int RF, int ALGOS, bool WD, int PROD = 1, bool KEEP = true, bool VIB = false>
__global__ void __launch_bounds__(256 * (1 + PROD)) mc_kernel_split(const ginsim_mc_params a_in) {
    static_assert(!VIB || WD, "vibration: general sensor model");
    constexpr int kSplitTile = VIB ? 4 : ginsim::kSplitTile;
    ginsim_mc_params a = a_in;
    if (!KEEP) {
        a.out_accel = a.out_gyro = a.out_odo = nullptr;
        a.out_traj[0] = a.out_traj[1] = nullptr;
    }
    extern __shared__ float zring[];                    // [2 stages][T steps][12 normals][256 runs]
    constexpr bool FREE = (ALGOS & GINSIM_ALGO_FREE) != 0;
    constexpr bool ODO = (ALGOS & GINSIM_ALGO_ODO) != 0;
    constexpr int kStepFloats = (VIB ? 18 : 12) * kSplitRuns;          // 3072 (4608) floats per step
    const int lane = threadIdx.x & (kSplitRuns - 1);
    const bool producer = threadIdx.x >= kSplitRuns;
    const int pgroup = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 8)) - 1;     // which producer group (wave-uniform)
    const int64_t r = (int64_t)blockIdx.x * kSplitRuns + lane;
    const bool active = r < a.runs;
    const int64_t n = a.n, runs = a.runs, plane = n * runs;
    const bool keep_last = a.out_accel || a.out_gyro || a.out_odo;      // the last sample only exists as sensor output
    const int64_t n_noise = keep_last ? n : n - 1;
    const int64_t ntiles = (n_noise + kSplitTile - 1) / kSplitTile;
    const uint64_t grun = a.run_offset + (uint64_t)r;
    const RngKey key{(uint32_t)a.seed, (uint32_t)(a.seed >> 32), (uint32_t)grun, (uint32_t)(grun >> 32)};
    MathConsts mk;
    mk.init<(ALGOS != (GINSIM_ALGO_FREE | GINSIM_ALGO_ODO))>();     // the two-algorithm consumer would spill
    __shared__ uint32_t ntab[kNormalLdsWords];
    const NormalTables tab = fill_normal_tables(ntab, threadIdx.x, blockDim.x);
    static_assert(kSplitTile <= ginsim::kSplitTile, "SplitInputs::truth is sized by the longer tile");
    // the two-producer instantiations only (the headline's, C4's): in the one-producer ones the same source costs the compiler
    // 36 bytes of scratch per lane that nothing uses, and they keep the step as it was
    constexpr bool STAGED = PROD == 2;
    __shared__ SplitInputs in;
    const bool need_odo = ODO || a.out_odo;
    __syncthreads();


    if (producer) {
        const int sl = (int)threadIdx.x - kSplitRuns;       // the first 8 T lanes of the first producer group stage the truth
        for (int64_t i = 0; i <= ntiles; ++i) {
            if (STAGED && i < ntiles && sl < 8 * kSplitTile) {
                const int t = sl >> 3, c = sl & 7;
                const int64_t j = i * kSplitTile + t;
                if (j < n_noise) {
                    double v = 0.0;
                    if (c < 3) v = a.ref_accel[3 * j + c];
                    else if (c < 6) v = a.ref_gyro[3 * j + (c - 3)];
                    else if (c == 6 && need_odo) v = a.ref_odo[j];
                    in.truth[i & 1][t][c] = v;
                }
            }
            if (i < ntiles && active) {
                float* stage = zring + (i & 1) * (kSplitTile * kStepFloats);
#pragma unroll
                for (int t = 0; t < kSplitTile; ++t) {
                    const int64_t j = i * kSplitTile + t;
                    if (j < n_noise && (PROD == 1 || (t % PROD) == pgroup)) {
                        float z0[6], z1[6];
                        normal_pairs_f32<S_ACC_D_XY, 6>(key, (uint32_t)j, z0, z1, tab);
                        float* zb = stage + t * kStepFloats + lane;
#pragma unroll
                        for (int k = 0; k < 6; ++k) {
                            zb[(2 * k) * kSplitRuns] = z0[k];
                            zb[(2 * k + 1) * kSplitRuns] = z1[k];
                        }
                        if (VIB) {              // streams 10-13: one block per sensor with a 'random' vibration (wave-uniform)
                            const params_ptr kv = kernarg_params();
                            if (kv->vib_accel.type == GINSIM_VIB_RANDOM) {
                                float v0[2], v1[2];
                                normal_pairs_f32<S_ACC_VIB_XY, 2>(key, (uint32_t)j, v0, v1, tab);
                                zb[12 * kSplitRuns] = v0[0]; zb[13 * kSplitRuns] = v1[0]; zb[14 * kSplitRuns] = v0[1];
                            }
                            if (kv->vib_gyro.type == GINSIM_VIB_RANDOM) {
                                float v0[2], v1[2];
                                normal_pairs_f32<S_GYR_VIB_XY, 2>(key, (uint32_t)j, v0, v1, tab);
                                zb[15 * kSplitRuns] = v0[0]; zb[16 * kSplitRuns] = v1[0]; zb[17 * kSplitRuns] = v0[1];
                            }
                        }
                    }
                }
            }
            __syncthreads();
        }
        return;
    }

    const double dt = 1.0 / a.fs;
    const uint64_t call = a.ini_first + (uint64_t)r;
    const double* ini = a.ini + 10 * ((active && call < (uint64_t)a.n_ini) ? call : 0);
    Nav fi, od;
    if (FREE) nav_init<RF>(fi, ini, a.ini_has_g);
    if (ODO) nav_init<RF>(od, ini, a.ini_has_g);
    Vec3 da{0.0, 0.0, 0.0}, dg{0.0, 0.0, 0.0};
    Vec3 vpa{0.0, 0.0, 0.0}, vpg{0.0, 0.0, 0.0};
    if (VIB) {
        vpa = vibration_phase<S_ACC_VIB_PHASE>(&kernarg_params()->vib_accel, key);
        vpg = vibration_phase<S_GYR_VIB_PHASE>(&kernarg_params()->vib_gyro, key);
    }
    if (active) {
        if (FREE && a.out_traj[0]) store9(a.out_traj[0], plane, r, fi);
        if (ODO && a.out_traj[1]) store9(a.out_traj[1], plane, r, od);
    }
    GINSIM_TIMING(uint64_t tm_in = 0, tm_step = 0;)
    for (int64_t i = 0; i <= ntiles; ++i) {
        if (i >= 1 && active) {
            const float* stage = zring + ((i - 1) & 1) * (kSplitTile * kStepFloats);
#pragma unroll 1
            for (int t = 0; t < kSplitTile; ++t) {
                const int64_t j = (i - 1) * kSplitTile + t;
                if (j >= n_noise) break;
                const int64_t off = j * runs + r;
                const bool last = (j == n - 1);
                GINSIM_TIMING(const uint64_t tm0 = __builtin_amdgcn_s_memtime();)
                Vec3 cur_a, cur_g;
                ModelBatch ma{}, mg{};
                const double __attribute__((address_space(3))) * tr = nullptr;
                if constexpr (STAGED) {
                    // this step's truth row: the same LDS address in every lane (a broadcast); opaque per step so that the loads stay here
                    split_inputs_ptr q = (split_inputs_ptr)&in;
                    asm volatile("" : "+v"(q));
                    tr = q->truth[(i - 1) & 1][t];
                    cur_a = Vec3{tr[0], tr[1], tr[2]};
                    cur_g = Vec3{tr[3], tr[4], tr[5]};
                    // the eighteen coefficients of the simple model in ONE batch of scalar loads, asked for here and all due at the asm:
                    // taken where sense3 uses them they came in three batches, each behind a wait of its own
                    const params_ptr kp = kernarg_params();
                    ma = load_model(&kp->accel);
                    mg = load_model(&kp->gyro);
                    asm volatile("" :: "s"(ma.gm_a[0]), "s"(ma.gm_a[1]), "s"(ma.gm_a[2]), "s"(ma.gm_b[0]), "s"(ma.gm_b[1]), "s"(ma.gm_b[2]),
                                 "s"(ma.white[0]), "s"(ma.white[1]), "s"(ma.white[2]), "s"(mg.gm_a[0]), "s"(mg.gm_a[1]), "s"(mg.gm_a[2]),
                                 "s"(mg.gm_b[0]), "s"(mg.gm_b[1]), "s"(mg.gm_b[2]), "s"(mg.white[0]), "s"(mg.white[1]), "s"(mg.white[2]));
                } else {
                    cur_a = load3(as_uniform(a.ref_accel), j);
                    cur_g = load3(as_uniform(a.ref_gyro), j);
                }
                const float* zb = stage + t * kStepFloats + lane;
                double p0[6], p1[6];                  // z0 / z1 of streams 0..5
#pragma unroll
                for (int k = 0; k < 6; ++k) {
                    p0[k] = (double)zb[(2 * k) * kSplitRuns];
                    p1[k] = (double)zb[(2 * k + 1) * kSplitRuns];
                }
                Vec3 acc, gyr;
                if constexpr (STAGED) {
                    acc = sense3<WD>(cur_a, &ma, da, Vec3{p0[0], p1[0], p0[1]}, Vec3{p1[1], p0[2], p1[2]});
                    gyr = sense3<WD>(cur_g, &mg, dg, Vec3{p0[3], p1[3], p0[4]}, Vec3{p1[4], p0[5], p1[5]});
                    // the drift update is due HERE: left alone it sinks to the bottom of the step, and the twelve coefficients and six
                    // normals it needs stay in registers through the whole mechanisation
                    asm volatile("" : "+v"(da.x), "+v"(da.y), "+v"(da.z), "+v"(dg.x), "+v"(dg.y), "+v"(dg.z));
                } else {
                    const params_ptr kp = kernarg_params();
                    acc = sense3<WD>(cur_a, &kp->accel, da, Vec3{p0[0], p1[0], p0[1]}, Vec3{p1[1], p0[2], p1[2]});
                    gyr = sense3<WD>(cur_g, &kp->gyro, dg, Vec3{p0[3], p1[3], p0[4]}, Vec3{p1[4], p0[5], p1[5]});
                }
                GINSIM_TIMING(
                    asm volatile("" : "+v"(acc.x), "+v"(acc.y), "+v"(acc.z), "+v"(gyr.x), "+v"(gyr.y), "+v"(gyr.z));
                    tm_in += __builtin_amdgcn_s_memtime() - tm0;)
                if (VIB) {              // added last, as pathgen.py:500, 562 do
                    const params_ptr kv = kernarg_params();
                    double va[3] = {0.0, 0.0, 0.0}, vg[3] = {0.0, 0.0, 0.0};
                    if (kv->vib_accel.type == GINSIM_VIB_RANDOM) {
                        va[0] = (double)zb[12 * kSplitRuns]; va[1] = (double)zb[13 * kSplitRuns]; va[2] = (double)zb[14 * kSplitRuns];
                    }
                    if (kv->vib_gyro.type == GINSIM_VIB_RANDOM) {
                        vg[0] = (double)zb[15 * kSplitRuns]; vg[1] = (double)zb[16 * kSplitRuns]; vg[2] = (double)zb[17 * kSplitRuns];
                    }
                    acc = vibration_term(acc, &kv->vib_accel, va[0], va[1], va[2], (uint32_t)j, vpa);
                    gyr = vibration_term(gyr, &kv->vib_gyro, vg[0], vg[1], vg[2], (uint32_t)j, vpg);
                }
                if (a.out_accel) store3(a.out_accel, plane, off, acc);
                if (a.out_gyro) store3(a.out_gyro, plane, off, gyr);
                double odo = 0.0;
                if (need_odo) {
                    double z0, z1;
                    normal_pair(key, S_ODO, (uint32_t)j, z0, z1, tab);
                    const params_ptr kq = kernarg_params();
                    odo = kq->odo_scale * (STAGED ? tr[6] : as_uniform(a.ref_odo)[j]) + kq->odo_stdv * z0;
                    if (a.out_odo) a.out_odo[off] = odo;
                }
                if (last) break;
                const bool resync = ((j + 1) & (kTrigResync - 1)) == 0;
                if (FREE) {
                    nav_step<RF, false>(fi, gyr, acc, 0.0, dt, a.earth_rot, resync, mk);
                    if (a.out_traj[0]) store9(a.out_traj[0], plane, off + runs, fi);
                }
                if (ODO) {
                    nav_step<RF, true>(od, gyr, acc, odo, dt, a.earth_rot, resync, mk);
                    if (a.out_traj[1]) store9(a.out_traj[1], plane, off + runs, od);
                }
                GINSIM_TIMING(tm_step += __builtin_amdgcn_s_memtime() - tm0;)
            }
        }
        __syncthreads();
    }
    GINSIM_TIMING(
        if (threadIdx.x == 0 && blockIdx.x < kTimingGroups) {
            unsigned long long* q = g_step_timing[blockIdx.x];
            q[0] = tm_in; q[1] = tm_step;
        })
    if (active) {
        if (FREE && a.out_end[0]) store_end(a.out_end[0], runs, r, fi);
        if (ODO && a.out_end[1]) store_end(a.out_end[1], runs, r, od);
        if (RF == 0) {
            if (FREE && a.out_end_ned[0]) store_end_ned(a.out_end_ned[0], runs, r, fi);
            if (ODO && a.out_end_ned[1]) store_end_ned(a.out_end_ned[1], runs, r, od);
        }
    }
}

// Launch geometry.  The kernel is VALU-bound and every wavefront of a launch does the same amount of work,
// so the only thing that matters is that wavefronts are spread evenly over the 1024 SIMDs.  Measured on
// MI355X: with 64-thread workgroups the dispatcher, depending on what ran before, doubles up ~6 % of the
// SIMDs and leaves as many idle (7.2 ms instead of 4.2 ms at 65 536 runs).  256-thread workgroups put one
// wavefront on each SIMD of a CU, and a dynamic-LDS reservation (never touched by the kernel) caps the
// workgroups per CU at k = 1 (<= 1024 wavefronts) or 2 (the VGPR budget allows no more), so every SIMD
// holds exactly k wavefronts until the tail.
constexpr int kBlock = 256;
constexpr size_t kLdsPerCu = 160 * 1024;

// 1 = wave-specialised kernel (mc_kernel_split), 0 = one wavefront does everything for its 64 runs (mc_kernel)
int mc_variant(const ginsim_mc_params& p) {
    if (any_psd_vibration(p)) return 0;
    if (any_vibration(p)) {
        // the vibration term lives in the plain kernels, except where they would run with one wavefront per SIMD: a single free
        // integration, generated sensors, at most 1024 wavefronts of runs (C2's shape) -> mc_kernel_split<..., VIB = true>
        const char* env = getenv("GINSIM_SPLIT_VIB");        // read per call: the tests run both kernels in one process
        return (env ? atoi(env) : 1) != 0 && split_policy() != 0 && p.algo_mask == GINSIM_ALGO_FREE && !p.given_sensors && p.block_threads == 0 &&
               !p.wave_trace && p.n >= 2 && !(p.out_proc[0] || p.out_proc[1]) && (p.runs + kWave - 1) / kWave <= 1024;
    }
    if (!(p.algo_mask & GINSIM_ALGO_FREE) || p.given_sensors || p.block_threads != 0 || p.wave_trace || p.n < 2) return 0;
    if (p.out_proc[0] || p.out_proc[1]) return 0;      // online process statistics live in the plain kernel
    const int pol = split_policy();
    if (pol >= 0) return pol != 0;
    // one algorithm: three wavefronts per SIMD (a consumer and two producers) beat the plain kernel's two at every size
    // (131 072 runs: 2.71 against 3.06 ms, 262 144: 5.76 against 6.13); two algorithms: only while the plain kernel
    // cannot fill the SIMDs with a second wavefront
    if (p.algo_mask == GINSIM_ALGO_FREE && p.ref_frame == 1) return 1;      // the variants with two producer groups (launch3)
    return (p.runs + kWave - 1) / kWave <= 1024 ? 1 : 0;
}

// name != nullptr: write the kernel's name (as rocprofv3 reports it, without arguments) instead of launching -- what
// ginsim_mc_kernel_name returns, so that profiles and the bench attribute to the instantiation that really runs
#define GINSIM_NAME_OR(fmt, ...)                         \
    if (name) {                                          \
        snprintf(name, cap, fmt, __VA_ARGS__);           \
        return hipSuccess;                               \
    }
static const char* tf(bool b) { return b ? "true" : "false"; }

template <int RF, int ALGOS, bool WD>
static hipError_t launch3(const ginsim_mc_params& p, hipStream_t stream, char* name, size_t cap, double* about) {
    const int tb = p.block_threads > 0 ? p.block_threads : kBlock;
    const int64_t waves = (p.runs + kWave - 1) / kWave;
    if constexpr ((ALGOS & GINSIM_ALGO_FREE) != 0) {
        if (mc_variant(p) == 1) {
            // one algorithm in the ECEF-free frame fits 168 registers: two producer wavefronts per consumer, three wavefronts
            // per SIMD (C2: 1.48 -> 1.41 ms); ref_frame 0 would spill 76-140 B per lane
            constexpr int PROD = (ALGOS == GINSIM_ALGO_FREE && RF == 1) ? 2 : 1;
            static const int prod = [] { const char* e = getenv("GINSIM_SPLIT_PROD"); return e ? atoi(e) : PROD; }();
            const dim3 sgrid((unsigned)((p.runs + kSplitRuns - 1) / kSplitRuns));
            if constexpr (ALGOS == GINSIM_ALGO_FREE && WD) {
                if (any_vibration(p)) {         // one producer group: the consumer with the vibration term wants more than 168 registers
                    constexpr size_t lds = (size_t)2 * 4 * 18 * 4 * kSplitRuns;
                    GINSIM_NAME_OR("ginsim::mc_kernel_split<%d, %d, %s, 1, true, true>", RF, ALGOS, tf(WD))
                    static PerDeviceOnce oncev;
                    oncev.run([] {
                        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&mc_kernel_split<RF, ALGOS, WD, 1, true, true>),
                                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
                    });
                    hipLaunchKernelGGL((mc_kernel_split<RF, ALGOS, WD, 1, true, true>), sgrid, dim3(512), lds, stream, p);
                    return hipGetLastError();
                }
            }
            if constexpr (ALGOS == GINSIM_ALGO_FREE && RF == 0) {     // nothing kept: two producer groups fit here too
                const bool keep = p.out_accel || p.out_gyro || p.out_odo || p.out_traj[0] || p.out_traj[1];
                if (!keep && prod != 1) {
                    GINSIM_NAME_OR("ginsim::mc_kernel_split<%d, %d, %s, 2, false, false>", RF, ALGOS, tf(WD))
                    static PerDeviceOnce once2;
                    once2.run([] {
                        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&mc_kernel_split<RF, ALGOS, WD, 2, false>),
                                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)kSplitLds);
                    });
                    hipLaunchKernelGGL((mc_kernel_split<RF, ALGOS, WD, 2, false>), sgrid, dim3(768), kSplitLds, stream, p);
                    return hipGetLastError();
                }
            }
            const bool two = prod == PROD && PROD > 1;
            GINSIM_NAME_OR("ginsim::mc_kernel_split<%d, %d, %s, %d, true, false>", RF, ALGOS, tf(WD), two ? PROD : 1)
            static PerDeviceOnce once;
            once.run([] {
                (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&mc_kernel_split<RF, ALGOS, WD, 1>),
                                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)kSplitLds);
                (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&mc_kernel_split<RF, ALGOS, WD, PROD>),
                                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)kSplitLds);
            });
            if (two)
                hipLaunchKernelGGL((mc_kernel_split<RF, ALGOS, WD, PROD>), sgrid, dim3(256 * (1 + PROD)), kSplitLds, stream, p);
            else
                hipLaunchKernelGGL((mc_kernel_split<RF, ALGOS, WD, 1>), sgrid, dim3(512), kSplitLds, stream, p);
            return hipGetLastError();
        }
    }
    const int per_cu = waves <= 1024 ? 1 : 2;
    // strictly more than 1/(k+1) of the LDS so that k+1 workgroups do not fit: 81 KB (k = 1), 54 KB (k = 2)
    const size_t lds = p.block_threads > 0 ? 0 : kLdsPerCu / (per_cu + 1) + 1024;
    const dim3 grid((unsigned)((p.runs + tb - 1) / tb)), block(tb);
    if constexpr (ALGOS == GINSIM_ALGO_FREE || ALGOS == GINSIM_ALGO_ODO) {
        if (p.out_proc[ALGOS == GINSIM_ALGO_FREE ? 0 : 1]) {
            const bool ned = RF == 0 && p.proc_pos_ned;
            // the variants whose sums are shifted per launch (Proc, SHIFT 2): the nine shifts are written first, on the same stream
            auto write_shift = [&](bool vib) -> hipError_t {
                if (!vib && !(RF == 0 && ALGOS == GINSIM_ALGO_FREE)) return hipSuccess;
                if (!about) return hipErrorInvalidValue;
                if (ned) hipLaunchKernelGGL((proc_shift_kernel<RF, RF == 0>), dim3(1), dim3(1), 0, stream, p, about);
                else hipLaunchKernelGGL((proc_shift_kernel<RF, false>), dim3(1), dim3(1), 0, stream, p, about);
                return hipGetLastError();
            };
            // ... unless the caller states that the runs start on the truth (nine zero shifts): the plain sums
            constexpr bool kPlainForm = RF == 0 && ALGOS == GINSIM_ALGO_FREE;
            const bool plain = kPlainForm && p.proc_plain_sums != 0 && !any_vibration(p);
            if constexpr (WD) {                     // the general sensor model: every statistics form, vibration included
                if (any_vibration(p)) {
                    GINSIM_NAME_OR("ginsim::mc_kernel<%d, %d, false, true, %d, true>", RF, ALGOS, ned ? 2 : 1)
                    if (hipError_t e = write_shift(true); e != hipSuccess) return e;
                    if (ned) hipLaunchKernelGGL((mc_kernel<RF, ALGOS, false, true, RF == 0 ? 2 : 1, true>), grid, block, lds, stream, p, about);
                    else hipLaunchKernelGGL((mc_kernel<RF, ALGOS, false, true, 1, true>), grid, block, lds, stream, p, about);
                    return hipGetLastError();
                }
                GINSIM_NAME_OR("ginsim::mc_kernel<%d, %d, false, true, %d, false>", RF, ALGOS, (ned ? 2 : 1) + (plain ? 2 : 0))
                if constexpr (kPlainForm) {
                    if (plain) {
                        if (ned) hipLaunchKernelGGL((mc_kernel<RF, ALGOS, false, true, 4>), grid, block, lds, stream, p, about);
                        else hipLaunchKernelGGL((mc_kernel<RF, ALGOS, false, true, 3>), grid, block, lds, stream, p, about);
                        return hipGetLastError();
                    }
                }
                if (hipError_t e = write_shift(false); e != hipSuccess) return e;
                if (ned) hipLaunchKernelGGL((mc_kernel<RF, ALGOS, false, true, RF == 0 ? 2 : 1>), grid, block, lds, stream, p, about);
                else hipLaunchKernelGGL((mc_kernel<RF, ALGOS, false, true, 1>), grid, block, lds, stream, p, about);
                return hipGetLastError();
            } else {                                // the simple model (every standard IMU grade), statistics in the state's own units
                GINSIM_NAME_OR("ginsim::mc_kernel<%d, %d, false, false, %d, false>", RF, ALGOS, plain ? 3 : 1)
                if constexpr (kPlainForm) {
                    if (plain) {
                        hipLaunchKernelGGL((mc_kernel<RF, ALGOS, false, false, 3>), grid, block, lds, stream, p, about);
                        return hipGetLastError();
                    }
                }
                if (hipError_t e = write_shift(false); e != hipSuccess) return e;
                hipLaunchKernelGGL((mc_kernel<RF, ALGOS, false, false, 1>), grid, block, lds, stream, p, about);
                return hipGetLastError();
            }
        }
    }
    if constexpr (WD) {
        if (any_vibration(p)) {
            GINSIM_NAME_OR("ginsim::mc_kernel<%d, %d, false, true, 0, true>", RF, ALGOS)
            hipLaunchKernelGGL((mc_kernel<RF, ALGOS, false, true, 0, true>), grid, block, lds, stream, p, about);
            return hipGetLastError();
        }
    }
    GINSIM_NAME_OR("ginsim::mc_kernel<%d, %d, false, %s, 0, false>", RF, ALGOS, tf(WD))
    hipLaunchKernelGGL((mc_kernel<RF, ALGOS, false, WD>), grid, block, lds, stream, p, about);
    return hipGetLastError();
}

template <int RF, int ALGOS>
static hipError_t launch2(const ginsim_mc_params& p, hipStream_t stream, char* name, size_t cap, double* about) {
    if (p.given_sensors) {
        if constexpr (ALGOS != 0) {
            GINSIM_NAME_OR("ginsim::mc_kernel<%d, %d, true, false, 0, false>", RF, ALGOS)
            const int tb = p.block_threads > 0 ? p.block_threads : kBlock;
            const int64_t waves = (p.runs + kWave - 1) / kWave;
            const int per_cu = waves <= 1024 ? 1 : 2;
            const size_t lds = p.block_threads > 0 ? 0 : kLdsPerCu / (per_cu + 1) + 1024;
            hipLaunchKernelGGL((mc_kernel<RF, ALGOS, true, false>), dim3((unsigned)((p.runs + tb - 1) / tb)), dim3(tb), lds, stream, p, about);
            return hipGetLastError();
        }
        return hipErrorInvalidValue;        // given sensors without an algorithm: rejected by the C ABI
    }
    // the simple-model variant of the two-algorithm ref_frame 0 kernels is the one instantiation that spills: use the general one
    constexpr bool kSimpleFits = !(RF == 0 && ALGOS == (GINSIM_ALGO_FREE | GINSIM_ALGO_ODO));
    // online process statistics: the simple model where the launch has no NED record to keep (round 6: that instantiation no longer
    // spills -- 245 registers -- and saves the general model's 30 selects per step; with the NED record it would, 36 B per lane)
    const bool proc = p.out_proc[0] || p.out_proc[1];
    const bool general_ps = proc && getenv("GINSIM_PS_GENERAL") != nullptr;       // read per call: the tests compare the two kernels bit for bit
    if (any_white_drift(p) || any_vibration(p) || !kSimpleFits || (proc && p.ref_frame == 0 && p.proc_pos_ned) || general_ps)
        return launch3<RF, ALGOS, true>(p, stream, name, cap, about);
    if constexpr (kSimpleFits) return launch3<RF, ALGOS, false>(p, stream, name, cap, about);
    return hipErrorInvalidValue;
}

template <int RF>
static hipError_t launch1(const ginsim_mc_params& p, hipStream_t stream, char* name, size_t cap, double* about) {
    switch (p.algo_mask) {
        case 0: return launch2<RF, 0>(p, stream, name, cap, about);      // sensors only (Sim without an algorithm)
        case GINSIM_ALGO_FREE: return launch2<RF, GINSIM_ALGO_FREE>(p, stream, name, cap, about);
        case GINSIM_ALGO_ODO: return launch2<RF, GINSIM_ALGO_ODO>(p, stream, name, cap, about);
        default: return launch2<RF, GINSIM_ALGO_FREE | GINSIM_ALGO_ODO>(p, stream, name, cap, about);
    }
}

hipError_t launch_mc(const ginsim_mc_params& p, hipStream_t stream, char* name, size_t cap, double* about) {
    return p.ref_frame == 1 ? launch1<1>(p, stream, name, cap, about) : launch1<0>(p, stream, name, cap, about);
}

}  // namespace ginsim

#ifdef GINSIM_STEP_TIMING
// experiment builds only: the timing table of the last wave-specialised launch, [groups][2]; returns the number of rows copied
extern "C" int ginsim_step_timing(unsigned long long* out, int groups) {
    if (groups > ginsim::kTimingGroups) groups = ginsim::kTimingGroups;
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(ginsim::g_step_timing), sizeof(unsigned long long) * 2 * groups) != hipSuccess) return -1;
    return groups;
}
#endif

