// The host interface between the kernel files and the C ABI glue (ginsim_api.hip and its api_*.hip units): every launcher and
// host helper that one file defines and another calls, grouped by the file that defines it, and the structs that describe a launch
// to them (LooseLaunch, TrajView).  Every defining file includes it, and the library is linked without undefined symbols, so a signature that drifts
// from its definition fails the build.  (allan.hpp, comm.hpp and placed.hpp are the same thing for their files.)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include "ginsim.h"

namespace ginsim {

// ginsim_api.hip
void set_error(const char* fmt, ...);

// mc_kernel.hip
hipError_t launch_mc(const ginsim_mc_params& p, hipStream_t stream, char* name, size_t cap, double* proc_about);      // name: report, do not launch
int mc_variant(const ginsim_mc_params& p);

// mc_kernel_f32.hip
hipError_t launch_mc_f32(const ginsim_mc_params& p, float* truth32, hipStream_t stream, char* name, size_t cap);
size_t mc_f32_truth_bytes(const ginsim_mc_params& p);
int mc_variant_f32(const ginsim_mc_params& p);

// series.hip
bool series_path_applies(const ginsim_mc_params& p);
int series_pass_b(const ginsim_mc_params& p);
int64_t series_chunks(const ginsim_mc_params& p, int32_t* L_out);
hipError_t launch_series(const ginsim_mc_params& p, double* carry, hipStream_t stream);

// inclinometer.hip
hipError_t launch_incl(const ginsim_mc_params& p, const ginsim_incl_params& b, hipStream_t stream, char* name, size_t cap);
int incl_variant(const ginsim_mc_params& p);

// One launch of the loose family, as api_mc.hip (loose_entry) describes it to the family's launcher.
struct LooseLaunch {
    const ginsim_mc_params* mc;                 // the two base blocks, checked
    const ginsim_loose_params* b;
    const ginsim_loose_cons_params* cons;       // the family blocks, checked: NULL when absent or degenerate (cons_m == 0,
    const ginsim_loose_mag_params* mag;         // mag_every == 0); launch_loose (api_mc.hip) picks the family from them
    const ginsim_loose_scale_params* scale;
    const ginsim_loose_still_params* still;     // NULL when absent or degenerate (still_mask == 0)
    char* name; size_t cap;                     // name != NULL: report the kernel's name into name[cap], do not launch
    const int64_t* stamp;                       // DEVICE copies of b->gps_stamp, b->gps_visible and cons->cons_sample
    const int32_t* visible;
    const int64_t* samples;
    hipStream_t stream;
    bool all;                                   // two or three of mag, scale and still are left: the combined family (ins_loose_all.hip)
    bool all_cons;                              // cons with any of mag, scale and still, or none: ins_loose_all_cons.hip (ginsim_loose_all_cons.h)
    const double* scale_truth;                  // all_cons: the DEVICE truth of the scale factor per run, or NULL
};

// ins_loose.hip, ins_loose_aided.hip (b->aid_mask != 0), ins_loose_cons.hip (cons), ins_loose_mag.hip (mag), ins_loose_scale.hip
// (scale; b->aid_mask has bit 0), ins_loose_still.hip (still): each chooses its <RF, flag> and launches, or names, one instantiation of its kernel
hipError_t launch_loose_plain(const LooseLaunch& L);
hipError_t launch_loose_aided(const LooseLaunch& L);
hipError_t launch_loose_cons(const LooseLaunch& L);
hipError_t launch_loose_mag(const LooseLaunch& L);
hipError_t launch_loose_scale(const LooseLaunch& L);
hipError_t launch_loose_still(const LooseLaunch& L);
// ins_loose_all.hip (L.all; 15 states) and ins_loose_all16.hip (with L.scale; 16 states): the three blocks L has, an absent one all
// zero, as the one ginsim_loose_all_params the kernel takes; b->aid_mask has bit 0 where L.scale is set
hipError_t launch_loose_all(const LooseLaunch& L);
hipError_t launch_loose_all16(const LooseLaunch& L);
// ins_loose_all_cons.hip (L.all_cons; 15 states) and ins_loose_all_cons16.hip (with L.scale; 16 states): the combined lane with
// checkpoints, then launch_cons_final
hipError_t launch_loose_all_cons(const LooseLaunch& L);
hipError_t launch_loose_all_cons16(const LooseLaunch& L);
// ins_loose_cons.hip: cons_final_kernel, out_cons = the sum of the `waves` partial records of cons_work
hipError_t launch_cons_final(const ginsim_loose_cons_params& c, int64_t waves, hipStream_t stream);
int loose_variant(const ginsim_mc_params& p);

// aux_sensors.hip
hipError_t launch_aux(const ginsim_aux_params& p, hipStream_t s);

// magcal.hip
hipError_t launch_magcal(const ginsim_magcal_params& p, hipStream_t s);

// vib_psd.hip
size_t vib_psd_scratch_bytes(int64_t period, int64_t runs);
int launch_vib_psd(int device, hipStream_t stream, const double* amp, int64_t period, int64_t runs, uint64_t run_offset, uint64_t seed,
                   int sensor, int halve, void* scratch, double* out);
void vib_psd_drop_plans(hipStream_t stream);

// rng_probe.hip
hipError_t launch_rng_probe(uint64_t seed, uint64_t run, uint32_t stream, int64_t count, double* z0, double* z1,
                            uint32_t* words, hipStream_t stream_h);
hipError_t launch_normal_transform(const uint32_t* words, int64_t count, double* z0, double* z1, hipStream_t s);

// layout.hip
hipError_t launch_aos_to_soa(const double* src, double* dst, int64_t R, int64_t n, int C, hipStream_t s);
hipError_t launch_runs_to_series(const double* in, double* out, int C, int64_t n, int64_t R, hipStream_t s);
hipError_t launch_gather_runs(const double* series, int C, int64_t n, int64_t runs, const int64_t* ids, int nsel,
                              double* out, hipStream_t s);
hipError_t launch_gather_series(const double* series, int C, int64_t n, const int64_t* ids, int nsel, double* out, hipStream_t s);
hipError_t launch_gather_runs_f32(const float* series, int C, int64_t n, int64_t runs, const int64_t* ids, int nsel,
                                  double* out, hipStream_t s);

// selftest.hip
hipError_t launch_pattern_fill(void* p, uint64_t words, uint32_t tag, hipStream_t s);
hipError_t launch_pattern_check(const void* p, uint64_t words, uint32_t tag, unsigned long long* out, hipStream_t s);
hipError_t launch_digest(const void* p, uint64_t words, unsigned long long* out, hipStream_t s);
hipError_t launch_first_xcc(uint32_t* out, hipStream_t s);

// The series of the fp32 kernel hold the DISPLACEMENT from the run's initial position in their position planes
// (ginsim_mc_params.precision), so the position of a sample is origin[run's initial state] + displacement, formed in fp64;
// everything after that (errors, moments) is the fp64 arithmetic of the double version.
struct ProcOrigin {
    const double* table;    // device [n_ini][3]: ECEF (ref_frame 1) or LLA (ref_frame 0) of every initial state, or nullptr (fp64 series)
    int64_t n_ini;
    uint64_t ini_first;     // the run's initial state is row (ini_first + run < n_ini ? ini_first + run : 0), as in the MC kernels
};

// Kept trajectories as the kernels that read them across the runs take them (stats.hip's process kernel, error_curve.hip,
// error_quantile.hip, error_cov.hip): one launcher per family, which picks the kernel's precision from f32.
struct TrajView {
    const void* traj;           // device [9][n][runs], double or (f32) float
    int f32;
    const double* ref;          // device [n][9], the truth
    int64_t n, runs;
    const int64_t* samples;     // device: the m sample indices, or NULL: every sample (m == n)
    int64_t m;
    ProcOrigin org;             // f32: the origin table; else {nullptr, 0, 0}
};

// stats.hip
size_t stats_scratch_bytes(int64_t runs);
int stats_blocks(int64_t runs);
hipError_t launch_end_stats(const double* end_err, int64_t runs, void* scratch, hipStream_t s);
void stats_merge_host(const ginsim_stats* parts, int nparts, ginsim_stats* out);
hipError_t launch_process_stats(const TrajView& v, int64_t j0, int pos_ned, int run_major, double* out, hipStream_t s);     // v.samples, v.m unused

// error_curve.hip
size_t error_curve_scratch_bytes(const TrajView& v);
hipError_t launch_error_curve(const TrajView& v, int pos_ned, void* scratch, hipStream_t s);
void curve_merge_host(const double* parts, int nparts, int64_t m, double* out);

// error_quantile.hip
hipError_t launch_radial_keys(const TrajView& v, int which, int pos_ned, double* keys, int64_t row_stride, int64_t col0, hipStream_t s);
hipError_t launch_quantile_rows(const double* keys, int64_t rows, int64_t len, int64_t row_stride, const double* probs, int q,
                                double* out, double* count, hipStream_t s);

// error_cov.hip
size_t error_cov_scratch_bytes(const TrajView& v);
hipError_t launch_error_cov(const TrajView& v, int which, int pos_ned, void* scratch, hipStream_t s);
void cov_merge_host(const double* parts, int nparts, int64_t m, double* out);

// Predicates on a parameter block that the dispatch of several files asks.
inline int split_policy() {        // GINSIM_SPLIT=0 / 1 forces the plain / wave-specialised kernel (A/B measurements)
    static const int v = [] { const char* e = getenv("GINSIM_SPLIT"); return e ? atoi(e) : -1; }();
    return v;
}

inline bool any_vibration(const ginsim_mc_params& p) { return p.vib_accel.type != GINSIM_VIB_NONE || p.vib_gyro.type != GINSIM_VIB_NONE; }
// a 'psd' vibration (ABI 8) is a series read per lane and sample: the lane-per-run kernel has it, nothing else
inline bool any_psd_vibration(const ginsim_mc_params& p) { return p.vib_accel.type == GINSIM_VIB_PSD || p.vib_gyro.type == GINSIM_VIB_PSD; }

// white-drift axes or a constant bias anywhere: the general sensor model (WD = true kernels)
inline bool any_white_drift(const ginsim_mc_params& p) {
    bool f = false;
    for (int k = 0; k < 3; ++k)
        f = f || p.accel.white_drift[k] || p.gyro.white_drift[k] || p.accel.bias[k] != 0.0 || p.gyro.bias[k] != 0.0;
    return f;
}

}  // namespace ginsim
