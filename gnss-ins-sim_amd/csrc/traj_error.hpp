// What the kernels that read kept trajectories ACROSS the runs share (error_curve.hip, error_quantile.hip's radial_keys_kernel,
// error_cov.hip; the origin lookup also with stats.hip's process kernel): the unit of work, the origin of a run in the fp32
// displacement series, the error of the selected quantity, and the cut of the run axis into slices.
//
// The unit of work is a WAVEFRONT: one requested sample and one slice of the run axis.  Its lanes stride along the runs (the
// trajectories are [9][n][runs], so the row of one (component, sample) is contiguous across runs); the truth row and the sample
// index are wave-uniform (scalar loads).  No LDS, no barrier, no atomics.  What a kernel accumulates (Mom, Cov, keys), how many
// runs a lane takes per step and its final kernel are its own.
#pragma once
#include "moments.hpp"
#include "launch.hpp"

namespace ginsim {

constexpr int kUnitBlock = 256;                     // four wavefronts, each with its own (sample, slice)
constexpr int kUnitWaves = kUnitBlock / 64;
constexpr int64_t kTargetWaves = 8192;              // 256 CUs x 4 SIMDs x 8 wavefronts

// the sample indices are the same for every lane of a wavefront: a scalar load, as the truth row (uniform_ref, moments.hpp)
typedef const int64_t __attribute__((address_space(4))) * uniform_idx;

// The slices of the run axis for `m` samples of `runs` runs: one wavefront per sample when there are many samples, else enough
// slices to fill the device, at most max_parts.  A slice holds at least one step of a wavefront, runs_per_step runs.  It depends
// on (runs, m) alone: the same shape takes the same path and gives the same bytes at every launch.
inline int run_slices(int64_t runs, int64_t m, int runs_per_step, int max_parts) {
    const int64_t most = (runs + runs_per_step - 1) / runs_per_step;
    int64_t want = (kTargetWaves + m - 1) / m;
    if (want > most) want = most;
    if (want > max_parts) want = max_parts;
    return (int)(want < 1 ? 1 : want);
}

inline unsigned unit_blocks(int64_t m, int parts) { return (unsigned)((m * parts + kUnitWaves - 1) / kUnitWaves); }

// the unit of the calling wavefront; units >= m * parts have nothing to do (wave-uniform)
__device__ __forceinline__ int64_t wave_unit() {
    return (int64_t)blockIdx.x * kUnitWaves + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
}

// Unit `unit` < m * parts: sample s of the m requested ones (index j of the series).  Its slice, part = (int)(unit - s * parts) of
// `parts`, is formed in the kernels, next to the run loop that scales it: formed here, the two-runs-per-load curve kernels came out
// with 16 to 22 more VGPRs and the fp32 one with an occupancy of 3 instead of 4.
struct WorkUnit {
    int64_t s, j, plane;                            // plane: the stride between the components of the series
    uniform_ref truth;                              // row 9 * j is the truth of the sample

    __device__ __forceinline__ WorkUnit(int64_t unit, const double* ref, int64_t n, int64_t runs, const int64_t* samples, int parts) {
        s = unit / parts;
        j = samples ? ((uniform_idx)(uintptr_t)samples)[s] : s;
        plane = n * runs;
        truth = (uniform_ref)(uintptr_t)ref;
    }
};

// the initial position of run r of the launch: the rule of the Monte-Carlo kernels (launch.hpp, ProcOrigin); org.table != nullptr
__device__ __forceinline__ void run_origin(const ProcOrigin& org, int64_t r, double (&o3)[3]) {
    const uint64_t call = org.ini_first + (uint64_t)r;
    const double* row = org.table + 3 * (call < (uint64_t)org.n_ini ? call : 0);
    o3[0] = row[0]; o3[1] = row[1]; o3[2] = row[2];
}

// The error of run r against the truth (t0, t1, t2) of the selected quantity, from its three plane values: which = 0 position
// (planes 3..5, the origin added in fp64 where there is a table), 1 velocity (planes 6..8); formed by sample_error (moments.hpp).
// NED: the position error in local NED metres (lla_error_ned), a template parameter so that the plain form does not carry the
// registers of the geodetic conversion; it has no effect on the velocity.
template <bool NED>
__device__ __forceinline__ void quantity_error(double a0, double a1, double a2, double t0, double t1, double t2, int which,
                                               const ProcOrigin& org, int64_t r, double (&e3)[3]) {
    double x[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, t[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, e[9];
    if (which) {                                    // wave-uniform
        x[6] = a0; x[7] = a1; x[8] = a2;
        t[6] = t0; t[7] = t1; t[8] = t2;
        sample_error(x, t, 0, e);
        e3[0] = e[6]; e3[1] = e[7]; e3[2] = e[8];
    } else {
        double o3[3] = {0.0, 0.0, 0.0};
        if (org.table) run_origin(org, r, o3);
        x[3] = a0 + o3[0]; x[4] = a1 + o3[1]; x[5] = a2 + o3[2];
        t[3] = t0; t[4] = t1; t[5] = t2;
        sample_error(x, t, NED ? 1 : 0, e);
        e3[0] = e[3]; e3[1] = e[4]; e3[2] = e[5];
    }
}

}  // namespace ginsim
