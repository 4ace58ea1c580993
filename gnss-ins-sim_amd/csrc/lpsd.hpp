// Planning code and launch interface of the decimating octave cascade (lpsd.hip) for the C ABI glue (api_series.hip).
// As in psd.hpp, everything a call's shape depends on is host arithmetic in this header: ginsim_lpsd launches from lpsd_plan_levels
// and ginsim_lpsd_plan reports it.  The Welch estimate of every level is psd.hpp's, unchanged.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "psd.hpp"

namespace ginsim {

constexpr int kHalfbandTaps = 27, kHalfbandM = 13;
constexpr int kLpsdMaxLevels = 32;                          // GINSIM_LPSD_MAX_LEVELS

// one workgroup of decimate2_kernel: kDecTile outputs from 2 kDecTile + 25 consecutive inputs, kDecTile / kDecThreads per lane
constexpr int kDecThreads = 256, kDecTile = 1024;
// the tiles of a series are a launch's grid x dimension
constexpr int64_t kDecMaxTiles = 0x7FFFFFFF;

// outputs of one decimation: only valid ones, no padding
constexpr int64_t decimate2_outputs(int64_t n) { return n >= kHalfbandTaps ? (n - kHalfbandTaps) / 2 + 1 : 0; }
constexpr int64_t decimate2_tiles(int64_t n_out) { return (n_out + kDecTile - 1) / kDecTile; }

// What one cascade runs: level j has n[j] samples at fs / 2^j, the Welch shape S[j] and reports the bins
// first_bin[j] .. first_bin[j] + bins[j] - 1 of its estimate; the output has level levels - 1 first.
struct LpsdLevels {
    int32_t levels;                                         // J + 1
    int32_t nbins;                                          // all reported bins
    int64_t n[kLpsdMaxLevels];
    PsdShape S[kLpsdMaxLevels];
    int32_t first_bin[kLpsdMaxLevels], bins[kLpsdMaxLevels];
};

// on checked arguments (psd_plan_shape's, and 1 <= min_segments <= the segments of level 0).  Levels past 0 are shorter than
// level 0, so their parts and records are fewer than its own: what the glue has held level 0 to holds for all.
inline LpsdLevels lpsd_plan_levels(int64_t n, int32_t L, int32_t D, int64_t min_segments) {
    LpsdLevels P;
    P.levels = 0;
    for (int64_t nj = n; P.levels < kLpsdMaxLevels && nj >= L && (nj - L) / D + 1 >= min_segments; nj = decimate2_outputs(nj)) {
        P.n[P.levels] = nj;
        P.S[P.levels] = psd_plan_shape(nj, L, D);
        ++P.levels;
    }
    P.nbins = 0;
    for (int j = 0; j < P.levels; ++j) {
        const int32_t lo = j == P.levels - 1 ? 0 : L / 8, hi = j == 0 ? L / 2 : L / 4 - 1;
        P.first_bin[j] = lo;
        P.bins[j] = hi - lo + 1;
        P.nbins += P.bins[j];
    }
    return P;
}

// y[s][i] = sum_t h[t] x[s][2 i + t], i = 0 .. n_out - 1, n_out = decimate2_outputs(n) >= 1 and at most kDecMaxTiles tiles: one
// workgroup per (tile, series); series s occupies x[s * series_stride .. + n) and y[s * y_stride .. + n_out)
hipError_t launch_decimate2(const double* x, int64_t n, int64_t series_stride, int32_t nseries, double* y, int64_t y_stride,
                            hipStream_t st);

// out[s * pitch + k] = dens[s * full + first + k], k = 0 .. bins - 1, s = 0 .. nseries - 1: the bins a level reports, from
// launch_psd_finish's densities to the level's columns of the output
hipError_t launch_lpsd_report(const double* dens, int32_t nseries, int32_t full, int32_t first, int32_t bins, double* out, int32_t pitch,
                              hipStream_t st);

}  // namespace ginsim
