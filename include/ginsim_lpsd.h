/*
 * ginsim_lpsd.h -- the multi-resolution power spectral density of libginsim.so: Welch's estimate (ginsim_psd.h) on a decimating
 * octave cascade.  A header of its own next to ginsim.h, ginsim_oallan.h and ginsim_psd.h (whose entry points and
 * GINSIM_ABI_VERSION it leaves as they are).  Plain C99; the same library exports these functions.
 *
 * The filter h[0..27) is a symmetric half-band low-pass of 27 taps (M = 13), a Kaiser-windowed sinc with unit DC gain; its taps at
 * even offsets m != 0 from the centre are exactly 0, which leaves 15.  csrc/halfband_table.inc is its specification.  One
 * decimation of x[0..n):
 *
 *     y[i]  = h[M] x[2i+M] + sum_{m = 1, 3, .. 13} h[M+m] (x[2i+M-m] + x[2i+M+m]),   i = 0 .. n_out - 1
 *     n_out = (n - 27) / 2 + 1 for n >= 27: only valid outputs, no padding
 *
 * The pair is added first and the terms are added in ascending m onto the centre term, each as one fused multiply-add.  Zero taps
 * are not evaluated: a non-finite sample reaches exactly the outputs one of whose 15 taps touches it.
 *
 * The cascade of a series x at rate fs, with ginsim_psd_welch's nperseg L, step D, window and detrend:
 *
 *     x_0 = x, fs_0 = fs;   x_{j+1} = decimate(x_j), fs_{j+1} = fs_j / 2
 *     level j exists while n_j >= L, K_j = (n_j - L) / D + 1 >= min_segments and j < GINSIM_LPSD_MAX_LEVELS; J is the last
 *     P_j   = what ginsim_psd_welch gives for x_j, n_j, fs_j, L, D, window, detrend: bit for bit and with its NaN rule
 *     level j reports the bins k = lo_j .. hi_j of P_j at f = k fs_j / L:   lo_j = 0 if j = J, else L/8;
 *                                                                             hi_j = L/2 if j = 0, else L/4 - 1
 *
 * in ascending frequency, level J first and level 0 last: the octaves tile [0, fs/2] without gap or overlap, and with J = 0 the
 * result is ginsim_psd_welch's.  A level keeps only frequencies below a quarter of its own rate, onto which only the band
 * [3/8, 1/2] of the rate before it folds (below -98 dB); the filter's droop over a level's reported band, under 3e-5 of the
 * density per level, is not compensated.
 */
#ifndef GINSIM_LPSD_H
#define GINSIM_LPSD_H

#include "ginsim.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GINSIM_LPSD_MAX_LEVELS 32
#define GINSIM_LPSD_TAPS 27

/* One decimation, device to device: series s occupies x[s*series_stride .. +n) and y[s*y_stride .. +*n_out); the caller owns y.
 * An output's bits depend on its 27 inputs alone, no atomics are used, and a series' outputs do not depend on nseries or on its
 * neighbours.  *n_out is reported whenever the sizes are legal.  Refusals, before any launch: a NULL argument; nseries < 1,
 * n < 27, series_stride < n (GINSIM_ERR_ARG); y_stride < *n_out; x and y ranges that overlap; more tiles of 1024 outputs than
 * 2^31 - 1; more series than the device's maxGridSize[1] (GINSIM_ERR_RANGE). */
int ginsim_decimate2(ginsim_ctx* ctx, const double* x, int64_t n, int32_t nseries, int64_t series_stride,
                     double* y, int64_t y_stride, int64_t* n_out);

/* x: device pointer as for ginsim_psd_welch.  Outputs (host): freq[cap], psd[nseries][cap] and level[cap], the level a bin came
 * from; *nbins of each are written.  Every level's NaN rule is ginsim_psd_welch's on that level's series: a non-finite sample
 * that level 0 does not read but level 1 does leaves level 0's bins finite.
 * Refusals, before any launch and in this order: those of ginsim_psd_welch for (n, nseries, series_stride, fs, nperseg, step,
 * window, detrend) up to and including the device's maxGridSize[1], under the prefix lpsd:; min_segments < 1 (GINSIM_ERR_ARG);
 * fewer than min_segments segments at level 0, a level 1 of more than 2^31 - 1 tiles, or level buffers that pass 2^63 bytes;
 * cap below *nbins, which is still reported (GINSIM_ERR_RANGE). */
int ginsim_lpsd(ginsim_ctx* ctx, const double* x, int64_t n, int32_t nseries, int64_t series_stride, double fs,
                int32_t nperseg, int32_t step, int32_t window, int32_t detrend, int32_t min_segments,
                double* freq, double* psd, int32_t* level, int32_t* nbins, int32_t cap);

/* What ginsim_lpsd with these arguments runs, from the planning code the call itself launches from.  Host arithmetic only.
 * levels = J + 1; per level j: its length n, its segments, the first bin it reports, how many, and the parts of its Welch call
 * (ginsim_psd_plan's nparts).  scratch_bytes: what the call takes from the context's scratch -- two level buffers of
 * nseries * n_1 and nseries * n_2 doubles (levels 1, 3, .. in the first, 2, 4, .. in the second), the Welch records of level 0
 * (every other level's fit in them) and one level's finished densities, nseries * (nperseg/2 + 1) doubles, each padded to 256
 * bytes.  The same refusals as the call's, as far as its arguments go, with the prefix lpsd_plan:.  A refused plan leaves *g as it
 * was. */
typedef struct {
    int64_t n, segments;
    int32_t first_bin, bins, nparts, reserved;
} ginsim_lpsd_level;
typedef struct {
    int64_t scratch_bytes;
    int32_t levels, nbins;
    ginsim_lpsd_level level[GINSIM_LPSD_MAX_LEVELS];
} ginsim_lpsd_geometry;
int ginsim_lpsd_plan(int64_t n, int32_t nseries, int64_t series_stride, double fs, int32_t nperseg, int32_t step,
                     int32_t min_segments, ginsim_lpsd_geometry* g);

#ifdef __cplusplus
}
#endif

#endif /* GINSIM_LPSD_H */
