/*
 * ginsim_csd.h -- Welch's cross-spectral density between pairs of series of libginsim.so, a header of its own next to ginsim.h,
 * ginsim_oallan.h, ginsim_psd.h and ginsim_lpsd.h (whose entry points and GINSIM_ABI_VERSION it leaves as they are).  Plain C99; the
 * same library exports these functions.
 *
 * For series x[0..n) and y[0..n), a segment length L = nperseg (a power of two, 8 <= L <= 4096), a step D (1 <= D <= L), a window w
 * and a sampling rate fs:
 *
 *     K       = (n - L) / D + 1                          segments; samples past (K-1) D + L are not read
 *     X_s     = DFT_L((segx_s - mean(segx_s)) w)         detrend = 1;  DFT_L(segx_s w) with detrend = 0;  Y_s likewise from y
 *     Pxx[k]  = c_k / (K fs U) sum_s |X_s[k]|^2          k = 0 .. L/2,  U = sum_k w[k]^2;  Pyy likewise
 *     Pxy[k]  = c_k / (K fs U) sum_s conj(X_s[k]) Y_s[k] complex
 *     c_k     = 2 for 0 < k < L/2,  1 for k = 0 and k = L/2;    f[k] = k fs / L
 *
 * The windows are ginsim_psd.h's: GINSIM_PSD_BOXCAR (0) and GINSIM_PSD_HANN (1, periodic).  This is scipy.signal.csd(x, y, fs,
 * window, nperseg=L, noverlap=L-D, detrend='constant' or False, scaling='density'), and Pxx is scipy.signal.welch of x.  The
 * magnitude-squared coherence is |Pxy|^2 / (Pxx Pyy), the H1 transfer estimate of y over x is Pxy / Pxx.
 *
 * nperseg = 8192, which ginsim_psd_welch takes, is refused here: a workgroup keeps four sums per bin in registers where the PSD
 * kernel keeps one, and at 8192 that kernel already holds 254 of a lane's 256 vector registers.
 */
#ifndef GINSIM_CSD_H
#define GINSIM_CSD_H

#include "ginsim.h"

#ifdef __cplusplus
extern "C" {
#endif

/* x: device pointer, series s occupies x[s*series_stride .. +n), as for ginsim_psd_welch.  pairs: host array int32[npairs][2] of
 * series indices (x-series, y-series); i == j is allowed and a series may stand in any number of pairs.  Outputs (host): freq[cap]
 * and pxx, pyy, pxy_re, pxy_im, each [npairs][cap]; *nfreq = nperseg/2 + 1.
 * No atomics are used: every launch gives the same bits.  A pair's bits depend on its two series and on (n, nperseg, step, window,
 * detrend, fs) alone: not on npairs, on its place in the table or on its neighbours.  A pair that reads a non-finite sample in
 * either series (or whose segment sum overflows) has NaN at every bin of all four outputs, and no other pair has one; a non-finite
 * value in the unread tail changes nothing.  pxy_im is exactly +0.0 at bins 0 and nperseg/2 (there X and Y are the real and the
 * imaginary part of one transform) unless the pair is NaN.
 * Refusals, before any launch and in this order: a NULL argument; n, nseries, series_stride < n or fs not positive and finite;
 * npairs < 1; nperseg not a power of two in [8, 4096]; step outside [1, nperseg]; window or detrend outside their values; a pair
 * index outside [0, nseries) (GINSIM_ERR_ARG); n < nperseg; a pair of more than 2^31 - 1 parts (ginsim_csd_plan's nparts), or
 * records of npairs * nparts * 4 * (nperseg/2 + 1) doubles that pass 2^63 bytes; more pairs than the device's maxGridSize[1]; cap
 * below *nfreq, which is still reported (GINSIM_ERR_RANGE). */
int ginsim_csd_welch(ginsim_ctx* ctx, const double* x, int64_t n, int32_t nseries, int64_t series_stride, double fs,
                     const int32_t* pairs, int32_t npairs, int32_t nperseg, int32_t step, int32_t window, int32_t detrend,
                     double* freq, double* pxx, double* pyy, double* pxy_re, double* pxy_im, int32_t* nfreq, int32_t cap);

/* What ginsim_csd_welch with these arguments runs, from the planning code the call itself launches from.  Host arithmetic only: no
 * context, no device, nothing launched.  A workgroup of `threads` owns one pair and one part, segs_per_part consecutive segments
 * (ginsim_psd_plan's function of nperseg and step alone, so a pair's partition depends on (n, nperseg, step) alone; the last part
 * has the rest), and leaves one partial record of 4 (nperseg/2 + 1) sums; a finishing launch adds a pair's nparts records in
 * ascending order.  lds_bytes: the workgroup's LDS; scratch_bytes: what the call takes from the context's scratch, the records and
 * the pair table.  The same refusals as the call's, as far as its arguments go, with the prefix csd_plan:.  A refused plan leaves
 * *g as it was. */
typedef struct {
    int64_t segments, scratch_bytes;
    int32_t segs_per_part, nparts, lds_bytes, threads;
} ginsim_csd_geometry;
int ginsim_csd_plan(int64_t n, int32_t nseries, int64_t series_stride, double fs, int32_t npairs, int32_t nperseg, int32_t step,
                    ginsim_csd_geometry* g);

#ifdef __cplusplus
}
#endif

#endif /* GINSIM_CSD_H */
