/*
 * ginsim_psd.h -- Welch's power spectral density of libginsim.so, a header of its own next to ginsim.h and ginsim_oallan.h (whose
 * entry points and GINSIM_ABI_VERSION it leaves as they are).  Plain C99; the same library exports these functions.
 *
 * For a series x[0..n), a segment length L = nperseg (a power of two, 8 <= L <= 8192), a step D (1 <= D <= L), a window w and a
 * sampling rate fs:
 *
 *     K      = (n - L) / D + 1                          segments; samples past (K-1) D + L are not read
 *     seg_s  = x[sD .. sD + L)                           s = 0 .. K-1
 *     y_s[k] = (seg_s[k] - mean(seg_s)) w[k]             detrend = 1;   seg_s[k] w[k] with detrend = 0
 *     X_s    = DFT_L(y_s)
 *     P[k]   = c_k (1/K) sum_s |X_s[k]|^2 / (fs U),      k = 0 .. L/2,   U = sum_k w[k]^2
 *     c_k    = 2 for 0 < k < L/2,  1 for k = 0 and k = L/2          (single-sided density, unit^2 / Hz)
 *     f[k]   = k fs / L
 *
 * window 0: boxcar (U = L); window 1: periodic Hann, w[k] = 0.5 - 0.5 cos(2 pi k / L) (U = 3 L / 8).  This is
 * scipy.signal.welch(x, fs, window, nperseg=L, noverlap=L-D, detrend='constant' or False, scaling='density'), and the single-sided
 * convention of the PSD that ginsim_vib_psd_series takes.
 */
#ifndef GINSIM_PSD_H
#define GINSIM_PSD_H

#include "ginsim.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GINSIM_PSD_BOXCAR 0
#define GINSIM_PSD_HANN 1

/* x: device pointer, series s occupies x[s*series_stride .. +n).  Outputs (host): freq[cap] and psd[nseries][cap];
 * *nfreq = nperseg/2 + 1.  A series with a non-finite value among the samples it reads (or whose segment sum overflows) has NaN at
 * every bin; a non-finite value in the unread tail changes nothing; every other series of the call keeps its bits, a series' bits
 * do not depend on nseries or on its neighbours, and no atomics are used: every launch gives the same bits.
 * Refusals, before any launch and in this order: a NULL argument; n, nseries, series_stride < n or fs not positive and finite;
 * nperseg not a power of two in [8, 8192]; step outside [1, nperseg]; window or detrend outside their values (GINSIM_ERR_ARG);
 * n < nperseg; a series of more than 2^31 - 1 parts (ginsim_psd_plan's nparts), or records of nseries * nparts * (nperseg/2 + 1)
 * doubles that pass 2^63 bytes -- the message names the number of parts; more series than the device's maxGridSize[1]; cap below
 * *nfreq, which is still reported (GINSIM_ERR_RANGE). */
int ginsim_psd_welch(ginsim_ctx* ctx, const double* x, int64_t n, int32_t nseries, int64_t series_stride, double fs,
                     int32_t nperseg, int32_t step, int32_t window, int32_t detrend,
                     double* freq, double* psd, int32_t* nfreq, int32_t cap);

/* What ginsim_psd_welch with these arguments runs, from the planning code the call itself launches from.  Host arithmetic only: no
 * context, no device, nothing launched.  A workgroup of `threads` owns one series and one part, segs_per_part consecutive segments
 * (a function of nperseg and step alone; the last part has the rest), and leaves one partial record of nperseg/2 + 1 sums; a
 * finishing launch adds a series' nparts records in ascending order.  lds_bytes: the workgroup's LDS; scratch_bytes: what the call
 * takes from the context's scratch.  The same refusals as the call's, as far as its arguments go, with the prefix psd_plan:; any n
 * is a legal question, and one whose nparts or scratch_bytes this structure cannot state is refused (GINSIM_ERR_RANGE), never
 * answered with a narrowed number.  A refused plan leaves *g as it was. */
typedef struct {
    int64_t segments, scratch_bytes;
    int32_t segs_per_part, nparts, lds_bytes, threads;
} ginsim_psd_geometry;
int ginsim_psd_plan(int64_t n, int32_t nseries, int64_t series_stride, double fs, int32_t nperseg, int32_t step,
                    ginsim_psd_geometry* g);

#ifdef __cplusplus
}
#endif

#endif /* GINSIM_PSD_H */
