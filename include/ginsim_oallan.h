/*
 * ginsim_oallan.h -- the overlapping Allan variance of libginsim.so, a header of its own next to ginsim.h (whose entry points and
 * GINSIM_ABI_VERSION it leaves as they are).  Plain C99; the same library exports these functions.
 *
 * For a series x[0..n) and an averaging factor m, with theta[k] = sum_{i<k} x[i]:
 *
 *     d_m[k]   = theta[k+2m] - 2 theta[k+m] + theta[k],      k = 0 .. n - 2m          (n - 2m + 1 terms)
 *     oavar(m) = sum_k d_m[k]^2 / (2 m^2 (n - 2m + 1)),      tau(m) = m * (1 / fs)
 *
 * the estimator of IEEE Std 952 that takes the window at every shift of one sample, where ginsim_allan takes the non-overlapping
 * bins of allan.allan_var (gnss_ins_sim/allan/allan.py:18-59).  The averaging factors are exactly ginsim_allan's (allan.py:29-43),
 * so the two curves share their tau.
 */
#ifndef GINSIM_OALLAN_H
#define GINSIM_OALLAN_H

#include "ginsim.h"

#ifdef __cplusplus
extern "C" {
#endif

/* x: device pointer, series s occupies x[s*series_stride .. +n).  Outputs (host): tau[cap] and oavar[nseries][cap] (the VARIANCE);
 * *ntau = number of averaging factors (0 when the series is shorter than 9 s).  A series with a non-finite sample has NaN at every
 * factor; every other series of the call keeps its bits, and a series' result does not depend on the other series of the call.
 * Refusals as ginsim_allan's: NULL argument; n, nseries, series_stride out of range or fs not positive and finite
 * (GINSIM_ERR_ARG); more series than the device's maxGridSize[1], cap below *ntau (GINSIM_ERR_RANGE, before any launch). */
int ginsim_oallan(ginsim_ctx* ctx, const double* x, int64_t n, int32_t nseries, int64_t series_stride, double fs,
                  double* tau, double* oavar, int32_t* ntau, int32_t cap);

/* What ginsim_oallan with these arguments runs, from the planning code the call itself launches from.  Host arithmetic only: no
 * context, no device, nothing launched, x never followed.  Per factor: m, terms = n - 2m + 1, the form (0 tile: 2m <= tile_halo,
 * evaluated from tile-local prefixes in LDS, tile_payload shifts per workgroup; 1 stream: from a prefix of x - x[0] kept in
 * scratch) and nparts, the partial records per series that the finishing launch folds in ascending order.  The environment
 * variable GINSIM_OALLAN_TILE=0, read per call, sends every factor through the stream form (a diagnostic).  scratch_bytes: what
 * the call takes from the context's scratch.  GINSIM_ERR_RANGE when cap is smaller than *ntau (which is still reported). */
typedef struct {
    int64_t m, terms;
    int32_t form, nparts;
} ginsim_oallan_factor;
typedef struct {
    int64_t tile_payload, tile_halo, scratch_bytes;
    int32_t tile_factors, stream_factors;
} ginsim_oallan_geometry;
int ginsim_oallan_plan(const double* x, int64_t n, int32_t nseries, int64_t series_stride, double fs, int32_t* ntau,
                       ginsim_oallan_factor* f /*[cap]*/, int32_t cap, ginsim_oallan_geometry* g);

#ifdef __cplusplus
}
#endif

#endif /* GINSIM_OALLAN_H */
