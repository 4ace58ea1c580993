/*
 * ginsim_loose_all_cons.h -- consistency checkpoints for the loosely coupled GPS/INS filter of libginsim.so with any of its aids, a
 * header of its own next to ginsim.h and ginsim_loose_all.h (whose entry points and GINSIM_ABI_VERSION it leaves as they are).
 * Plain C99; the same library exports these functions.
 *
 * ginsim_loose_cons_run (ginsim.h) takes checkpoints of the plain filter and of the odometer / non-holonomic one.  The entry point
 * below takes them of the filter with any of the magnetometer block, the scale-factor state and the standstill block, in one kernel
 * that has them all (csrc/ins_loose_all_cons.hip).  The checkpoint of sample j stands after the fix, the odometer /
 * non-holonomic block, the magnetometer block and the standstill block of that sample, before the row is stored.
 *
 * The record is ginsim_loose_cons_params' (GINSIM_CONS_RECORD = 43 doubles per checkpoint), slots 0-36 as there.  With the
 * scale-factor state, sums over the included runs:
 *   [37] P[15][15]   [38] (k_est - k_true)^2   [39] (k_est - k_true)^2 / P[15][15]   [40..42] 0
 * Without it [37..42] are 0.  A run is included as there and, with the scale-factor state, only if P[15][15] > 0 and finite and,
 * with a truth, both quotients are finite.
 */
#ifndef GINSIM_LOOSE_ALL_CONS_H
#define GINSIM_LOOSE_ALL_CONS_H

#include "ginsim.h"
#include "ginsim_loose_all.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ginsim_loose_all_run with checkpoints; each of mag, scale and still may be NULL.  scale_truth: DEVICE [runs], the true scale
 * factor of every run, indexed by the run id (not by the position in run_list), or NULL: [38] and [39] are then 0 and the scale
 * error takes no part in a run's inclusion.  The checks, in this order, the first failure returned: everything
 * ginsim_loose_all_run refuses for the same blocks, with its messages; then everything ginsim_loose_cons_run refuses of cons, with
 * its messages (out_proc among it); then a scale_truth without a scale block.  A degenerate block (mag_every == 0,
 * still_mask == 0) is then no block.  cons_m == 0 is ginsim_loose_all_run.  Otherwise, with any number of blocks left (0 - 3), the
 * launch is loose_all_cons_kernel, with 16 states where scale is among them and 15 otherwise, then cons_final_kernel. */
int ginsim_loose_all_cons_run(ginsim_ctx* ctx, const ginsim_mc_params* mc, const ginsim_loose_params* p, const ginsim_loose_mag_params* mag,
                              const ginsim_loose_scale_params* scale, const ginsim_loose_still_params* still,
                              const ginsim_loose_cons_params* cons, const double* scale_truth);
/* the NAME of the kernel it launches (e.g. "ginsim::loose_all_cons_kernel<1, false, false, 16>" = RF, GIVEN, VIB, NS) */
int ginsim_loose_all_cons_kernel_name(const ginsim_mc_params* mc, const ginsim_loose_params* p, const ginsim_loose_mag_params* mag,
                                      const ginsim_loose_scale_params* scale, const ginsim_loose_still_params* still,
                                      const ginsim_loose_cons_params* cons, const double* scale_truth, char* buf, size_t cap);

#ifdef __cplusplus
}
#endif

#endif /* GINSIM_LOOSE_ALL_CONS_H */
