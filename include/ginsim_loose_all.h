/*
 * ginsim_loose_all.h -- the loosely coupled GPS/INS filter of libginsim.so with all its aids in one launch, a header of its own next
 * to ginsim.h (whose entry points and GINSIM_ABI_VERSION it leaves as they are).  Plain C99; the same library exports these functions.
 *
 * ginsim.h has one entry point per optional block of the filter: the magnetometer (ginsim_loose_mag_run), the odometer's scale
 * factor as a 16th state (ginsim_loose_scale_run), the standstill updates (ginsim_loose_still_run).  Each launches a kernel that
 * has that block and none of the others.  The entry point below takes any of the three blocks and launches one kernel that has
 * them all (csrc/ins_loose_all.hip).  Nothing new is specified: at IMU sample j the order is the GPS fix, the
 * odometer / non-holonomic block, the magnetometer block, the standstill block, then the row is stored; each block keeps its own
 * period counter, starts from x = 0, forms every z and h from the state before its first row and ends in the feedback.  With the
 * scale-factor state every block's feedback also does k_est -= x[15]; the magnetometer rows and the standstill rows have
 * h[15] = 0.
 */
#ifndef GINSIM_LOOSE_ALL_H
#define GINSIM_LOOSE_ALL_H

#include "ginsim.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The kernel's fifth argument, by value: the three blocks one after the other.  An absent block is all zero (mag_every = 0,
 * still_mask = 0; the scale block is not read by the kernel with 15 states): it never fires and none of its pointers is read. */
typedef struct {
    ginsim_loose_mag_params   mag;
    ginsim_loose_scale_params scale;
    ginsim_loose_still_params still;
} ginsim_loose_all_params;

/* ginsim_loose_run with any of the three blocks; each of mag, scale and still may be NULL.  The checks, in this order, the first
 * failure returned: everything ginsim_loose_run refuses (fp32 among it); then each block that is not NULL as its own entry point
 * checks it, with that entry point's message: mag as ginsim_loose_mag_run, scale as ginsim_loose_scale_run (an aid_mask without
 * bit 0 among it), still as ginsim_loose_still_run.  A degenerate block (mag_every == 0, still_mask == 0) is then no block.
 * With two or three blocks left the launch is loose_all_kernel, with 16 states where scale is among them and 15 otherwise.  With
 * one block left it is that block's own entry point, with none ginsim_loose_run: the same kernel, the same bits. */
int ginsim_loose_all_run(ginsim_ctx* ctx, const ginsim_mc_params* mc, const ginsim_loose_params* p, const ginsim_loose_mag_params* mag,
                         const ginsim_loose_scale_params* scale, const ginsim_loose_still_params* still);
/* the NAME of the kernel it launches (e.g. "ginsim::loose_all_kernel<1, false, false, false, 16>" = RF, GIVEN, VIB, PS, NS) */
int ginsim_loose_all_kernel_name(const ginsim_mc_params* mc, const ginsim_loose_params* p, const ginsim_loose_mag_params* mag,
                                 const ginsim_loose_scale_params* scale, const ginsim_loose_still_params* still, char* buf, size_t cap);

#ifdef __cplusplus
}
#endif

#endif /* GINSIM_LOOSE_ALL_H */
