// InsLoose aided at standstill: loose_aided_kernel's lane (ins_loose.hpp, loose_body) with the zero-velocity update (ZUPT) and the
// zero-angular-rate update (ZARU).  DESIGN 4.11g; restated in NumPy by tests/ins_loose_ref.py.
//
// State order, x = estimate - truth and C_est = (I - [psi x]) C as in ins_loose.hip.  Every row observes one state, H = e_I, and is
// the scalar update of a GPS fix, Cov::update<I>(z, R, x):
//   ZUPT (bit 0 of still_mask), I = 3, 4, 5:    z_i = vel_i, R = r_zupt.  vel is the mechanised velocity in the coordinates of dv
//        (the three numbers loose_correct subtracts fix[3..5] from); the truth is zero, so z = dv.
//   ZARU (bit 1), I = 9, 10, 11:                z_i = bg_est_i + w_rest_i - gyro_i, R = r_zaru[i].  At rest the raw gyro sample is
//        w_rest + bg_true + noise, so z = dbg - noise.  gyro is the RAW sample j - 1, before the bias is subtracted: the last
//        sample the lane integrated, carried across the iteration (three doubles, in these instantiations only).  w_rest is the
//        rate the mechanisation itself assumes of a body at rest (nav_step with v = 0): C_est^T (W cos lat, 0, -W sin lat) from
//        the reported latitude and attitude in ref_frame 0 with earth_rot, zero otherwise.
//   Neglected: w_rest depends on psi (C_est^T = C^T (I + [psi x]): about W |psi| = 7e-5 psi rad/s).  H has no entry on psi for it, as F
//        has none for earth rate.  The ZARU sample's noise is the gyro noise the process noise q_psi already accounts for: a known,
//        small correlation.
// Every z is formed once, from the state before the first row.  A block starts from x = 0, runs the selected rows in ascending
// state order, then feeds x back exactly as a GPS fix does (loose_feedback) and zeroes it.
// It runs at every IMU sample j > 0 with j % still_every == 0 and still_flags[j] != 0 on the state that row j reports: after a GPS
// correction and after an odometer / non-holonomic block of the same sample (each has had its own feedback), before the row is
// stored.  The period is the block's own counter.  still_flags is int32[n] on the device, one standstill signal per IMU sample for
// all runs (the role gps_visible plays for fixes), read with a wave-uniform index: the branch around a block does not diverge.  A
// per-lane detector on the noisy sensors would diverge the wavefront and is not built.
// The odometer / non-holonomic block is compiled in (AID): aid_mask stays a wave-uniform run-time value and aid_mask == 0 never
// fires a block.  No consistency checkpoints, no magnetometer block, 15 states.  12 instantiations <RF, GIVEN, VIB, PS>.
// The block's numbers are the kernel's fifth argument, a ginsim_loose_still_params by value: the lane reads them from the kernarg
// segment where they are used (loose_still_params() of ins_loose.hpp), as it reads the two blocks before them.
//
// The launch is launch_loose_family (loose_launch.hpp) on the file's trait, with PS as the flag and the block as the tail argument.
// Built with ins_loose.hip's flags; P stays in LDS as [120][64], one wavefront per workgroup, nothing new in LDS.  The build's
// resource report (build/ins_loose_still.resources.txt, read by tests/test_ins_loose_still_oracle.py): 0 bytes of scratch in all 12.
#include <hip/hip_runtime.h>
#include "ginsim.h"
#include "ins_loose.hpp"
#include "launch.hpp"
#include "loose_launch.hpp"

namespace ginsim {

// g is read through loose_still_params(), not through the argument
template <int RF, bool GIVEN, bool VIB, bool PS>
__global__ void __launch_bounds__(kLooseBlock)
loose_still_kernel(const ginsim_mc_params a, const ginsim_loose_params b, const int64_t* __restrict__ stamp, const int32_t* __restrict__ visible,
                   const ginsim_loose_still_params g) {
    static_assert(!VIB || !GIVEN, "vibration: generate mode");
    __shared__ uint32_t ntab[GIVEN ? 4 : kNormalLdsWords];
    loose_body<RF, GIVEN, VIB, PS, true, false, false, kLooseStates, true>(a, b, stamp, visible, ntab);
}

struct StillFamily {
    static constexpr const char* name = "loose_still_kernel";
    static constexpr size_t lds = kLooseCovLds;
    template <int RF, bool GIVEN, bool VIB, bool PS> static constexpr auto kernel = &loose_still_kernel<RF, GIVEN, VIB, PS>;
};

// L.still->still_mask != 0 (api_mc.hip checks the block and takes still_mask == 0 for no standstill block)
hipError_t launch_loose_still(const LooseLaunch& L) { return launch_loose_family<StillFamily>(L, L.b->out_proc != nullptr, *L.still); }

}  // namespace ginsim
