// Consistency checkpoints for every InsLoose family: loose_all_kernel's lane (ins_loose_all.hip: the odometer / non-holonomic
// block, the magnetometer block, the standstill block and, in ins_loose_all_cons16.hip, the odometer's scale factor as a 16th state)
// with the flag CONS of ins_loose_cons.hip.  DESIGN 4.11i; restated in NumPy by tests/ins_loose_all_cons_ref.py.
//
// Nothing of the filter is new: every block is compiled in and gated at run time, so a launch with an absent block computes the
// single family's bits, and one kernel family serves every subset of the three blocks.  The checkpoint of sample j stands where
// loose_cons_kernel has it: after the fix, the odometer / constraint block, the magnetometer block and the standstill block of
// that sample, before the row is stored.  The record keeps its 43 doubles (ginsim.h, GINSIM_CONS_RECORD) and slots 0-36 their
// meaning.  With 16 states three of the six reserved slots carry the scale state:
//   [37] the sum of P[15][15], [38] of (k_est - k_true)^2, [39] of (k_est - k_true)^2 / P[15][15];  [40..42] = 0.
// k_true is scale_truth[r] of the run id r (not of the lane).  Without a truth (NULL) [38] and [39] are 0 and the scale error takes
// no part in a lane's inclusion; with 16 states a lane is included only with P[15][15] > 0 and finite, and with a truth only with
// both quotients finite.  With 15 states [37..42] = 0.
// The sums are loose_cons_kernel's: one xor butterfly per value in a fixed order, lane 0 stores the wavefront's partial record, and
// cons_final_kernel (ins_loose_cons.hip) adds the wavefronts in ascending order.  No atomics: the same bits from launch to launch.
// Tail lanes stay in the loop, repeat the last run of the list and weigh 0, as under CONS everywhere.
// The kernel's arguments after loose_all_kernel's five: the checkpoint arguments (ConsArgs) and the truth pointer.  PS is false:
// online process statistics and checkpoints in one launch are refused.
//
// This file: the 6 instantiations <RF, GIVEN, VIB, 15>; P in LDS as [120][64].  ins_loose_all_cons16.hip: <..., 16>, [136][64].
// Built with ins_loose.hip's flags; the build's resource report (build/ins_loose_all_cons.resources.txt,
// build/ins_loose_all_cons16.resources.txt; read by tests/test_ins_loose_all_cons_oracle.py): 0 bytes of scratch in all 12.
#include "ins_loose_all_cons.hpp"

namespace ginsim {

// L.cons is set; any of L.mag, L.scale and L.still (api_mc.hip checks each block as its own family does); with L.scale the
// launch is ins_loose_all_cons16.hip's
hipError_t launch_loose_all_cons(const LooseLaunch& L) {
    return L.scale ? launch_loose_all_cons16(L) : launch_loose_all_cons_ns<kLooseStates>(L);
}

}  // namespace ginsim
