// InsLoose with all its aids in one launch: loose_aided_kernel's lane (ins_loose.hpp, loose_body) with the magnetometer block
// (ins_loose_mag.hip), the standstill block (ins_loose_still.hip) and, in ins_loose_all16.hip, the odometer's scale factor as a 16th
// state (ins_loose_scale.hip).  DESIGN 4.11h; restated in NumPy by tests/ins_loose_all_ref.py, which composes tests/ins_loose_ref.py
// and tests/ins_loose_scale_ref.py without a change to either.
//
// Nothing new is specified.  At IMU sample j the order is the GPS fix, the odometer / non-holonomic block, the magnetometer block,
// the standstill block, then the row is stored.  Each block keeps its own period counter and its own gate, starts from x = 0, forms
// every z and h from the state before its first row and ends in the feedback (loose_feedback).  With 16 states every block's feedback
// also does k_est -= x[15]; the magnetometer rows (Cov::update_row_psi) and the standstill rows (Cov::update<I>) have h[15] = 0 and
// move k_est through the cross-covariance, as a GPS fix does.
// The three blocks are compiled in (AID, MAG, STILL) and gated at run time by wave-uniform values, as aid_mask gates the aiding block:
// mag_every == 0 (or >= n) fires no magnetometer block, still_mask == 0 no standstill block, and none of an absent block's pointers
// is read.  NS is a template argument: a launch without the scale block is the 15-state instantiation.
// The kernel's fifth argument is one ginsim_loose_all_params by value, the three family blocks one after the other; the lane reads
// each from the kernarg segment where it is used, at its member's offset (ins_loose.hpp, Tail::ALL), as the single families read
// theirs at the argument's start.  No consistency checkpoints here: ins_loose_all_cons.hip has this lane with them.  Every store is
// an ordinary per-lane store.
//
// This file: the 12 instantiations <RF, GIVEN, VIB, PS, 15>; P stays in LDS as [120][64].  ins_loose_all16.hip: <..., 16>, [136][64].
// Built with ins_loose.hip's flags; the build's resource report (build/ins_loose_all.resources.txt, build/ins_loose_all16.resources.txt;
// read by tests/test_ins_loose_all_oracle.py): 0 bytes of scratch in all 24.
#include "ins_loose_all.hpp"

namespace ginsim {

// two or three of L.mag, L.scale and L.still are set (api_mc.hip checks each block as its own family does); with L.scale the
// launch is ins_loose_all16.hip's
hipError_t launch_loose_all(const LooseLaunch& L) { return L.scale ? launch_loose_all16(L) : launch_loose_all_ns<kLooseStates>(L); }

}  // namespace ginsim
