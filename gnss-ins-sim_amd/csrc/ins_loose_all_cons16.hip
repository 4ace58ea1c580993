// Consistency checkpoints for every InsLoose family, the 16-state half: the 6 instantiations <RF, GIVEN, VIB, 16> of
// loose_all_cons_kernel (ins_loose_all_cons.hpp; the account is in ins_loose_all_cons.hip's header).  68 KB of dynamic LDS, P as
// [136][64] doubles, one wavefront per workgroup; with the 8 KB of normal tables of the generating forms two workgroups fit a CU's
// 160 KB, as loose_all_kernel.
// Built with ins_loose.hip's flags; the build's resource report is build/ins_loose_all_cons16.resources.txt.
#include "ins_loose_all_cons.hpp"

namespace ginsim {

// L.cons and L.scale are set and L.b->aid_mask has bit 0 (api_mc.hip checks it)
hipError_t launch_loose_all_cons16(const LooseLaunch& L) { return launch_loose_all_cons_ns<kLooseScaleStates>(L); }

}  // namespace ginsim
