// InsLoose with all its aids in one launch, the 16-state half: the 12 instantiations <RF, GIVEN, VIB, PS, 16> of loose_all_kernel
// (ins_loose_all.hpp; the account is in ins_loose_all.hip's header).  68 KB of dynamic LDS, P as [136][64] doubles, one wavefront per
// workgroup; with the 8 KB of normal tables of the generating forms two workgroups fit a CU's 160 KB, as loose_scale_kernel.
// Built with ins_loose.hip's flags; the build's resource report is build/ins_loose_all16.resources.txt.
#include "ins_loose_all.hpp"

namespace ginsim {

// L.scale is set and L.b->aid_mask has bit 0 (api_mc.hip checks it)
hipError_t launch_loose_all16(const LooseLaunch& L) { return launch_loose_all_ns<kLooseScaleStates>(L); }

}  // namespace ginsim
