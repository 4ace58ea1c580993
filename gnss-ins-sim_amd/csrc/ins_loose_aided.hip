// InsLoose aided by the odometer and the non-holonomic constraints of a land vehicle: loose_kernel's lane (ins_loose.hpp,
// loose_body) with an aiding block.  DESIGN 4.11b; restated in NumPy by tests/ins_loose_ref.py.
//
// State order, x = estimate - truth and C_est = (I - [psi x]) C as in ins_loose.hip.  With D = C_est^T (navigation -> body) of the
// reported attitude, v the reported navigation-frame velocity and v_b = D v, to first order v_b,est = v_b + D dv - D [v x] psi:
//   row 0 (aid_mask bit 0)      the odometer   z0 = v_b[0] - odo_j / odo_scale_f,  R0 = r_odo
//   rows 1, 2 (bits 1, 2)       the vehicle neither slides sideways nor leaves the road   z_i = v_b[i] - 0,  R_i = r_nhc
//   h_i = [0 0 0, D[i,:], -(D [v x])[i,:], 0 0 0, 0 0 0]: non-zero on states 3-8 only
// D, v, v_b and every h_i are formed once, from the state before the first row.  A block starts from x = 0 and runs the selected
// rows in ascending order, each  Ph = P h (15 values, 6 products each), s = h.Ph + R, g = (z - h.x) / s, x += Ph g,
// P -= Ph Ph^T / s  (Cov::update_row), then feeds x back exactly as a GPS fix does (loose_feedback) and zeroes it.
// It runs at every IMU sample j > 0 with j % aid_every == 0 on the state that row j reports, after a GPS correction of the same
// sample (which has had its own feedback) and before the row is stored.  odo_j is regenerated in the lane from stream S_ODO at
// counter j (the bits ginsim_mc_run writes to out_odo) or read from in_odo[j runs + r] (given_sensors).
// aid_mask and aid_every are wave-uniform kernel arguments, not template parameters: 12 instantiations as loose_kernel's.
//
// The launch is launch_loose_family (loose_launch.hpp) on the file's trait, with PS as the flag.
// Built with ins_loose.hip's flags; P stays in LDS as [120][64], one wavefront per workgroup.  The build's resource report
// (build/ins_loose_aided.resources.txt, read by tests/test_ins_loose_aided_oracle.py): 0 bytes of scratch in all 12.
#include <hip/hip_runtime.h>
#include "ginsim.h"
#include "ins_loose.hpp"
#include "launch.hpp"
#include "loose_launch.hpp"

namespace ginsim {

template <int RF, bool GIVEN, bool VIB, bool PS>
__global__ void __launch_bounds__(kLooseBlock)
loose_aided_kernel(const ginsim_mc_params a, const ginsim_loose_params b, const int64_t* __restrict__ stamp, const int32_t* __restrict__ visible) {
    static_assert(!VIB || !GIVEN, "vibration: generate mode");
    __shared__ uint32_t ntab[GIVEN ? 4 : kNormalLdsWords];
    loose_body<RF, GIVEN, VIB, PS, true>(a, b, stamp, visible, ntab);
}

struct AidedFamily {
    static constexpr const char* name = "loose_aided_kernel";
    static constexpr size_t lds = kLooseCovLds;
    template <int RF, bool GIVEN, bool VIB, bool PS> static constexpr auto kernel = &loose_aided_kernel<RF, GIVEN, VIB, PS>;
};

hipError_t launch_loose_aided(const LooseLaunch& L) { return launch_loose_family<AidedFamily>(L, L.b->out_proc != nullptr); }

}  // namespace ginsim
