// InsLoose aided by the magnetometer: loose_aided_kernel's lane (ins_loose.hpp, loose_body) with a three-row heading block.
// DESIGN 4.11d; restated in NumPy by tests/ins_loose_ref.py.
//
// State order, x = estimate - truth and C_est = (I - [psi x]) C as in ins_loose.hip.  With D = C_est^T (navigation -> body) of the
// reported attitude, m_n the field the filter assumes in the navigation frame and the calibrated sample
// m_cal = cal_si . mag_j - cal_hi, to first order D_est m_n = m_b - D [m_n x] psi.  For body axis i = 0, 1, 2:
//   z_i = D[i,:] . m_n - m_cal[i],   R_i = r_mag[i]
//   h_i = [0 0 0, 0 0 0, m_n x D[i,:], 0 0 0, 0 0 0]: the psi part of an odometer row with v replaced by m_n, non-zero on states 6-8
// D, z and every h_i are formed once, from the state before the first row.  A block starts from x = 0 and runs the three rows in
// ascending order, each  Ph = P h (15 values, 3 products each), s = h.Ph + R, g = (z - h.x) / s, x += Ph g, P -= Ph Ph^T / s
// (Cov::update_row_psi), then feeds x back exactly as a GPS fix does (loose_feedback) and zeroes it.
// It runs at every IMU sample j > 0 with j % mag_every == 0 on the state that row j reports: after a GPS correction and after an
// odometer / non-holonomic block of the same sample (each has had its own feedback), before the row is stored.  The period is
// the block's own counter.  mag_j is regenerated in the lane by mag_normals / mag_axis of mag_synth.hpp on ref_mag[j] + mag_hi
// (the bits ginsim_aux_sensors writes to out_mag; this file is compiled with aux_sensors.hip's -ffp-contract=on) or read from
// in_mag[(c n + j) runs + r] (given_sensors).
// The odometer / non-holonomic block is compiled in (AID): aid_mask stays a wave-uniform run-time value and aid_mask == 0 never
// fires a block.  No consistency checkpoints (CONS = false).  12 instantiations <RF, GIVEN, VIB, PS> as loose_kernel's.
// The magnetometer block's numbers are the kernel's fifth argument, a ginsim_loose_mag_params by value: the lane reads them from
// the kernarg segment where they are used (loose_mag_params() of ins_loose.hpp), as it reads the two blocks before them.
//
// The launch is launch_loose_family (loose_launch.hpp) on the file's trait, with PS as the flag and the block as the tail argument.
// Built with ins_loose.hip's flags; P stays in LDS as [120][64], one wavefront per workgroup, nothing new in LDS.  The build's
// resource report (build/ins_loose_mag.resources.txt, read by tests/test_ins_loose_mag_oracle.py): 0 bytes of scratch in all 12.
#include <hip/hip_runtime.h>
#include "ginsim.h"
#include "ins_loose.hpp"
#include "launch.hpp"
#include "loose_launch.hpp"

namespace ginsim {

// g is read through loose_mag_params(), not through the argument
template <int RF, bool GIVEN, bool VIB, bool PS>
__global__ void __launch_bounds__(kLooseBlock)
loose_mag_kernel(const ginsim_mc_params a, const ginsim_loose_params b, const int64_t* __restrict__ stamp, const int32_t* __restrict__ visible,
                 const ginsim_loose_mag_params g) {
    static_assert(!VIB || !GIVEN, "vibration: generate mode");
    __shared__ uint32_t ntab[GIVEN ? 4 : kNormalLdsWords];
    loose_body<RF, GIVEN, VIB, PS, true, false, true>(a, b, stamp, visible, ntab);
}

struct MagFamily {
    static constexpr const char* name = "loose_mag_kernel";
    static constexpr size_t lds = kLooseCovLds;
    template <int RF, bool GIVEN, bool VIB, bool PS> static constexpr auto kernel = &loose_mag_kernel<RF, GIVEN, VIB, PS>;
};

// L.mag->mag_every > 0 (api_mc.hip checks it and takes mag_every == 0 for no magnetometer block)
hipError_t launch_loose_mag(const LooseLaunch& L) { return launch_loose_family<MagFamily>(L, L.b->out_proc != nullptr, *L.mag); }

}  // namespace ginsim
