// InsLoose aided by the odometer and the non-holonomic constraints of a land vehicle: loose_kernel's lane (ins_loose.hpp,
// loose_body) with an aiding block.  DESIGN 4.11b; restated in NumPy by tests/ins_loose_aided_ref.py.
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
// Built with ins_loose.hip's flags; P stays in LDS as [120][64], one wavefront per workgroup.  The build's resource report
// (build/ins_loose_aided.resources.txt, read by tests/test_ins_loose_aided_oracle.py): 0 bytes of scratch in all 12.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include "ginsim.h"
#include "device_once.hpp"
#include "ins_loose.hpp"
#include "launch.hpp"

namespace ginsim {

template <int RF, bool GIVEN, bool VIB, bool PS>
__global__ void __launch_bounds__(kLooseBlock)
loose_aided_kernel(const ginsim_mc_params a, const ginsim_loose_params b, const int64_t* __restrict__ stamp, const int32_t* __restrict__ visible) {
    static_assert(!VIB || !GIVEN, "vibration: generate mode");
    __shared__ uint32_t ntab[GIVEN ? 4 : kNormalLdsWords];
    loose_body<RF, GIVEN, VIB, PS, true>(a, b, stamp, visible, ntab);
}

template <int RF, bool PS>
static hipError_t launch_aided_a(const ginsim_mc_params& p, const ginsim_loose_params& b, const int64_t* stamp, const int32_t* visible,
                                 hipStream_t stream, char* name, size_t cap) {
    const int tb = kLooseBlock;
    const dim3 grid((unsigned)((b.n_list + tb - 1) / tb)), block((unsigned)tb);
    const bool given = p.given_sensors != 0, vib = any_vibration(p);
    if (name) {
        snprintf(name, cap, "ginsim::loose_aided_kernel<%d, %s, %s, %s>", RF, given ? "true" : "false", vib ? "true" : "false", PS ? "true" : "false");
        return hipSuccess;
    }
    constexpr size_t kLooseLds = kLooseCovLds;
    static PerDeviceOnce once;          // more than 64 KB of dynamic LDS: the attribute, on every device that launches
    once.run([] {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&loose_aided_kernel<RF, true, false, PS>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLooseLds);
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&loose_aided_kernel<RF, false, true, PS>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLooseLds);
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&loose_aided_kernel<RF, false, false, PS>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLooseLds);
    });
    if (given) hipLaunchKernelGGL((loose_aided_kernel<RF, true, false, PS>), grid, block, kLooseLds, stream, p, b, stamp, visible);
    else if (vib) hipLaunchKernelGGL((loose_aided_kernel<RF, false, true, PS>), grid, block, kLooseLds, stream, p, b, stamp, visible);
    else hipLaunchKernelGGL((loose_aided_kernel<RF, false, false, PS>), grid, block, kLooseLds, stream, p, b, stamp, visible);
    return hipGetLastError();
}

// name != NULL: report the kernel's name, do not launch.  stamp / visible: DEVICE copies of b.gps_stamp / b.gps_visible
hipError_t launch_loose_aided(const ginsim_mc_params& p, const ginsim_loose_params& b, const int64_t* stamp, const int32_t* visible,
                              hipStream_t stream, char* name, size_t cap) {
    const bool ps = b.out_proc != nullptr;
    if (p.ref_frame == 1) return ps ? launch_aided_a<1, true>(p, b, stamp, visible, stream, name, cap) : launch_aided_a<1, false>(p, b, stamp, visible, stream, name, cap);
    return ps ? launch_aided_a<0, true>(p, b, stamp, visible, stream, name, cap) : launch_aided_a<0, false>(p, b, stamp, visible, stream, name, cap);
}

}  // namespace ginsim
