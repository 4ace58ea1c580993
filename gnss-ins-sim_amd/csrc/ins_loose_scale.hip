// InsLoose with the odometer's scale factor as a 16th state: loose_aided_kernel's lane (ins_loose.hpp, loose_body) with NS = 16.
// DESIGN 4.11e; restated in NumPy by tests/ins_loose_scale_ref.py.
//
// State order, x = estimate - truth and C_est = (I - [psi x]) C as in ins_loose.hip; state 15 is dk = k_est - k, k the true scale
// of odo_j = k v_b[0] + stdv z.  k_est is a double of the lane: scale0 at sample 0, P[15][15] = p0_scale^2, row / column 15
// otherwise zero.
//   propagation    dk is a constant with an optional random walk: Phi is the identity on state 15 and couples it to nothing, so the
//                  congruences T_r, T_v, T_psi and the scaling D of loose_propagate run over 16 columns (row 15's cross terms move
//                  because the other rows move) and P[15][15] += q_k
//   odometer row   with D = C_est^T and v_b = D v of the state before the first row:  z0 = v_b[0] - odo_j / k_est.  With
//                  odo_j = k v_b,true[0] + n and 1 / k_est = (1 - dk / k_est) / k to first order,
//                  z0 = h.x - n / k_est,  h = the six entries of loose_aided_kernel's row on states 3-8 and h[15] = v_b[0] / k_est
//                  R0 = r_odo, a fixed parameter (its dependence on dk is second order)
//   other rows     the two constraint rows have h[15] = 0 (Cov::update_row's six-entry form over 16 states); a GPS fix is
//                  Cov::update<I> over 16 states: it moves k_est through the cross-covariance
//   feedback       k_est -= x[15] next to loose_feedback, at every block that ran a row
// The order inside a sample is loose_aided_kernel's: fix, aiding block, row stored.  No magnetometer block, no checkpoints.
// 12 instantiations <RF, GIVEN, VIB, PS> as loose_kernel's.  The scale block's numbers and outputs are the kernel's fifth argument, a
// ginsim_loose_scale_params by value, read from the kernarg segment where they are used (loose_scale_params() of ins_loose.hpp).
// k_est and everything else of a lane is written with ordinary per-lane (vector) stores.
//
// The launch is launch_loose_family (loose_launch.hpp) on the file's trait with 68 KB of dynamic LDS: P is [136][64] doubles, one wavefront per
// workgroup; with the 8 KB of normal tables of the generating forms two workgroups fit a CU's 160 KB.
// Built with ins_loose.hip's flags; the build's resource report is build/ins_loose_scale.resources.txt (read by
// tests/test_ins_loose_scale_oracle.py).
#include <hip/hip_runtime.h>
#include "ginsim.h"
#include "ins_loose.hpp"
#include "launch.hpp"
#include "loose_launch.hpp"

namespace ginsim {

// g is read through loose_scale_params(), not through the argument
template <int RF, bool GIVEN, bool VIB, bool PS>
__global__ void __launch_bounds__(kLooseBlock)
loose_scale_kernel(const ginsim_mc_params a, const ginsim_loose_params b, const int64_t* __restrict__ stamp, const int32_t* __restrict__ visible,
                   const ginsim_loose_scale_params g) {
    static_assert(!VIB || !GIVEN, "vibration: generate mode");
    __shared__ uint32_t ntab[GIVEN ? 4 : kNormalLdsWords];
    loose_body<RF, GIVEN, VIB, PS, true, false, false, kLooseScaleStates>(a, b, stamp, visible, ntab);
}

struct ScaleFamily {
    static constexpr const char* name = "loose_scale_kernel";
    static constexpr size_t lds = loose_cov_lds(kLooseScaleStates);
    template <int RF, bool GIVEN, bool VIB, bool PS> static constexpr auto kernel = &loose_scale_kernel<RF, GIVEN, VIB, PS>;
};

// L.b->aid_mask has bit 0 (api_mc.hip checks it)
hipError_t launch_loose_scale(const LooseLaunch& L) { return launch_loose_family<ScaleFamily>(L, L.b->out_proc != nullptr, *L.scale); }

}  // namespace ginsim
