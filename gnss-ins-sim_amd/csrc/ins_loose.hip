// Loosely coupled GPS/INS Kalman filter (InsLoose): sensor synthesis + free-integration mechanisation on bias-corrected
// samples + a 15-state closed-loop error-state filter, one lane per run.
//
// The reference declares the interface only (demo_algorithms/ins_loose.py: input fs, gyro, accel, time, gps_time, gps; output
// pos, vel, att_euler, wb, ab; prediction and correction are `pass`), so the arithmetic is specified here and restated in NumPy
// by tests/ins_loose_ref.py:
//   state order   dr(0-2) dv(3-5) psi(6-8) dbg(9-11) dba(12-14), error = estimate - truth, C_est = (I - [psi x]) C
//   propagation   P <- Phi P Phi^T + Qd, Phi = I + F dt; F: (r,v) = I, (v,psi) = [f^n x], (v,ba) = -C, (psi,bg) = C,
//                 (bg,bg) = -1/tau_g, (ba,ba) = -1/tau_a.  Phi is applied as the block congruences T_r, T_v, T_psi, D in that
//                 order (each reads rows the earlier ones left untouched: the product is exactly I + F dt), 3x3 blocks
//   correction    z = ins - gps, H = [I6 0], six sequential scalar updates, feedback, x = 0
// P is the upper triangle (120 doubles) per lane in LDS, [element][lane], 60 KB per single-wavefront workgroup (two per CU).
// Registers were tried first (one wavefront per SIMD: 256 VGPRs + 256 AGPRs per lane, but arithmetic takes its operands from the
// VGPRs only and a double needs an aligned pair).  The build's resource report with the 240 registers of P, per lane:
//   default flags                  100-700 bytes of scratch in every instantiation
//   machine-LICM off (build.py)    0 for the given-sensors ones without statistics, 12-430 for the others; scheduling fences
//                                  changed nothing; part of P in LDS (30, 60 elements, or 36 parked outside the covariance phases)
//                                  116-490
// With all of P in LDS: 0 bytes in all 12 instantiations (machine-LICM off; with it on the vibration variants keep a 36-byte
// private segment that no instruction addresses).  Every loop over P has compile-time bounds and is fully unrolled, so every LDS
// offset is an immediate.
//
// The sensor synthesis keeps mc_kernel.hip's -ffp-contract=on (same bits as ginsim_mc_run's sensors); a fix is gps_fix of
// gps_synth.hpp (same bits as ginsim_aux_sensors).  The generated and the given form share every line after the samples are in
// registers.
// What loose_aided_kernel (ins_loose_aided.hip) shares with this file -- Cov, the propagation, the correction, the time loop -- is
// in ins_loose.hpp; the host side that launches an instantiation of either, or of loose_cons_kernel (ins_loose_cons.hip), is
// launch_loose_family (loose_launch.hpp) on the file's trait; which family a launch takes is decided in api_mc.hip (launch_loose).
#include <hip/hip_runtime.h>
#include "ginsim.h"
#include "ins_loose.hpp"
#include "launch.hpp"
#include "loose_launch.hpp"

namespace ginsim {

// RF: ref_frame.  GIVEN: samples from in_accel / in_gyro, fixes from in_gps.  VIB: the generated sensors carry a vibration term.
// PS: online process-error statistics (out_proc).
template <int RF, bool GIVEN, bool VIB, bool PS>
__global__ void __launch_bounds__(kLooseBlock)
loose_kernel(const ginsim_mc_params a, const ginsim_loose_params b, const int64_t* __restrict__ stamp, const int32_t* __restrict__ visible) {
    static_assert(!VIB || !GIVEN, "vibration: generate mode");
    __shared__ uint32_t ntab[GIVEN ? 4 : kNormalLdsWords];
    loose_body<RF, GIVEN, VIB, PS, false>(a, b, stamp, visible, ntab);
}

int loose_variant(const ginsim_mc_params& p) { return p.given_sensors ? 1 : 0; }

struct PlainFamily {
    static constexpr const char* name = "loose_kernel";
    static constexpr size_t lds = kLooseCovLds;
    template <int RF, bool GIVEN, bool VIB, bool PS> static constexpr auto kernel = &loose_kernel<RF, GIVEN, VIB, PS>;
};

hipError_t launch_loose_plain(const LooseLaunch& L) { return launch_loose_family<PlainFamily>(L, L.b->out_proc != nullptr); }

}  // namespace ginsim
