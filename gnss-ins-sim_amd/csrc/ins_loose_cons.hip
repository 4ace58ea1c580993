// Consistency checkpoints of InsLoose: loose_kernel's / loose_aided_kernel's lane (ins_loose.hpp, loose_body) with the flag CONS,
// and the kernel that adds the wavefronts' partial records.  DESIGN 4.11c; restated in NumPy by tests/ins_loose_cons_ref.py.
//
// A Monte-Carlo user asks whether the filter's covariance is honest ALONG the run: its predicted 1 sigma against the across-run
// error before, during and after a GPS outage.  The covariance exists only inside the launch (P in LDS, 60 KB per wavefront),
// and keeping its diagonal per sample and run would be [15][n][runs] more without the 3x3 blocks a normalised error needs.  So the
// across-run sums are taken here.  At a checkpoint (a sample of the strictly increasing list cons_sample, walked with a counter as
// the fixes are) every lane forms e = estimate - truth in the filter's own coordinates against row j of ref_nav and the values of
// the record (ginsim.h, ginsim_loose_cons_params):
//   P_kk (15), e_k^2 and e_k^2 / P_kk of the 9 navigation states, and e_b^T P_bb^-1 e_b of the three 3x3 blocks by the explicit
//   adjugate and determinant of the symmetric block.
// A lane with a non-finite value, a P_kk <= 0 or a block that is not positive definite enters no sum.  LDS is full (P and the
// normal tables), so the lanes of the wavefront are summed with cross-lane operations: one 6-level xor butterfly per value, whose
// order is fixed, and lane 0 stores the 37 sums to cons_work[wave][checkpoint][43].  cons_final_kernel adds the wavefronts in
// ascending order.  No atomics: the record is the same bits from launch to launch.
// A value is made from e (18 registers) and the lane's column of P in LDS when its turn comes, so the record itself never
// occupies registers.  Lanes past n_list stay in the loop (the butterfly needs defined partners): they filter the last run of the
// list again and weigh 0.
// The errors of the six bias states are left out (they carry P_kk only): the given form has no bias truth.
// PS is false here: online process statistics and checkpoints in one launch are refused.  12 instantiations, <RF, GIVEN, VIB, AID>.
// The filter's launch is launch_loose_family (loose_launch.hpp) on the file's trait, with AID as the flag and the checkpoint
// arguments behind the filter's own; launch_loose_cons launches cons_final_kernel after it.
// Built with ins_loose.hip's flags; the build's resource report is build/ins_loose_cons.resources.txt
// (tests/test_ins_loose_cons_oracle.py reads it).
#include <hip/hip_runtime.h>
#include "ginsim.h"
#include "ins_loose.hpp"
#include "launch.hpp"
#include "loose_launch.hpp"

namespace ginsim {

template <int RF, bool GIVEN, bool VIB, bool AID>
__global__ void __launch_bounds__(kLooseBlock)
loose_cons_kernel(const ginsim_mc_params a, const ginsim_loose_params b, const int64_t* __restrict__ stamp, const int32_t* __restrict__ visible,
                  const ConsArgs cq) {
    static_assert(!VIB || !GIVEN, "vibration: generate mode");
    __shared__ uint32_t ntab[GIVEN ? 4 : kNormalLdsWords];
    loose_body<RF, GIVEN, VIB, false, AID, true>(a, b, stamp, visible, ntab, cq);
}

// out[c][k] = the sum over the wavefronts, ascending, of work[wave][c][k]; one thread per element of the record
__global__ void __launch_bounds__(256) cons_final_kernel(const double* __restrict__ work, int64_t waves, int64_t len, double* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= len) return;
    double acc = 0.0;
    for (int64_t w = 0; w < waves; ++w) acc += work[w * len + i];
    out[i] = acc;
}

struct ConsFamily {
    static constexpr const char* name = "loose_cons_kernel";
    static constexpr size_t lds = kLooseCovLds;
    template <int RF, bool GIVEN, bool VIB, bool AID> static constexpr auto kernel = &loose_cons_kernel<RF, GIVEN, VIB, AID>;
};

// L.cons->cons_m > 0 (api_mc.hip checks it and takes cons_m == 0 for no checkpoint block)
hipError_t launch_loose_cons(const LooseLaunch& L) {
    const ginsim_loose_cons_params& c = *L.cons;
    const hipError_t e = launch_loose_family<ConsFamily>(L, L.b->aid_mask != 0, ConsArgs{L.samples, c.cons_m, c.cons_work});
    if (L.name || e != hipSuccess) return e;
    return launch_cons_final(c, (L.b->n_list + kLooseBlock - 1) / kLooseBlock, L.stream);
}

hipError_t launch_cons_final(const ginsim_loose_cons_params& c, int64_t waves, hipStream_t stream) {
    const int64_t len = c.cons_m * GINSIM_CONS_RECORD;
    hipLaunchKernelGGL(cons_final_kernel, dim3((unsigned)((len + 255) / 256)), dim3(256), 0, stream, c.cons_work, waves, len, c.out_cons);
    return hipGetLastError();
}

}  // namespace ginsim
