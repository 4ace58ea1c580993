// What ins_loose_all_cons.hip (15 states) and ins_loose_all_cons16.hip (16 states) share: loose_all_cons_kernel, loose_all_kernel's
// lane (ins_loose_all.hpp) with the consistency checkpoints of ins_loose_cons.hip, its trait for launch_loose_family
// (loose_launch.hpp) and the launch.  DESIGN 4.11i.  The 12 instantiations <RF, GIVEN, VIB, NS> are split by NS over the two
// files, six each, as ins_loose_all*.hip are.
#pragma once
#include <hip/hip_runtime.h>
#include <string.h>
#include "ginsim.h"
#include "ginsim_loose_all.h"
#include "ins_loose.hpp"
#include "launch.hpp"
#include "loose_launch.hpp"

namespace ginsim {

// g is read through loose_mag_params<Tail::ALL>(), loose_scale_params<Tail::ALL>() and loose_still_params<Tail::ALL>(), not through
// the argument.  ktrue: the scale factor's truth [runs], indexed by the run id, or NULL; read with 16 states only
template <int RF, bool GIVEN, bool VIB, int NS>
__global__ void __launch_bounds__(kLooseBlock)
loose_all_cons_kernel(const ginsim_mc_params a, const ginsim_loose_params b, const int64_t* __restrict__ stamp, const int32_t* __restrict__ visible,
                      const ginsim_loose_all_params g, const ConsArgs cq, const double* __restrict__ ktrue) {
    static_assert(!VIB || !GIVEN, "vibration: generate mode");
    static_assert(NS == kLooseStates || NS == kLooseScaleStates, "15 or 16 states");
    __shared__ uint32_t ntab[GIVEN ? 4 : kNormalLdsWords];
    loose_body<RF, GIVEN, VIB, false, true, true, true, NS, true, Tail::ALL>(a, b, stamp, visible, ntab, cq, ktrue);
}
static_assert(kLooseTailOffset + sizeof(ginsim_loose_all_params) + sizeof(ConsArgs) + sizeof(void*) <= 4096,
              "the kernarg segment of loose_all_cons_kernel: HIP's limit of 4 KB");

// launch_loose_family chooses <RF, flag> for a kernel with a bool as its fourth template argument: here both flags are the one
// instantiation with NS states, and the printed name's fourth argument is replaced by NS
template <int NS>
struct AllConsFamily {
    static constexpr const char* name = "loose_all_cons_kernel";
    static constexpr size_t lds = loose_cov_lds(NS);
    template <int RF, bool GIVEN, bool VIB, bool> static constexpr auto kernel = &loose_all_cons_kernel<RF, GIVEN, VIB, NS>;
};

// The launch, or the name, of the instantiation with NS states, then cons_final_kernel: the blocks L has one after the other, an
// absent one all zero, as launch_loose_all_ns; L.cons->cons_m > 0 (api_mc.hip checks it)
template <int NS>
hipError_t launch_loose_all_cons_ns(const LooseLaunch& L) {
    ginsim_loose_all_params g;
    memset(&g, 0, sizeof(g));
    if (L.mag) g.mag = *L.mag;
    if (L.scale) g.scale = *L.scale;
    if (L.still) g.still = *L.still;
    const ginsim_loose_cons_params& c = *L.cons;
    const hipError_t e = launch_loose_family<AllConsFamily<NS>>(L, false, g, ConsArgs{L.samples, c.cons_m, c.cons_work}, L.scale_truth);
    if (L.name) {
        char* const last = strrchr(L.name, ',');
        if (last) snprintf(last, L.cap - (size_t)(last - L.name), ", %d>", NS);
        return e;
    }
    if (e != hipSuccess) return e;
    return launch_cons_final(c, (L.b->n_list + kLooseBlock - 1) / kLooseBlock, L.stream);
}

}  // namespace ginsim
