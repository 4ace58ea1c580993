// What ins_loose_all.hip (15 states) and ins_loose_all16.hip (16 states) share: loose_all_kernel, the lane of ins_loose.hpp's loose_body
// with every block compiled in, its trait for launch_loose_family (loose_launch.hpp) and the one by-value block a launch hands it.
// DESIGN 4.11h.  The 24 instantiations <RF, GIVEN, VIB, PS, NS> are split by NS over the two files, twelve each: one file with all of
// them compiles twice as long as any other file of the library.
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
// the argument
template <int RF, bool GIVEN, bool VIB, bool PS, int NS>
__global__ void __launch_bounds__(kLooseBlock)
loose_all_kernel(const ginsim_mc_params a, const ginsim_loose_params b, const int64_t* __restrict__ stamp, const int32_t* __restrict__ visible,
                 const ginsim_loose_all_params g) {
    static_assert(!VIB || !GIVEN, "vibration: generate mode");
    static_assert(NS == kLooseStates || NS == kLooseScaleStates, "15 or 16 states");
    __shared__ uint32_t ntab[GIVEN ? 4 : kNormalLdsWords];
    loose_body<RF, GIVEN, VIB, PS, true, false, true, NS, true, Tail::ALL>(a, b, stamp, visible, ntab);
}

template <int NS>
struct AllFamily {
    static constexpr const char* name = "loose_all_kernel";
    static constexpr size_t lds = loose_cov_lds(NS);
    template <int RF, bool GIVEN, bool VIB, bool PS> static constexpr auto kernel = &loose_all_kernel<RF, GIVEN, VIB, PS, NS>;
};

// The launch, or the name, of the instantiation with NS states: the blocks L has one after the other, an absent one all zero
// (mag_every = 0 and still_mask = 0 never fire; the scale block is read with 16 states only).  The printed name gains the kernel's
// fifth template argument.
template <int NS>
hipError_t launch_loose_all_ns(const LooseLaunch& L) {
    ginsim_loose_all_params g;
    memset(&g, 0, sizeof(g));
    if (L.mag) g.mag = *L.mag;
    if (L.scale) g.scale = *L.scale;
    if (L.still) g.still = *L.still;
    const hipError_t e = launch_loose_family<AllFamily<NS>>(L, L.b->out_proc != nullptr, g);
    if (L.name) {
        const size_t len = strlen(L.name);
        if (len > 0 && L.name[len - 1] == '>') snprintf(L.name + len - 1, L.cap - (len - 1), ", %d>", NS);
    }
    return e;
}

}  // namespace ginsim
