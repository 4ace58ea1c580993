// The host-side launch of the loose family (ins_loose.hip, ins_loose_aided.hip, ins_loose_cons.hip, ins_loose_mag.hip,
// ins_loose_scale.hip, ins_loose_still.hip, ins_loose_all*.hip, ins_loose_all_cons*.hip): each file defines its own __global__ wrapper of loose_body, describes it by a trait and hands a LooseLaunch
// (launch.hpp) to launch_loose_family, which chooses <RF, flag> and gives the three instantiations to launch_loose_trio.
#pragma once
#include <hip/hip_runtime.h>
#include <stdio.h>
#include "ginsim.h"
#include "device_once.hpp"
#include "ins_loose.hpp"
#include "launch.hpp"

namespace ginsim {

// GIVEN / VIB / PLAIN: the instantiations <RF, true, false, F>, <RF, false, true, F> and <RF, false, false, F> of one kernel template
// (samples from in_accel / in_gyro; generated with a vibration term; generated without).  kernel, rf, flag: the template's name and
// the values of RF and F, for the printed name.  tail: the kernel's arguments after (p, b, stamp, visible).
// LDS: the bytes of dynamic LDS the family's covariance takes (loose_cov_lds of its number of states), for the attribute and the launch.
// name != NULL: report the kernel's name, do not launch.
template <size_t LDS, auto GIVEN, auto VIB, auto PLAIN, class... Tail>
hipError_t launch_loose_trio(const char* kernel, int rf, bool flag, const ginsim_mc_params& p, const ginsim_loose_params& b,
                             const int64_t* stamp, const int32_t* visible, hipStream_t stream, char* name, size_t cap, Tail... tail) {
    const dim3 grid((unsigned)((b.n_list + kLooseBlock - 1) / kLooseBlock)), block((unsigned)kLooseBlock);
    const bool given = p.given_sensors != 0, vib = any_vibration(p);
    if (name) {
        snprintf(name, cap, "ginsim::%s<%d, %s, %s, %s>", kernel, rf, given ? "true" : "false", vib ? "true" : "false", flag ? "true" : "false");
        return hipSuccess;
    }
    static PerDeviceOnce once;          // one per trio.  More than 64 KB of dynamic LDS: the attribute, on every device that launches
    once.run([] {
        for (auto k : {GIVEN, VIB, PLAIN})
            (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS);
    });
    hipLaunchKernelGGL(given ? GIVEN : (vib ? VIB : PLAIN), grid, block, LDS, stream, p, b, stamp, visible, tail...);
    return hipGetLastError();
}

// The choice of <RF, FLAG> for a family.  Family: a struct with
//   static constexpr const char* name      the kernel template's name, as printed
//   static constexpr size_t lds            the bytes of dynamic LDS of its covariance
//   kernel<RF, GIVEN, VIB, FLAG>           a static constexpr variable template: the address of that instantiation
// flag: the value of the kernel's fourth template argument for this launch.  tail: the kernel's arguments after the four common ones.
template <class Family, int RF, bool FLAG, class... Tail>
hipError_t launch_loose_as(const LooseLaunch& L, Tail... tail) {
    return launch_loose_trio<Family::lds, Family::template kernel<RF, true, false, FLAG>, Family::template kernel<RF, false, true, FLAG>,
                             Family::template kernel<RF, false, false, FLAG>>(Family::name, RF, FLAG, *L.mc, *L.b, L.stamp, L.visible, L.stream,
                                                                              L.name, L.cap, tail...);
}

template <class Family, class... Tail>
hipError_t launch_loose_family(const LooseLaunch& L, bool flag, Tail... tail) {
    if (L.mc->ref_frame == 1) return flag ? launch_loose_as<Family, 1, true>(L, tail...) : launch_loose_as<Family, 1, false>(L, tail...);
    return flag ? launch_loose_as<Family, 0, true>(L, tail...) : launch_loose_as<Family, 0, false>(L, tail...);
}

}  // namespace ginsim
