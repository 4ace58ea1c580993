// GPS synthesis shared by aux_gps_kernel (aux_sensors.hip) and loose_kernel (ins_loose.hip): fix k of one run, pathgen.gps_gen
// (pathgen.py:621-624).  One expression in one place, so that the filter's lane regenerates bit for bit the fix that
// ginsim_aux_sensors stores for the same seed, run and sigma (both files are compiled with -ffp-contract=on).
#pragma once
#include <hip/hip_runtime.h>
#include "philox.hpp"

namespace ginsim {

// ref: the truth row [6] = pos3, vel3 of fix k; sigma [6]; out [6]
template <class Ref, class Sigma>
__device__ __forceinline__ void gps_fix(Ref ref, Sigma sigma, const RngKey& key, uint32_t k, const NormalTables& tab, double (&out)[6]) {
    double z0[3], z1[3];
    normal_pairs<S_GPS_P_XY, 3>(key, k, z0, z1, tab);
    const double z[6] = {z0[0], z1[0], z0[1], z1[1], z0[2], z1[2]};     // pos x,y,z  vel x,y,z
#pragma unroll
    for (int c = 0; c < 6; ++c) out[c] = ref[c] + sigma[c] * z[c];
}

}  // namespace ginsim
