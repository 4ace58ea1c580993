// Magnetometer synthesis shared by the kernels that make a run's magnetometer samples (aux_mag_kernel of aux_sensors.hip, which
// writes them, and magcal.hip, which consumes them in registers): pathgen.mag_gen (pathgen.py:658-661),
//     mag = si . (ref_mag + hi) + std * N,    N = the three normals of (seed, run) at counter j, stream S_MAG_XY.
// Moved here verbatim from aux_mag_kernel: the ISA of that kernel is unchanged.  Both files are compiled with
// -ffp-contract=on, and mag_axis is ONE source expression, so the front end fuses the same multiply-adds in both: the same bits.
#pragma once
#include <hip/hip_runtime.h>
#include "philox.hpp"

namespace ginsim {

// the three normals of magnetometer sample j of the run behind `key`: x, y from the pair of S_MAG_XY, z from the first of S_MAG_Z
__device__ __forceinline__ void mag_normals(const RngKey& key, uint32_t j, const NormalTables& tab, double (&z)[3]) {
    double z0[2], z1[2];
    normal_pairs<S_MAG_XY, 2>(key, j, z0, z1, tab);
    z[0] = z0[0];
    z[1] = z1[0];
    z[2] = z0[1];
}

// one axis of the sample: row `si` of the soft-iron matrix times v = ref_mag + hi, plus the noise      (ref + hi) . si^T + std * N
template <typename Row>
__device__ __forceinline__ double mag_axis(Row si, const double (&v)[3], double sd, double z) {
    return si[0] * v[0] + si[1] * v[1] + si[2] * v[2] + sd * z;
}

}  // namespace ginsim
