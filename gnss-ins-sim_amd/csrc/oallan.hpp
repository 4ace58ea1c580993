// Launch interface of the overlapping Allan-variance kernels (oallan.hip) for the C ABI glue (api_series.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ginsim {

constexpr int kOallanMaxFactors = 64;       // the reference's list has 9 factors per decade: 64 covers n < 9e7 with room
constexpr int kOallanTileFactors = 32;      // factors one tile launch takes: its per-factor wavefront sums live in LDS

// One entry per averaging factor of the call, in the order of the factor list.  A series owns `records` doubles of the record
// array; factor i owns nparts[i] of them from offset[i], one per tile (tile form) or per work item (stream form).
struct OallanFactors {
    int32_t count;
    int32_t records;                        // sum of nparts
    int32_t m[kOallanMaxFactors];
    int32_t nparts[kOallanMaxFactors];
    int32_t offset[kOallanMaxFactors];
};

int oallan_tile_payload();                  // C: the shifts k one tile evaluates
int oallan_tile_halo();                     // H: the tile form takes the factors with 2 m <= H
int oallan_scan_chunk();                    // samples per workgroup of the blocked scan (stream form)
int oallan_stream_item();                   // shifts k per work item of the stream form

// tile form: factors first .. first + count - 1 of F for every series; grid (tiles, nseries)
hipError_t launch_oallan_tile(const double* x, int64_t n, int64_t series_stride, int32_t nseries, const OallanFactors& F, int first,
                              int count, double* records, hipStream_t st);
// theta[s][0..n] = prefix of x - x[0] (theta_stride entries per series) in three launches: chunk sums, their scan, apply
hipError_t launch_oallan_theta(const double* x, int64_t n, int64_t series_stride, int32_t nseries, double* chunk_sums, double* theta,
                               int64_t theta_stride, hipStream_t st);
// stream form: factors first .. first + count - 1 of F from theta; grid (work items of the smallest factor, count, nseries)
hipError_t launch_oallan_stream(const double* theta, int64_t n, int64_t theta_stride, int32_t nseries, const OallanFactors& F, int first,
                                int count, double* records, hipStream_t st);
// ONE launch folds the records of every factor, tiles ascending, and writes out[0..count) = tau, out[count + s * count + i] = oavar
hipError_t launch_oallan_finish(const double* records, int64_t n, int32_t nseries, double ts, const OallanFactors& F, double* out,
                                hipStream_t st);

}  // namespace ginsim
