// Planning code and launch interface of the Welch cross-spectral-density kernels (csd.hip) for the C ABI glue (api_series.hip).
// A pair of series is partitioned exactly as psd.hpp partitions one series -- psd_plan_shape(n, L, D), the same segs_per_part, a
// function of (L, D) alone -- and a workgroup has psd.hip's size and LDS arrays; what differs is the record, four planes per part,
// and the pair table that goes to the device behind the records.
#pragma once
#include "psd.hpp"

namespace ginsim {

// 8 <= nperseg <= 4096: at 8192 the PSD kernel already holds 254 VGPRs and this one keeps twice its accumulators
constexpr int kCsdMinLog2 = kPsdMinLog2, kCsdMaxLog2 = 12;
constexpr int kCsdPlanes = 4;                               // sum |X|^2, sum |Y|^2, Re and Im of sum conj(X) Y

constexpr int csd_threads(int L) { return psd_threads(L); }
constexpr int csd_lds_bytes(int L) { return psd_lds_bytes(L); }

// the scratch of a call on a shape whose nparts is at most kPsdMaxParts: records [npairs][nparts][4][nbins] doubles padded to 256,
// then the pair table int32[npairs][2] padded to 256.  false, and nothing set, when the bytes pass INT64_MAX (npairs nparts < 2^62
// is exact; the bytes are compared by division, never formed past 64 bits)
inline bool csd_scratch_bytes(PsdShape& s, int32_t npairs, size_t& table_bytes) {
    const int64_t records = (int64_t)npairs * s.nparts;
    const size_t tb = (sizeof(int32_t) * 2 * (size_t)npairs + 255) & ~(size_t)255;
    const int64_t per = (int64_t)(sizeof(double) * (size_t)kCsdPlanes * (size_t)s.nbins);
    if (records > (INT64_MAX - 255 - (int64_t)tb) / per) return false;
    s.record_bytes = ((size_t)per * (size_t)records + 255) & ~(size_t)255;
    table_bytes = tb;
    return true;
}

// one workgroup per (part, pair): records[pair][part][4][0 .. L/2] = the part's sums of |X_s[k]|^2, |Y_s[k]|^2, Re and Im of
// conj(X_s[k]) Y_s[k] for the series x + pairs[2 pair] stride and x + pairs[2 pair + 1] stride; NaN at every bin of the four planes
// when a sample the part reads in either series is not finite.  pairs is a device pointer.
hipError_t launch_csd_parts(const double* x, int64_t series_stride, const int32_t* pairs, int32_t npairs, int32_t D, int32_t window,
                            int32_t detrend, const PsdShape& s, double* records, hipStream_t st);
// out[plane][pair][k] = c_k * scale * (the parts' records added in ascending order), c_k = 2 for 0 < k < L/2 and 1 at both ends
hipError_t launch_csd_finish(const double* records, int32_t npairs, const PsdShape& s, double scale, double* out, hipStream_t st);

}  // namespace ginsim
