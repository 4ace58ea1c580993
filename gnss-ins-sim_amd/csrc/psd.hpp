// Planning code and launch interface of the Welch power-spectral-density kernels (psd.hip) for the C ABI glue (api_series.hip).
// Everything a call's shape depends on is host arithmetic in this header: ginsim_psd_welch launches from psd_plan_shape and
// ginsim_psd_plan reports it, and psd.hip sizes its workgroups and LDS arrays from the same constexpr functions.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ginsim {

constexpr int kPsdMinLog2 = 3, kPsdMaxLog2 = 13;            // 8 <= nperseg <= 8192

// threads of the workgroup that transforms segments of L samples: a butterfly of the radix-2 stage is one thread's work, L / 2 of
// them per stage; between one and eight wavefronts
constexpr int psd_threads(int L) { return L / 4 < 64 ? 64 : (L / 4 > 512 ? 512 : L / 4); }

// the quarter-wave cosine table C[q] = cos(2 pi q / L), q = 0 .. L/4, with one pad entry per 32 and one more per 1024 (psd.hip)
constexpr int psd_table_slot(int q) { return q + (q >> 5) + (q >> 10); }
constexpr int psd_table_doubles(int L) { return (psd_table_slot(L / 4) + 2) & ~1; }     // an even count: 16-byte arrays

// LDS of one workgroup: the complex array as two planes of L doubles, the table, two wavefront totals per wavefront (a single
// wavefront needs none)
constexpr int psd_lds_bytes(int L) { return 8 * (2 * L + psd_table_doubles(L) + (psd_threads(L) > 64 ? 2 * (psd_threads(L) / 64) : 0)); }

// What one call runs.  A part is segs_per_part consecutive segments of one series (an even count: a workgroup transforms its
// segments two at a time as one complex transform) and a function of (L, D) alone, so that the partition of a series never depends
// on the other series of the call.  It is large enough that a workgroup reads at least 16384 new samples between two partial
// records (the cosine table and the record are paid once per part) and that the records take at most an eighth of the samples'
// bytes: nparts (L/2 + 1) <= K L / (2 segs_per_part) + .. <= n / 8 with segs_per_part >= 4 L / D.
struct PsdShape {
    int64_t segments;           // K = (n - L) / D + 1
    int64_t nparts;             // ceil(K / segs_per_part): 64 bits until the glue has held it to kPsdMaxParts
    int32_t segs_per_part;
    int32_t nbins;              // L/2 + 1
    int32_t log2L;
    size_t record_bytes;        // [nseries][nparts][nbins] doubles, padded to 256; 0 until psd_record_bytes has set it
};

// the parts of a series are a launch's grid x dimension and an int32_t of ginsim_psd_geometry
constexpr int64_t kPsdMaxParts = 0x7FFFFFFF;

inline int64_t psd_segs_per_part(int64_t L, int64_t D) {
    int64_t pairs = 8192 / D;
    if (pairs < 2 * L / D) pairs = 2 * L / D;
    if (pairs < 1) pairs = 1;
    return 2 * pairs;
}

// on checked arguments: L a power of two in range, 1 <= D <= L <= n.  Nothing is narrowed here: any such n has an answer in 64 bits
// (K <= n, and K - 1 + segs_per_part is never formed), and the caller refuses what a launch or the geometry cannot state
inline PsdShape psd_plan_shape(int64_t n, int32_t L, int32_t D) {
    PsdShape s;
    s.segments = (n - L) / D + 1;
    s.segs_per_part = (int32_t)psd_segs_per_part(L, D);
    s.nparts = (s.segments - 1) / s.segs_per_part + 1;
    s.nbins = L / 2 + 1;
    s.log2L = 0;
    while ((1 << s.log2L) < L) ++s.log2L;
    s.record_bytes = 0;
    return s;
}

// the records of a shape whose nparts is at most kPsdMaxParts: false, and nothing set, when their padded bytes pass INT64_MAX
// (nseries nparts < 2^62 is exact; the bytes are compared by division, never formed past 64 bits)
inline bool psd_record_bytes(PsdShape& s, int32_t nseries) {
    const int64_t records = (int64_t)nseries * s.nparts;
    if (records > (INT64_MAX - 255) / (int64_t)(sizeof(double) * (size_t)s.nbins)) return false;
    s.record_bytes = (sizeof(double) * (size_t)records * (size_t)s.nbins + 255) & ~(size_t)255;
    return true;
}

// one workgroup per (part, series): records[series][part][0 .. L/2] = sum over the part's segments of |X_s[k]|^2, NaN at every
// bin when a sample the part reads is not finite
hipError_t launch_psd_parts(const double* x, int64_t series_stride, int32_t nseries, int32_t D, int32_t window, int32_t detrend,
                            const PsdShape& s, double* records, hipStream_t st);
// out[series][k] = c_k * scale * (the parts' records added in ascending order), c_k = 2 for 0 < k < L/2 and 1 at both ends
hipError_t launch_psd_finish(const double* records, int32_t nseries, const PsdShape& s, double scale, double* out, hipStream_t st);

}  // namespace ginsim
