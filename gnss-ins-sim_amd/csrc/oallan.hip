// Overlapping Allan variance: for an averaging factor m and theta[k] = sum_{i<k} x[i],
//
//     d_m[k] = theta[k+2m] - 2 theta[k+m] + theta[k],  k = 0 .. n-2m,      oavar(m) = sum_k d_m[k]^2 / (2 m^2 (n-2m+1))
//
// d is unchanged when theta gains a + b k, so every prefix here is one of SHIFTED samples: the tile form shifts by the tile's
// first sample and keeps a tile-local theta in LDS, the stream form keeps theta of x - x[0] in scratch.
//
// Tile form (2m <= H): a workgroup stages C + H samples of one series, scans them in place (every thread its own run of kSeg
// entries, the runs' totals by wave64 shuffles, the wavefronts' totals through LDS) and evaluates every tile-form factor from
// that one staging: lane l takes k = l, l + T, ..., its three taps are stride-1 across the lanes.  kSeg is odd so that the
// threads' runs start on different banks.  One record per (series, factor, tile).
// Stream form (the other factors): theta by a blocked scan in three launches (chunk sums, scan of the chunk sums, apply: no
// workgroup waits for another), then three taps m apart per shift, one record per (series, factor, work item).
// Finish: one launch folds the records of every factor, tiles ascending, divides, and writes tau and oavar to pinned memory.
// No atomics anywhere: every sum has one fixed order, and a series' records depend on that series alone.
#include "oallan.hpp"

namespace ginsim {

namespace {

constexpr int kThreads = 512;                   // tile / scan workgroup: 8 wavefronts
constexpr int kWaves = kThreads / 64;
constexpr int kSeg = 19;                        // entries per thread in the in-place scan (odd: conflict-free runs)
constexpr int kStage = kThreads * kSeg;         // C + H = 9728 entries = 76 KB of LDS: two workgroups per CU
constexpr int kHalo = 4096;                     // H: m <= 2048, the factors up to 2000
constexpr int kPayload = kStage - kHalo;        // C = 5632
constexpr int kStreamThreads = 256;
constexpr int kStreamItem = 16384;              // shifts per stream work item: 64 per lane

static_assert(kPayload > 0 && kHalo % 2 == 0, "tile geometry");

__device__ inline double wave_sum(double a) {
    for (int m = 32; m >= 1; m >>= 1) a += __shfl_xor(a, m, 64);
    return a;
}

__device__ inline double wave_inclusive(double v, int lane) {
    for (int d = 1; d < 64; d <<= 1) {
        const double o = __shfl_up(v, d, 64);
        if (lane >= d) v += o;
    }
    return v;
}

// s[0 .. kStage) in, s[i] = sum_{j<i} of them out (s[0] = 0); the caller has synchronised after filling s.
__device__ inline void block_exclusive_scan(double* s, double* wave_tot) {
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    double* seg = s + t * kSeg;
    double tot = 0.0;
#pragma unroll
    for (int i = 0; i < kSeg; ++i) tot += seg[i];
    const double inc = wave_inclusive(tot, lane);
    double run = __shfl_up(inc, 1, 64);
    if (lane == 0) run = 0.0;
    if (lane == 63) wave_tot[w] = inc;
    __syncthreads();
    double base = 0.0;
    for (int q = 0; q < w; ++q) base += wave_tot[q];
    run += base;
#pragma unroll
    for (int i = 0; i < kSeg; ++i) {
        const double v = seg[i];
        seg[i] = run;
        run += v;
    }
    __syncthreads();
}

// A non-finite sample (or shift) counts as NaN: it lies in some window of every factor, and every factor of the series is then
// NaN -- also where the exact sum would be +inf (an infinite last sample enters one window only).
__device__ inline double shifted(double v, double shift) {
    const double w = v - shift;
    return __builtin_isfinite(w) ? w : __builtin_nan("");
}

// stage samples [g0, g0 + kStage) of one series minus `shift`, zero past n
__device__ inline void stage(double* s, const double* __restrict__ xs, int64_t g0, int64_t n, double shift) {
    for (int i = threadIdx.x; i < kStage; i += kThreads) {
        const int64_t g = g0 + i;
        s[i] = g < n ? shifted(__builtin_nontemporal_load(&xs[g]), shift) : 0.0;
    }
    __syncthreads();
}

__global__ void __launch_bounds__(kThreads)
oallan_tile_kernel(const double* __restrict__ x, int64_t n, int64_t series_stride, OallanFactors F, int first, int count,
                   double* __restrict__ records) {
    __shared__ double s[kStage];
    __shared__ double wave_tot[kWaves];
    __shared__ double part[kOallanTileFactors * kWaves];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int tile = blockIdx.x;
    const int64_t sidx = blockIdx.y;
    const double* xs = x + sidx * series_stride;
    const int64_t k0 = (int64_t)tile * kPayload;            // < n - 2 m of the first factor: the grid has no tile beyond it
    stage(s, xs, k0, n, xs[k0]);
    block_exclusive_scan(s, wave_tot);
    for (int f = 0; f < count; ++f) {
        const int m = F.m[first + f];
        const int64_t left = n - 2 * (int64_t)m + 1 - k0;   // shifts of this factor from k0 on: k <= n - 2m
        const int kmax = left < kPayload ? (left < 0 ? 0 : (int)left) : kPayload;
        double acc = 0.0;
        for (int k = t; k < kmax; k += kThreads) {          // k + 2m <= C - 1 + H: inside the staging
            const double d = s[k + 2 * m] - 2.0 * s[k + m] + s[k];
            acc += d * d;
        }
        acc = wave_sum(acc);
        if (lane == 0) part[f * kWaves + w] = acc;
    }
    __syncthreads();
    if (t < count && tile < F.nparts[first + t]) {
        double sum = 0.0;
        for (int q = 0; q < kWaves; ++q) sum += part[t * kWaves + q];
        records[sidx * F.records + F.offset[first + t] + tile] = sum;
    }
}

// ---- stream form: theta of x - x[0]
__global__ void __launch_bounds__(kThreads)
oallan_chunk_sum_kernel(const double* __restrict__ x, int64_t n, int64_t series_stride, int nchunks, double* __restrict__ chunk_sums) {
    __shared__ double wave_tot[kWaves];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int64_t sidx = blockIdx.y;
    const double* xs = x + sidx * series_stride;
    const double shift = xs[0];
    const int64_t g0 = (int64_t)blockIdx.x * kStage;
    double acc = 0.0;
    for (int i = t; i < kStage; i += kThreads) {
        const int64_t g = g0 + i;
        if (g < n) acc += shifted(__builtin_nontemporal_load(&xs[g]), shift);
    }
    acc = wave_sum(acc);
    if (lane == 0) wave_tot[w] = acc;
    __syncthreads();
    if (t == 0) {
        double sum = 0.0;
        for (int q = 0; q < kWaves; ++q) sum += wave_tot[q];
        chunk_sums[sidx * nchunks + blockIdx.x] = sum;
    }
}

// one wavefront per series: the chunk sums become the chunks' bases, in place
__global__ void __launch_bounds__(64) oallan_chunk_scan_kernel(double* __restrict__ chunk_sums, int nchunks) {
    const int lane = threadIdx.x;
    double* cs = chunk_sums + (int64_t)blockIdx.x * nchunks;
    double carry = 0.0;
    for (int b = 0; b < nchunks; b += 64) {
        const int i = b + lane;
        const double v = i < nchunks ? cs[i] : 0.0;
        const double inc = wave_inclusive(v, lane);
        double ex = __shfl_up(inc, 1, 64);
        if (lane == 0) ex = 0.0;
        if (i < nchunks) cs[i] = carry + ex;
        carry += __shfl(inc, 63, 64);
    }
}

__global__ void __launch_bounds__(kThreads)
oallan_theta_kernel(const double* __restrict__ x, int64_t n, int64_t series_stride, int nchunks, const double* __restrict__ bases,
                    double* __restrict__ theta, int64_t theta_stride) {
    __shared__ double s[kStage];
    __shared__ double wave_tot[kWaves];
    const int64_t sidx = blockIdx.y;
    const double* xs = x + sidx * series_stride;
    const int64_t g0 = (int64_t)blockIdx.x * kStage;
    stage(s, xs, g0, n, xs[0]);
    block_exclusive_scan(s, wave_tot);
    const double base = bases[sidx * nchunks + blockIdx.x];
    double* th = theta + sidx * theta_stride;
    for (int i = threadIdx.x; i < kStage; i += kThreads) {
        const int64_t g = g0 + i;
        if (g <= n) th[g] = base + s[i];                    // theta has n + 1 entries
    }
}

__global__ void __launch_bounds__(kStreamThreads)
oallan_stream_kernel(const double* __restrict__ theta, int64_t n, int64_t theta_stride, OallanFactors F, int first,
                     double* __restrict__ records) {
    __shared__ double wave_tot[kStreamThreads / 64];
    const int f = first + blockIdx.z;
    const int item = blockIdx.x;
    if (item >= F.nparts[f]) return;                        // the whole workgroup: the grid is sized for the smallest factor
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int64_t sidx = blockIdx.y;
    const int64_t m = F.m[f];
    const int64_t terms = n - 2 * m + 1;
    const int64_t kb = (int64_t)item * kStreamItem;
    const int64_t ke = kb + kStreamItem < terms ? kb + kStreamItem : terms;
    const double* th = theta + sidx * theta_stride;
    double acc = 0.0;
    for (int64_t k = kb + t; k < ke; k += kStreamThreads) { // k + 2m <= n: theta's last entry
        const double a = __builtin_nontemporal_load(&th[k]);
        const double b = __builtin_nontemporal_load(&th[k + m]);
        const double c = __builtin_nontemporal_load(&th[k + 2 * m]);
        const double d = c - 2.0 * b + a;
        acc += d * d;
    }
    acc = wave_sum(acc);
    if (lane == 0) wave_tot[w] = acc;
    __syncthreads();
    if (t == 0) {
        double sum = 0.0;
        for (int q = 0; q < kStreamThreads / 64; ++q) sum += wave_tot[q];
        records[sidx * F.records + F.offset[f] + item] = sum;
    }
}

__global__ void __launch_bounds__(kOallanMaxFactors)
oallan_finish_kernel(const double* __restrict__ records, int64_t n, double ts, OallanFactors F, double* __restrict__ out) {
    const int i = threadIdx.x;
    if (i >= F.count) return;
    const int64_t sidx = blockIdx.x;
    const double* r = records + sidx * F.records + F.offset[i];
    double sum = 0.0;
    for (int p = 0; p < F.nparts[i]; ++p) sum += r[p];      // tiles ascending
    const double m = (double)F.m[i];
    const double terms = (double)(n - 2 * (int64_t)F.m[i] + 1);
    out[F.count + sidx * F.count + i] = sum / (2.0 * (m * m) * terms);
    if (sidx == 0) out[i] = m * ts;
}

}  // namespace

int oallan_tile_payload() { return kPayload; }
int oallan_tile_halo() { return kHalo; }
int oallan_scan_chunk() { return kStage; }
int oallan_stream_item() { return kStreamItem; }

hipError_t launch_oallan_tile(const double* x, int64_t n, int64_t series_stride, int32_t nseries, const OallanFactors& F, int first,
                              int count, double* records, hipStream_t st) {
    if (count < 1 || count > kOallanTileFactors) return hipErrorInvalidValue;
    hipLaunchKernelGGL(oallan_tile_kernel, dim3(F.nparts[first], nseries), dim3(kThreads), 0, st, x, n, series_stride, F, first, count,
                       records);
    return hipGetLastError();
}

hipError_t launch_oallan_theta(const double* x, int64_t n, int64_t series_stride, int32_t nseries, double* chunk_sums, double* theta,
                               int64_t theta_stride, hipStream_t st) {
    const int nchunks = (int)(n / kStage + 1);              // the chunk of theta[n] too
    hipLaunchKernelGGL(oallan_chunk_sum_kernel, dim3(nchunks, nseries), dim3(kThreads), 0, st, x, n, series_stride, nchunks, chunk_sums);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    // the series on x here: any count the other launches take
    hipLaunchKernelGGL(oallan_chunk_scan_kernel, dim3(nseries), dim3(64), 0, st, chunk_sums, nchunks);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(oallan_theta_kernel, dim3(nchunks, nseries), dim3(kThreads), 0, st, x, n, series_stride, nchunks, chunk_sums, theta,
                       theta_stride);
    return hipGetLastError();
}

hipError_t launch_oallan_stream(const double* theta, int64_t n, int64_t theta_stride, int32_t nseries, const OallanFactors& F, int first,
                                int count, double* records, hipStream_t st) {
    hipLaunchKernelGGL(oallan_stream_kernel, dim3(F.nparts[first], nseries, count), dim3(kStreamThreads), 0, st, theta, n, theta_stride, F,
                       first, records);
    return hipGetLastError();
}

hipError_t launch_oallan_finish(const double* records, int64_t n, int32_t nseries, double ts, const OallanFactors& F, double* out,
                                hipStream_t st) {
    hipLaunchKernelGGL(oallan_finish_kernel, dim3(nseries), dim3(kOallanMaxFactors), 0, st, records, n, ts, F, out);
    return hipGetLastError();
}

}  // namespace ginsim
