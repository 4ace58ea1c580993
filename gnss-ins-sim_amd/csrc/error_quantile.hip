// Error quantiles across the runs: the radius that holds a given share of the runs (CEP50, CEP95 / R95) and the same quantiles of
// the vertical and the 3-D error, at every requested sample.  Two kernels, both over kept trajectory planes:
//
//   radial_keys_kernel    per (sample, run) the error of position or velocity against the truth (sample_error, moments.hpp, the
//                         expression of error_curve.hip) and from it three non-negative KEYS: horizontal sqrt(e0^2 + e1^2),
//                         vertical |e2|, 3-D sqrt(e0^2 + e1^2 + e2^2), written to keys[(k * m + s) * row_stride + col0 + r].
//                         row_stride and col0 let blocks of runs (and devices) fill one long row per (key, sample).
//   quantile_rows_kernel  exact order statistics of every key row for up to 8 probabilities at once: nearest rank
//                         (np.quantile(method='inverted_cdf')), the k-th smallest finite key, k = min(max(ceil(p N), 1), N).
//
// Keys: the unit of work is a WAVEFRONT, as in error_curve.hip: one sample and one slice of the run axis, lanes stride along the
// runs (coalesced loads and stores), the truth row is wave-uniform (scalar loads), no LDS, no barrier.  Only the three planes of
// the selected quantity are read: 24 B (fp64) per sample*run in, 24 B out.
//
// Select: one workgroup per row, MSB-first radix select with 8-bit digits.  A finite double x orders as the integer
// u(x) = bits ^ (sign ? ~0 : 1 << 63) (for the non-negative keys above: the bit pattern itself), so eight passes fix u of the
// wanted key digit by digit: a pass counts, for every probability, the digit of the keys that carry that probability's prefix
// (LDS histogram of 256 counters, LDS atomics), one wavefront per probability scans its histogram, picks the digit that holds the
// wanted rank and narrows prefix and rank.  Pass 0 has one prefix (none) and therefore one histogram; its total is N, the number
// of finite keys.  The counters are integers: the order of the atomics cannot change them, the same row gives the same bits at
// every launch.  Nothing is sorted or moved, the result is one of the keys bit for bit.  Rows of at most kSelStage keys are copied
// to LDS once and every pass reads them there; longer rows are read again per pass from global memory (a 65 536-key row is 512 KiB:
// it stays in L2).  Keys that are not finite are left out (-0.0 orders before +0.0).
#include <hip/hip_runtime.h>
#include "ginsim.h"
#include "moments.hpp"
#include "launch.hpp"

namespace ginsim {

constexpr int kKeysBlock = 256;                     // four wavefronts, each with its own (sample, slice)
constexpr int kKeysWaves = kKeysBlock / 64;
constexpr int kKeysMaxParts = 1024;
constexpr int64_t kKeysTargetWaves = 8192;          // 256 CUs x 4 SIMDs x 8 wavefronts

typedef const int64_t __attribute__((address_space(4))) * uniform_idx;

// the slices of the run axis for `m` samples of `runs` runs: one wavefront per sample when there are many samples, else enough
// slices to fill the device (a slice holds at least one step of a wavefront)
static int keys_parts(int64_t runs, int64_t m) {
    const int64_t most = (runs + 63) / 64;
    int64_t want = (kKeysTargetWaves + m - 1) / m;
    if (want > most) want = most;
    if (want > kKeysMaxParts) want = kKeysMaxParts;
    return (int)(want < 1 ? 1 : want);
}

// which: 0 position (planes 3..5), 1 velocity (planes 6..8).  NED: the position error in local NED metres (lla_error_ned), a
// template parameter as in curve_partial_kernel; it has no effect on the velocity.  org: the origin table of the fp32 displacement
// series (T = float), added to the position in fp64 exactly as curve_partial_kernel adds it.
template <typename T, bool NED>
__global__ void __launch_bounds__(kKeysBlock) radial_keys_kernel(const T* __restrict__ traj, const double* __restrict__ ref, int64_t n,
                                                                int64_t runs, const int64_t* __restrict__ samples, int64_t m, int parts,
                                                                int which, double* __restrict__ keys, int64_t row_stride, int64_t col0,
                                                                const ProcOrigin org) {
    const int lane = threadIdx.x & 63;
    const int64_t unit = (int64_t)blockIdx.x * kKeysWaves + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (unit >= m * parts) return;                  // wave-uniform
    const int64_t s = unit / parts;
    const int part = (int)(unit - s * parts);
    const int64_t j = samples ? ((uniform_idx)(uintptr_t)samples)[s] : s;
    const int64_t plane = n * runs;
    const int c0 = which ? 6 : 3;
    const uniform_ref truth = (uniform_ref)(uintptr_t)ref;
    const double t0 = truth[9 * j + c0], t1 = truth[9 * j + c0 + 1], t2 = truth[9 * j + c0 + 2];
    const T* row = traj + c0 * plane + j * runs;
    double* out = keys + s * row_stride + col0;
    const int64_t kstep = m * row_stride;           // from one key's rows to the next key's
    for (int64_t r = (int64_t)part * 64 + lane; r < runs; r += (int64_t)parts * 64) {
        const double a0 = (double)row[r], a1 = (double)row[plane + r], a2 = (double)row[2 * plane + r];
        double x[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, t[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, e[9];
        double e0, e1, e2;
        if (which) {                                // wave-uniform
            x[6] = a0; x[7] = a1; x[8] = a2;
            t[6] = t0; t[7] = t1; t[8] = t2;
            sample_error(x, t, 0, e);
            e0 = e[6]; e1 = e[7]; e2 = e[8];
        } else {
            double o0 = 0.0, o1 = 0.0, o2 = 0.0;
            if (org.table) {                        // the run's initial state, as in the MC kernels (moments.hpp, ProcOrigin)
                const uint64_t call = org.ini_first + (uint64_t)r;
                const double* o = org.table + 3 * (call < (uint64_t)org.n_ini ? call : 0);
                o0 = o[0]; o1 = o[1]; o2 = o[2];
            }
            x[3] = a0 + o0; x[4] = a1 + o1; x[5] = a2 + o2;
            t[3] = t0; t[4] = t1; t[5] = t2;
            sample_error(x, t, NED ? 1 : 0, e);
            e0 = e[3]; e1 = e[4]; e2 = e[5];
        }
        const double h2 = e0 * e0 + e1 * e1;
        out[r] = sqrt(h2);
        out[kstep + r] = fabs(e2);
        out[2 * kstep + r] = sqrt(h2 + e2 * e2);
    }
}

template <typename T>
static hipError_t launch_keys(const T* traj, const double* ref, int64_t n, int64_t runs, const int64_t* samples, int64_t m, int which,
                              int pos_ned, double* keys, int64_t row_stride, int64_t col0, const ProcOrigin org, hipStream_t st) {
    const int parts = keys_parts(runs, m);
    const unsigned blocks = (unsigned)((m * parts + kKeysWaves - 1) / kKeysWaves);
    hipLaunchKernelGGL((pos_ned ? radial_keys_kernel<T, true> : radial_keys_kernel<T, false>), dim3(blocks), dim3(kKeysBlock), 0, st, traj,
                       ref, n, runs, samples, m, parts, which, keys, row_stride, col0, org);
    return hipGetLastError();
}

hipError_t launch_radial_keys(const double* traj, const double* ref, int64_t n, int64_t runs, const int64_t* samples, int64_t m,
                              int which, int pos_ned, double* keys, int64_t row_stride, int64_t col0, hipStream_t st) {
    return launch_keys<double>(traj, ref, n, runs, samples, m, which, pos_ned, keys, row_stride, col0, ProcOrigin{nullptr, 0, 0}, st);
}

hipError_t launch_radial_keys_f32(const float* traj, const double* ref, int64_t n, int64_t runs, const int64_t* samples, int64_t m,
                                  int which, int pos_ned, double* keys, int64_t row_stride, int64_t col0, const double* origin,
                                  int64_t n_ini, uint64_t ini_first, hipStream_t st) {
    return launch_keys<float>(traj, ref, n, runs, samples, m, which, pos_ned, keys, row_stride, col0, ProcOrigin{origin, n_ini, ini_first},
                              st);
}

// ------------------------------------------------------------------------------------------------------------------ the select
constexpr int kSelBlock = 1024;                     // sixteen wavefronts per row: a long row is read from L2 with many loads in flight
constexpr int kSelStage = 4096;                     // a row of at most this many keys is staged in LDS (32 KiB) and read there
constexpr int kSelMaxQ = GINSIM_QUANTILE_MAX_PROBS;
constexpr int kSelBatch = 4;                        // loads of a lane in flight per step over a row in global memory
constexpr uint64_t kSelSkip = 0x7FF8000000000000ull;        // a NaN: what a lane past the end of the row holds

__device__ __forceinline__ bool key_finite(uint64_t b) { return (b & 0x7FF0000000000000ull) != 0x7FF0000000000000ull; }
// finite doubles order as these integers; key_bits is the way back
__device__ __forceinline__ uint64_t key_order(uint64_t b) { return b ^ ((b >> 63) ? ~0ull : 0x8000000000000000ull); }
__device__ __forceinline__ uint64_t key_bits(uint64_t u) { return u ^ ((u >> 63) ? 0x8000000000000000ull : ~0ull); }

__device__ __forceinline__ uint64_t uniform64(uint64_t v) {
    return ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32)) << 32) |
           (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
}

// One more key with digit d, called by the lanes whose key carries the prefix.  The keys of a row share their leading digits
// (sign, exponent), so most lanes of a wavefront hit one counter: the lanes that hold the digit of the first active lane are
// counted with one atomic, the others add for themselves.
__device__ __forceinline__ void hist_add(unsigned* h, unsigned d) {
    const unsigned first = (unsigned)__builtin_amdgcn_readfirstlane((int)d);
    const unsigned long long same = __ballot(d == first);
    if (d == first) {
        if ((int)(threadIdx.x & 63) == __ffsll((long long)same) - 1) atomicAdd(h + first, (unsigned)__popcll(same));
    } else {
        atomicAdd(h + d, 1u);
    }
}

// pre[j]: the digits above `shift + 8` that probability j has fixed (pass > 0); nh: the histograms of this pass
__device__ __forceinline__ void count_key(uint64_t b, int pass, int shift, int nh, const uint64_t (&pre)[kSelMaxQ],
                                          unsigned (*hist)[256]) {
    if (!key_finite(b)) return;
    const uint64_t u = key_order(b);
    const unsigned d = (unsigned)(u >> shift) & 255u;
    const uint64_t hi = pass ? u >> (shift + 8) : 0;
#pragma unroll
    for (int j = 0; j < kSelMaxQ; ++j)
        if (j < nh && hi == pre[j]) hist_add(hist[j], d);
}

// keys: rows of `len` doubles, row_stride apart; probs: device [q]; out: device [rows][q]; count: device [rows]
__global__ void __launch_bounds__(kSelBlock) quantile_rows_kernel(const double* __restrict__ keys, int64_t len, int64_t row_stride,
                                                                  const double* __restrict__ probs, int q, double* __restrict__ out,
                                                                  double* __restrict__ count) {
    __shared__ uint64_t stage[kSelStage];
    __shared__ __attribute__((aligned(16))) unsigned hist[kSelMaxQ][256];
    __shared__ uint64_t s_prefix[kSelMaxQ];
    __shared__ unsigned s_rank[kSelMaxQ];
    __shared__ unsigned s_n;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const uint64_t* row = reinterpret_cast<const uint64_t*>(keys) + (int64_t)blockIdx.x * row_stride;
    const bool staged = len <= kSelStage;
    if (staged)
        for (int i = tid; i < (int)len; i += kSelBlock) stage[i] = row[i];
    for (int pass = 0; pass < 8; ++pass) {
        const int shift = 56 - 8 * pass;
        const int nh = pass ? q : 1;
        for (int i = tid; i < nh * 256; i += kSelBlock) (&hist[0][0])[i] = 0u;
        __syncthreads();
        uint64_t pre[kSelMaxQ];
#pragma unroll
        for (int j = 0; j < kSelMaxQ; ++j) pre[j] = (pass && j < nh) ? uniform64(s_prefix[j]) >> (shift + 8) : 0;
        if (staged) {
            for (int i = tid; i < (int)len; i += kSelBlock) count_key(stage[i], pass, shift, nh, pre, hist);
        } else {
            for (int64_t i0 = tid; i0 < len; i0 += kSelBatch * kSelBlock) {
                uint64_t b[kSelBatch];
#pragma unroll
                for (int k = 0; k < kSelBatch; ++k) {
                    const int64_t i = i0 + (int64_t)k * kSelBlock;
                    b[k] = i < len ? row[i] : kSelSkip;
                }
#pragma unroll
                for (int k = 0; k < kSelBatch; ++k) count_key(b[k], pass, shift, nh, pre, hist);
            }
        }
        __syncthreads();
        if (w < q) {                                // wavefront w scans the histogram of probability w: four counters per lane
            const uint4 c = *reinterpret_cast<const uint4*>(&hist[pass ? w : 0][4 * lane]);
            const unsigned sum = c.x + c.y + c.z + c.w;
            unsigned incl = sum;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const unsigned v = __shfl_up(incl, off, 64);
                if (lane >= off) incl += v;
            }
            const unsigned total = __shfl(incl, 63, 64);
            unsigned rank;
            if (pass == 0) {                        // total = N, the finite keys of the row; the rank wanted: nearest rank
                if (tid == 0) {
                    s_n = total;
                    count[blockIdx.x] = (double)total;
                }
                const double want = ceil(probs[w] * (double)total);     // one fp64 product
                rank = want < 1.0 ? 1u : want > (double)total ? total : (unsigned)want;
            } else {
                rank = s_rank[w];
            }
            const unsigned excl = incl - sum;
            if (total > 0u && excl < rank && rank <= incl) {            // the one lane whose four counters hold the rank
                unsigned d = 4u * lane, base = excl;
                if (base + c.x < rank) {
                    base += c.x; ++d;
                    if (base + c.y < rank) {
                        base += c.y; ++d;
                        if (base + c.z < rank) { base += c.z; ++d; }
                    }
                }
                s_prefix[w] = (pass ? s_prefix[w] : 0ull) | ((uint64_t)d << shift);
                s_rank[w] = rank - base;
            }
        }
        __syncthreads();
        if (s_n == 0u) break;                       // no finite key in the row (block-uniform)
    }
    if (w < q && lane == 0) {
        const uint64_t b = s_n ? key_bits(s_prefix[w]) : kSelSkip;
        out[(int64_t)blockIdx.x * q + w] = __longlong_as_double((long long)b);
    }
}

hipError_t launch_quantile_rows(const double* keys, int64_t rows, int64_t len, int64_t row_stride, const double* probs, int q,
                                double* out, double* count, hipStream_t st) {
    hipLaunchKernelGGL(quantile_rows_kernel, dim3((unsigned)rows), dim3(kSelBlock), 0, st, keys, len, row_stride, probs, q, out, count);
    return hipGetLastError();
}

}  // namespace ginsim
