// Error quantiles across the runs: the radius that holds a given share of the runs (CEP50, CEP95 / R95) and the same quantiles of
// the vertical and the 3-D error, at every requested sample.  Two kernels, both over kept trajectory planes:
//
//   radial_keys_kernel    per (sample, run) the error of position or velocity against the truth (quantity_error,
//                         traj_error.hpp) and from it three non-negative KEYS: horizontal sqrt(e0^2 + e1^2),
//                         vertical |e2|, 3-D sqrt(e0^2 + e1^2 + e2^2), written to keys[(k * m + s) * row_stride + col0 + r].
//                         row_stride and col0 let blocks of runs (and devices) fill one long row per (key, sample).
//   quantile_rows_kernel  exact order statistics of every key row for up to 8 probabilities at once: nearest rank
//                         (np.quantile(method='inverted_cdf')), the k-th smallest finite key, k = min(max(ceil(p N), 1), N).
//
// Keys: the unit of work and the cut of the run axis are traj_error.hpp's (coalesced loads and stores).  Only the three planes of
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
#include "traj_error.hpp"

namespace ginsim {

constexpr int kKeysMaxParts = 1024;

// which, NED, org: see quantity_error (traj_error.hpp)
template <typename T, bool NED>
__global__ void __launch_bounds__(kUnitBlock) radial_keys_kernel(const T* __restrict__ traj, const double* __restrict__ ref, int64_t n,
                                                                int64_t runs, const int64_t* __restrict__ samples, int64_t m, int parts,
                                                                int which, double* __restrict__ keys, int64_t row_stride, int64_t col0,
                                                                const ProcOrigin org) {
    const int lane = threadIdx.x & 63;
    const int64_t unit = wave_unit();
    if (unit >= m * parts) return;
    const WorkUnit w(unit, ref, n, runs, samples, parts);
    const int64_t j = w.j, plane = w.plane;
    const int c0 = which ? 6 : 3;
    const double t0 = w.truth[9 * j + c0], t1 = w.truth[9 * j + c0 + 1], t2 = w.truth[9 * j + c0 + 2];
    const T* row = traj + c0 * plane + j * runs;
    double* out = keys + w.s * row_stride + col0;
    const int64_t kstep = m * row_stride;           // from one key's rows to the next key's
    const int part = (int)(unit - w.s * parts);
    for (int64_t r = (int64_t)part * 64 + lane; r < runs; r += (int64_t)parts * 64) {
        double e[3];
        quantity_error<NED>((double)row[r], (double)row[plane + r], (double)row[2 * plane + r], t0, t1, t2, which, org, r, e);
        // the fused form is spelt out: left to the compiler's contraction, which product is fused, and so every key's rounding, is its choice
        const double h2 = __builtin_fma(e[1], e[1], e[0] * e[0]);
        out[r] = sqrt(h2);
        out[kstep + r] = fabs(e[2]);
        out[2 * kstep + r] = sqrt(__builtin_fma(e[2], e[2], h2));
    }
}

template <typename T>
static hipError_t launch_keys(const TrajView& v, int which, int pos_ned, double* keys, int64_t row_stride, int64_t col0, hipStream_t st) {
    const int parts = run_slices(v.runs, v.m, 64, kKeysMaxParts);
    hipLaunchKernelGGL((pos_ned ? radial_keys_kernel<T, true> : radial_keys_kernel<T, false>), dim3(unit_blocks(v.m, parts)),
                       dim3(kUnitBlock), 0, st, static_cast<const T*>(v.traj), v.ref, v.n, v.runs, v.samples, v.m, parts, which, keys,
                       row_stride, col0, v.org);
    return hipGetLastError();
}

hipError_t launch_radial_keys(const TrajView& v, int which, int pos_ned, double* keys, int64_t row_stride, int64_t col0, hipStream_t st) {
    return v.f32 ? launch_keys<float>(v, which, pos_ned, keys, row_stride, col0, st)
                 : launch_keys<double>(v, which, pos_ned, keys, row_stride, col0, st);
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
