// The transform core of the Welch part kernels: what psd.hip and csd.hip do alike to two rows of L samples, stated
// once.  Both make ONE complex transform z = y_a + i y_b of two real rows -- two segments of one series there, one segment of two
// series here -- with y = (row - mean(row)) w, and differ only in the last stage and in what they add up from it.
//   - load: lane t takes samples t, t + T, ... of both rows into registers;
//   - mean: a balanced tree in a fixed order -- the lane's samples pairwise, the wavefront by xor shuffles, the wavefronts'
//     totals pairwise from LDS -- log2(L) levels in all; a total that is not finite marks the part (NaN at every bin);
//   - the detrended, windowed samples go to LDS as two planes of doubles (re, im);
//   - transform in place: radix-2 decimation in frequency, natural order in, bit-reversed order out, one butterfly per lane and
//     stage step, a barrier per stage.  The last stage (twiddle 1) is the caller's: neither kernel writes it back whole.
// Twiddles and the Hann window come from one table C[q] = cospi(2 q / L), q = 0 .. L/4, made per workgroup in LDS:
// cos and sin of every multiple of 2 pi / L up to pi are +-C at a mirrored index.
// LDS banks (64 of 4 bytes; an 8-byte read is served 32 lanes at a time over all 64, an 8-byte write 16 lanes at a time over 32):
// a stage of half size h < 32 has 32 consecutive butterflies on 32 of the 64 doubles of two rows, the same 32 columns in both;
// the planes therefore store element i at i ^ 31 in odd rows (plane_slot), which turns the second row's columns into the
// complement: every read of every stage is conflict-free; the writes of the stages with h < 16 are 2-way.  The table is read at
// strides L / 2h, powers of two up to L/4: padded by one entry per 32 and one per 1024 (psd_table_slot) its 32 lanes hit 32
// distinct banks or the same address.
// Behind the device code: the finish kernel's body for any number of planes, and the choice of an instantiation by log2(L).
#pragma once
#include <type_traits>
#include "psd.hpp"

namespace ginsim {
namespace welch {

__device__ inline int plane_slot(int i) { return i ^ (-((i >> 5) & 1) & 31); }

template <int L>
struct Geom {
    static constexpr int T = psd_threads(L);
    static constexpr int W = T / 64;
    static constexpr int E = L / T > 1 ? L / T : 1;             // samples per lane and row
    static constexpr int B = L / 2 / T > 1 ? L / 2 / T : 1;     // butterflies per lane and stage
    static constexpr int LOG2L = __builtin_ctz(L);
};

// cos(2 pi q / L) and sin(2 pi q / L) for 0 <= q <= L/2 from the quarter table
template <int L>
__device__ inline double table_cos(const double* C, int q) {
    return q <= L / 4 ? C[psd_table_slot(q)] : -C[psd_table_slot(L / 2 - q)];
}
template <int L>
__device__ inline double table_sin(const double* C, int q) {
    return C[psd_table_slot(q <= L / 4 ? L / 4 - q : q - L / 4)];
}

// v[0 .. N) added as a balanced tree (N a power of two); v is left as it is
template <int N>
__device__ inline double tree_sum(const double (&v)[N]) {
    if constexpr (N == 1) {
        return v[0];
    } else {
        double h[N / 2];
#pragma unroll
        for (int i = 0; i < N / 2; ++i) h[i] = v[i] + v[i + N / 2];
        return tree_sum(h);
    }
}

__device__ inline double wave_tree(double a) {
    for (int m = 32; m >= 1; m >>= 1) a += __shfl_xor(a, m, 64);
    return a;
}

// the workgroup's table C (psd_table_doubles(L) doubles of LDS), barrier included, and the window weights of this lane's samples
template <int L>
__device__ __forceinline__ void make_table_and_window(double* C, int32_t window, double (&w)[Geom<L>::E]) {
    constexpr int T = Geom<L>::T, E = Geom<L>::E;
    const int t = threadIdx.x;
    for (int q = t; q <= L / 4; q += T) C[psd_table_slot(q)] = cospi(2.0 * (double)q / (double)L);
    __syncthreads();
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const int i = t + e * T;
        w[e] = 1.0;
        if (window == 1 && i < L) w[e] = 0.5 - 0.5 * table_cos<L>(C, i <= L / 2 ? i : L - i);
    }
}

// rows pa[0 .. L) and, if `second`, pb[0 .. L) (zeros otherwise) -> re, im: detrended if `detrend`, windowed, swizzled; bad is
// set when a row's total is not finite.  wave_tot: 2 W doubles of LDS, untouched by a single wavefront.  Ends with the barrier.
template <int L>
__device__ __forceinline__ void load_rows(const double* pa, const double* pb, bool second, int32_t detrend,
                                          const double (&w)[Geom<L>::E], double* re, double* im, double* wave_tot, bool& bad) {
    constexpr int T = Geom<L>::T, W = Geom<L>::W, E = Geom<L>::E;
    const int t = threadIdx.x;
    double va[E], vb[E];
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const int i = t + e * T;
        va[e] = i < L ? pa[i] : 0.0;
        vb[e] = (second && i < L) ? pb[i] : 0.0;
    }
    double sa = wave_tree(tree_sum(va)), sb = wave_tree(tree_sum(vb));
    if (W > 1) {
        // the barrier also ends the previous transform's last reads of re / im
        const int lane = t & 63, wv = t >> 6;
        if (lane == 0) { wave_tot[2 * wv] = sa; wave_tot[2 * wv + 1] = sb; }
        __syncthreads();
        double qa[W], qb[W];
#pragma unroll
        for (int q = 0; q < W; ++q) { qa[q] = wave_tot[2 * q]; qb[q] = wave_tot[2 * q + 1]; }
        sa = tree_sum(qa);
        sb = tree_sum(qb);
    }
    bad = bad || !__builtin_isfinite(sa) || !__builtin_isfinite(sb);
    const double ma = detrend ? sa * (1.0 / L) : 0.0, mb = detrend ? sb * (1.0 / L) : 0.0;
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const int i = t + e * T;
        if (i < L) {
            re[plane_slot(i)] = (va[e] - ma) * w[e];
            im[plane_slot(i)] = second ? (vb[e] - mb) * w[e] : 0.0;
        }
    }
    __syncthreads();
}

// the stages of half size h = L/2 .. 2, a barrier behind each; the last one (h = 1, twiddle 1) is left to the caller
template <int L>
__device__ __forceinline__ void dif_stages(double* re, double* im, const double* C) {
    constexpr int T = Geom<L>::T, B = Geom<L>::B, LOG2L = Geom<L>::LOG2L;
    const int t = threadIdx.x;
    // the stages stay a loop: unrolled, their addresses (invariant from one transform to the next) are all hoisted and spilled
#pragma unroll 1
    for (int lh = LOG2L - 1; lh >= 1; --lh) {
        const int h = 1 << lh;
#pragma unroll
        for (int b = 0; b < B; ++b) {
            const int j = t + b * T;
            if (j < L / 2) {
                const int pos = j & (h - 1);
                const int i0 = ((j - pos) << 1) + pos, i1 = i0 + h;
                const int p0 = plane_slot(i0), p1 = plane_slot(i1);
                const int q = pos << (LOG2L - 1 - lh);
                const double c = table_cos<L>(C, q), sn = table_sin<L>(C, q);
                const double ar = re[p0], ai = im[p0], br = re[p1], bi = im[p1];
                const double dr = ar - br, di = ai - bi;
                re[p0] = ar + br;
                im[p0] = ai + bi;
                re[p1] = dr * c + di * sn;                      // (dr + i di) (c - i sn)
                im[p1] = di * c - dr * sn;
            }
        }
        __syncthreads();
    }
}

// Finish kernels, grid (ceil(P nbins / 256), sets) of 256 threads: element e = plane * nbins + k of a set's P planes,
// out[plane][set][k] = c_k * scale * (the parts' records [set][part][P][nbins] added in ascending order).  No atomics: every sum
// has one fixed order.  With one plane q is 0 and nsets is not read.
template <int P>
__device__ __forceinline__ void finish_planes(const double* __restrict__ records, int32_t nparts, int32_t nbins, int32_t nsets,
                                              double scale, double* __restrict__ out) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= P * nbins) return;
    int q = 0, k = e;
    if constexpr (P > 1) { q = e / nbins; k = e - q * nbins; }
    const int64_t set = blockIdx.y;
    const int64_t per = (int64_t)P * nbins;
    const double* r = records + set * nparts * per + e;
    double sum = 0.0;
    for (int p = 0; p < nparts; ++p) sum += r[(int64_t)p * per];        // parts ascending
    out[((int64_t)q * nsets + set) * nbins + k] = sum * ((k == 0 || k == nbins - 1) ? scale : 2.0 * scale);
}

// f(std::integral_constant<int, L>()) for L = 2^log2L, kPsdMinLog2 <= log2L <= MAXLOG2: the launchers' choice of an instantiation
template <int MAXLOG2, int N = kPsdMinLog2, class F>
hipError_t for_segment_length(int log2L, F&& f) {
    if constexpr (N > MAXLOG2) {
        return hipErrorInvalidValue;
    } else {
        return log2L == N ? f(std::integral_constant<int, (1 << N)>()) : for_segment_length<MAXLOG2, N + 1>(log2L, f);
    }
}

}  // namespace welch
}  // namespace ginsim
