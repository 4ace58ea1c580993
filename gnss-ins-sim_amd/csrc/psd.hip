// Welch power spectral density (include/ginsim_psd.h): for segments seg_s = x[sD .. sD + L) of one series,
//
//     y_s[k] = (seg_s[k] - mean(seg_s)) w[k],   X_s = DFT_L(y_s),   P[k] = c_k / (K fs U) sum_s |X_s[k]|^2,   k = 0 .. L/2
//
// Part kernel: a workgroup owns one series (blockIdx.y) and one part, segs_per_part consecutive segments (psd.hpp).  It takes
// its segments two at a time as ONE complex transform z = y_a + i y_b; then |X_a[k]|^2 + |X_b[k]|^2 = (|Z[k]|^2 + |Z[L-k]|^2) / 2,
// so the two spectra are never separated: the workgroup only adds |Z|^2.  An odd last segment pairs with zeros.
//   - load: lane t takes samples t, t + T, ... of both segments into registers (the overlap of consecutive segments was read
//     by this workgroup one transform earlier and comes back from L2, not from HBM);
//   - mean: a balanced tree in a fixed order -- the lane's samples pairwise, the wavefront by xor shuffles, the wavefronts'
//     totals pairwise from LDS -- log2(L) levels in all; a total that is not finite marks the part (NaN at every bin);
//   - the detrended, windowed samples go to LDS as two planes of doubles (re, im);
//   - transform in place: radix-2 decimation in frequency, natural order in, bit-reversed order out, one butterfly per lane and
//     stage step, a barrier per stage; the last stage (twiddle 1) is not written back: its two outputs are squared and added
//     to the lane's registers, L / T doubles per lane, one per POSITION of the bit-reversed array;
//   - at the end of the part the sums per position go to LDS once and bin k is folded from positions rev(k) and rev(L - k).
// Twiddles and the Hann window come from one table C[q] = cospi(2 q / L), q = 0 .. L/4, made per workgroup in LDS:
// cos and sin of every multiple of 2 pi / L up to pi are +-C at a mirrored index.
// LDS banks (64 of 4 bytes; an 8-byte read is served 32 lanes at a time over all 64, an 8-byte write 16 lanes at a time over 32):
// a stage of half size h < 32 has 32 consecutive butterflies on 32 of the 64 doubles of two rows, the same 32 columns in both;
// the planes therefore store element i at i ^ 31 in odd rows (plane_slot), which turns the second row's columns into the
// complement: every read of every stage is conflict-free; the writes of the stages with h < 16 are 2-way.  The table is read at
// strides L / 2h, powers of two up to L/4: padded by one entry per 32 and one per 1024 (psd_table_slot) its 32 lanes hit 32
// distinct banks or the same address.
// Finish kernel: adds the parts' records in ascending order and scales.  No atomics: every sum has one fixed order, and a
// series' records depend on that series alone.
#include "psd.hpp"

namespace ginsim {

namespace {

__device__ inline int plane_slot(int i) { return i ^ (-((i >> 5) & 1) & 31); }

template <int L>
struct PsdGeom {
    static constexpr int T = psd_threads(L);
    static constexpr int W = T / 64;
    static constexpr int E = L / T > 1 ? L / T : 1;             // samples per lane and segment
    static constexpr int B = L / 2 / T > 1 ? L / 2 / T : 1;     // butterflies per lane and stage
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

template <int L>
__global__ void __launch_bounds__(PsdGeom<L>::T)
psd_part_kernel(const double* __restrict__ x, int64_t series_stride, int32_t D, int32_t window, int32_t detrend, int64_t K,
                int32_t segs_per_part, int32_t nparts, double* __restrict__ records) {
    using G = PsdGeom<L>;
    constexpr int T = G::T, W = G::W, E = G::E, B = G::B, LOG2L = __builtin_ctz(L);
    __shared__ double re[L];
    __shared__ double im[L];
    __shared__ double C[psd_table_doubles(L)];
    __shared__ double wave_tot[2 * W];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int part = blockIdx.x;
    const int64_t sidx = blockIdx.y;
    const double* xs = x + sidx * series_stride;

    for (int q = t; q <= L / 4; q += T) C[psd_table_slot(q)] = cospi(2.0 * (double)q / (double)L);
    __syncthreads();
    double w[E];
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const int i = t + e * T;
        w[e] = 1.0;
        if (window == 1 && i < L) w[e] = 0.5 - 0.5 * table_cos<L>(C, i <= L / 2 ? i : L - i);
    }
    double acc[2 * B];
#pragma unroll
    for (int b = 0; b < 2 * B; ++b) acc[b] = 0.0;
    bool bad = false;

    const int64_t s_begin = (int64_t)part * segs_per_part;
    const int64_t s_end = s_begin + segs_per_part < K ? s_begin + segs_per_part : K;
    for (int64_t s = s_begin; s < s_end; s += 2) {
        const bool second = s + 1 < s_end;
        const double* pa = xs + s * D;                          // segment s: samples sD .. sD + L - 1 <= (K-1) D + L - 1 < n
        const double* pb = pa + D;
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
        // the stages stay a loop: unrolled, their addresses (invariant from one pair to the next) are all hoisted and spilled
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
                    re[p1] = dr * c + di * sn;                  // (dr + i di) (c - i sn)
                    im[p1] = di * c - dr * sn;
                }
            }
            __syncthreads();
        }
#pragma unroll
        for (int b = 0; b < B; ++b) {
            const int j = t + b * T;
            if (j < L / 2) {
                const int p0 = plane_slot(2 * j), p1 = plane_slot(2 * j + 1);
                const double ar = re[p0], ai = im[p0], br = re[p1], bi = im[p1];
                const double sr = ar + br, si = ai + bi, dr = ar - br, di = ai - bi;
                acc[2 * b] += sr * sr + si * si;
                acc[2 * b + 1] += dr * dr + di * di;
            }
        }
        if (W == 1) __syncthreads();                            // one wavefront: no barrier in the mean, so one here
    }

    __syncthreads();
#pragma unroll
    for (int b = 0; b < B; ++b) {
        const int j = t + b * T;
        if (j < L / 2) {
            re[plane_slot(2 * j)] = acc[2 * b];
            re[plane_slot(2 * j + 1)] = acc[2 * b + 1];
        }
    }
    __syncthreads();
    double* rec = records + (sidx * nparts + part) * (int64_t)(L / 2 + 1);
    for (int k = t; k <= L / 2; k += T) {
        const int r1 = (int)(__brev((unsigned)k) >> (32 - LOG2L));
        const int r2 = (int)(__brev((unsigned)((L - k) & (L - 1))) >> (32 - LOG2L));
        const double v = 0.5 * (re[plane_slot(r1)] + re[plane_slot(r2)]);
        rec[k] = bad ? __builtin_nan("") : v;
    }
}

__global__ void __launch_bounds__(256)
psd_finish_kernel(const double* __restrict__ records, int32_t nparts, int32_t nbins, double scale, double* __restrict__ out) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= nbins) return;
    const int64_t sidx = blockIdx.y;
    const double* r = records + sidx * nparts * (int64_t)nbins + k;
    double sum = 0.0;
    for (int p = 0; p < nparts; ++p) sum += r[(int64_t)p * nbins];      // parts ascending
    out[sidx * nbins + k] = sum * ((k == 0 || k == nbins - 1) ? scale : 2.0 * scale);
}

template <int L>
hipError_t launch_parts(const double* x, int64_t series_stride, int32_t nseries, int32_t D, int32_t window, int32_t detrend,
                        const PsdShape& s, double* records, hipStream_t st) {
    static_assert(psd_lds_bytes(L) <= 160 * 1024, "the workgroup's LDS");
    const int32_t nparts = (int32_t)s.nparts;                   // at most kPsdMaxParts: the glue has refused the rest
    hipLaunchKernelGGL(psd_part_kernel<L>, dim3(nparts, nseries), dim3(PsdGeom<L>::T), 0, st, x, series_stride, D, window, detrend,
                       s.segments, s.segs_per_part, nparts, records);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_psd_parts(const double* x, int64_t series_stride, int32_t nseries, int32_t D, int32_t window, int32_t detrend,
                            const PsdShape& s, double* records, hipStream_t st) {
    switch (s.log2L) {
#define GINSIM_PSD_CASE(N) case N: return launch_parts<(1 << N)>(x, series_stride, nseries, D, window, detrend, s, records, st);
        GINSIM_PSD_CASE(3) GINSIM_PSD_CASE(4) GINSIM_PSD_CASE(5) GINSIM_PSD_CASE(6) GINSIM_PSD_CASE(7) GINSIM_PSD_CASE(8)
        GINSIM_PSD_CASE(9) GINSIM_PSD_CASE(10) GINSIM_PSD_CASE(11) GINSIM_PSD_CASE(12) GINSIM_PSD_CASE(13)
#undef GINSIM_PSD_CASE
    }
    return hipErrorInvalidValue;
}

hipError_t launch_psd_finish(const double* records, int32_t nseries, const PsdShape& s, double scale, double* out, hipStream_t st) {
    hipLaunchKernelGGL(psd_finish_kernel, dim3((s.nbins + 255) / 256, nseries), dim3(256), 0, st, records, (int32_t)s.nparts, s.nbins, scale, out);
    return hipGetLastError();
}

}  // namespace ginsim
