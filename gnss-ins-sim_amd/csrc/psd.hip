// Welch power spectral density (include/ginsim_psd.h): for segments seg_s = x[sD .. sD + L) of one series,
//
//     y_s[k] = (seg_s[k] - mean(seg_s)) w[k],   X_s = DFT_L(y_s),   P[k] = c_k / (K fs U) sum_s |X_s[k]|^2,   k = 0 .. L/2
//
// Part kernel: a workgroup owns one series (blockIdx.y) and one part, segs_per_part consecutive segments (psd.hpp).  It takes
// its segments two at a time as ONE complex transform z = y_a + i y_b; then |X_a[k]|^2 + |X_b[k]|^2 = (|Z[k]|^2 + |Z[L-k]|^2) / 2,
// so the two spectra are never separated: the workgroup only adds |Z|^2.  An odd last segment pairs with zeros.
//   - load, balanced-tree means, cosine table, the swizzled LDS planes and the radix-2 stages but the last: welch_core.hpp (the
//     overlap of consecutive segments was read by this workgroup one transform earlier and comes back from L2, not from HBM);
//   - the last stage (twiddle 1) is not written back: its two outputs are squared and added to the lane's registers, L / T
//     doubles per lane, one per POSITION of the bit-reversed array;
//   - at the end of the part the sums per position go to LDS once and bin k is folded from positions rev(k) and rev(L - k).
// Finish kernel: adds the parts' records in ascending order and scales (welch_core.hpp).  A series' records depend on that
// series alone.
#include "welch_core.hpp"

namespace ginsim {

namespace {

using namespace welch;

template <int L>
__global__ void __launch_bounds__(Geom<L>::T)
psd_part_kernel(const double* __restrict__ x, int64_t series_stride, int32_t D, int32_t window, int32_t detrend, int64_t K,
                int32_t segs_per_part, int32_t nparts, double* __restrict__ records) {
    using G = Geom<L>;
    constexpr int T = G::T, W = G::W, E = G::E, B = G::B, LOG2L = G::LOG2L;
    __shared__ double re[L];
    __shared__ double im[L];
    __shared__ double C[psd_table_doubles(L)];
    __shared__ double wave_tot[2 * W];
    const int t = threadIdx.x;
    const int part = blockIdx.x;
    const int64_t sidx = blockIdx.y;
    const double* xs = x + sidx * series_stride;

    double w[E];
    make_table_and_window<L>(C, window, w);
    double acc[2 * B];
#pragma unroll
    for (int b = 0; b < 2 * B; ++b) acc[b] = 0.0;
    bool bad = false;

    const int64_t s_begin = (int64_t)part * segs_per_part;
    const int64_t s_end = s_begin + segs_per_part < K ? s_begin + segs_per_part : K;
    for (int64_t s = s_begin; s < s_end; s += 2) {
        const double* pa = xs + s * D;                          // segment s: samples sD .. sD + L - 1 <= (K-1) D + L - 1 < n
        load_rows<L>(pa, pa + D, s + 1 < s_end, detrend, w, re, im, wave_tot, bad);
        dif_stages<L>(re, im, C);
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
    finish_planes<1>(records, nparts, nbins, 0, scale, out);
}

}  // namespace

hipError_t launch_psd_parts(const double* x, int64_t series_stride, int32_t nseries, int32_t D, int32_t window, int32_t detrend,
                            const PsdShape& s, double* records, hipStream_t st) {
    const int32_t nparts = (int32_t)s.nparts;                   // at most kPsdMaxParts: the glue has refused the rest
    return for_segment_length<kPsdMaxLog2>(s.log2L, [&](auto length) {
        constexpr int L = length;
        static_assert(psd_lds_bytes(L) <= 160 * 1024, "the workgroup's LDS");
        hipLaunchKernelGGL(psd_part_kernel<L>, dim3(nparts, nseries), dim3(Geom<L>::T), 0, st, x, series_stride, D, window, detrend,
                           s.segments, s.segs_per_part, nparts, records);
        return hipGetLastError();
    });
}

hipError_t launch_psd_finish(const double* records, int32_t nseries, const PsdShape& s, double scale, double* out, hipStream_t st) {
    hipLaunchKernelGGL(psd_finish_kernel, dim3((s.nbins + 255) / 256, nseries), dim3(256), 0, st, records, (int32_t)s.nparts, s.nbins, scale, out);
    return hipGetLastError();
}

}  // namespace ginsim
