// Welch cross-spectral density (include/ginsim_csd.h): for segments segx_s = x[sD .. sD + L), segy_s = y[sD .. sD + L)
// of a pair of series,
//
//     X_s = DFT_L((segx_s - mean(segx_s)) w),  Y_s likewise,   sums over s of |X_s[k]|^2, |Y_s[k]|^2, conj(X_s[k]) Y_s[k],  k = 0 .. L/2
//
// Part kernel: a workgroup owns one pair (blockIdx.y) and one part, segs_per_part consecutive segments (psd.hpp's partition).  It
// transforms segment s of BOTH series as one complex transform z = yx + i yy, as psd.hip transforms two segments of one series, and
// then separates the two spectra per segment: with A = Z[k], B = conj(Z[L-k]), X = (A + B) / 2 and Y = (A - B) / (2i).  The four
// sums are added from the separated X and Y -- never from |A|^2, |B|^2 and A conj(B) recombined at the end, which cancels when one
// series is much smaller than the other.
//   - load, balanced-tree means (one per series), cosine table, the swizzled LDS planes (plane_slot) and the radix-2 stages but
//     the last: welch_core.hpp, the code psd.hip runs;
//   - the mirror bin: the transform leaves Z[k] at position rev(k) of the array.  Bins 0 .. L/2 - 1 are the EVEN positions 2j
//     (k = rev(2j) has a clear top bit) and their mirrors L - k the odd ones; bin L/2 is position 1.  The last stage's butterfly j
//     produces positions 2j and 2j + 1 in lane registers, so a lane keeps the even output -- its own bin -- and writes only the odd
//     one back.  Negation in bit-reversed order is the complement plus a carry that runs from the top bit down:
//     rev(L - rev(p)) = p ^ (2^m - 1) with m the highest set bit of p, so butterfly j >= 1 finds its mirror at position 2 j' + 1 with
//     j' = j ^ (2^floor(log2 j) - 1).  Butterfly 0 has both self-mirrored bins, 0 and L/2, in its own registers.
//   - LDS pattern of the mirror read: 64 consecutive j >= 64 share floor(log2 j), so j' runs over 64 consecutive butterflies in
//     descending order; the lanes j < 64 read a permutation of butterflies 0 .. 63.  Either way a wavefront reads the 64 odd
//     positions of 128 consecutive elements, each once: the access set of the last stage's own reads of its odd inputs, which
//     plane_slot serves without a bank conflict (32 lanes at a time: 16 odd columns of an even row and, reversed, 16 even columns of
//     the odd row next to it).  The write-back of the odd outputs is 2-way like the writes of the stages with h < 16.
//   - accumulators: four per butterfly and lane in registers, and three more for bin L/2, which only thread 0 adds to.
//   - at the end of the part the sums go to LDS by BIN (the four planes of L/2 sums fill the two planes of the transform) and
//     from there to the record [pair][part][4][L/2 + 1] in coalesced rows.
// Finish kernel: adds the parts' records in ascending order and scales (welch_core.hpp).  A pair's records depend on its two
// series alone.
#include "csd.hpp"
#include "welch_core.hpp"

namespace ginsim {

namespace {

using namespace welch;

template <int L>
__global__ void __launch_bounds__(Geom<L>::T)
csd_part_kernel(const double* __restrict__ x, int64_t series_stride, const int32_t* __restrict__ pairs, int32_t D, int32_t window,
                int32_t detrend, int64_t K, int32_t segs_per_part, int32_t nparts, double* __restrict__ records) {
    using G = Geom<L>;
    constexpr int T = G::T, W = G::W, E = G::E, B = G::B, LOG2L = G::LOG2L, NB = L / 2 + 1;
    __shared__ double zz[2 * L];
    __shared__ double C[psd_table_doubles(L)];
    __shared__ double wave_tot[2 * W];
    double* const re = zz;
    double* const im = zz + L;
    const int t = threadIdx.x;
    const int part = blockIdx.x;
    const int64_t pidx = blockIdx.y;
    const double* xs = x + (int64_t)pairs[2 * pidx] * series_stride;
    const double* ys = x + (int64_t)pairs[2 * pidx + 1] * series_stride;

    double w[E];
    make_table_and_window<L>(C, window, w);
    // 4 sums per butterfly, of 2 X and 2 Y (the factor 4 leaves with the record); edge: bin L/2, thread 0 alone
    double acc[4 * B], edge[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int b = 0; b < 4 * B; ++b) acc[b] = 0.0;
    bool bad = false;

    const int64_t s_begin = (int64_t)part * segs_per_part;
    const int64_t s_end = s_begin + segs_per_part < K ? s_begin + segs_per_part : K;
    for (int64_t s = s_begin; s < s_end; ++s) {
        // segment s: samples sD .. sD + L - 1 <= (K-1) D + L - 1 < n; the load's first barrier also ends the previous segment's
        // mirror reads of re / im
        load_rows<L>(xs + s * D, ys + s * D, true, detrend, w, re, im, wave_tot, bad);
        dif_stages<L>(re, im, C);
        // last stage (twiddle 1): the even output Z[rev(2j)] stays here, the odd one goes back for the lane whose mirror it is
        double er[B], ei[B];
#pragma unroll
        for (int b = 0; b < B; ++b) {
            const int j = t + b * T;
            er[b] = ei[b] = 0.0;
            if (j < L / 2) {
                const int p0 = plane_slot(2 * j), p1 = plane_slot(2 * j + 1);
                const double ar = re[p0], ai = im[p0], br = re[p1], bi = im[p1];
                const double dr = ar - br, di = ai - bi;
                er[b] = ar + br;
                ei[b] = ai + bi;
                re[p1] = dr;
                im[p1] = di;
                if (j == 0) {                                   // bin L/2: X = Re Z[L/2], Y = Im Z[L/2]
                    edge[0] += dr * dr;
                    edge[1] += di * di;
                    edge[2] += dr * di;
                }
            }
        }
        __syncthreads();
#pragma unroll
        for (int b = 0; b < B; ++b) {
            const int j = t + b * T;
            if (j < L / 2) {
                // A = Z[k] = er + i ei;  Z[L - k] = mr + i mi, for bin 0 Z[0] itself;  B = conj(Z[L - k])
                double mr = er[b], mi = ei[b];
                if (j > 0) {
                    const int jm = j ^ ((1 << (31 - __clz(j))) - 1);
                    const int pm = plane_slot(2 * jm + 1);
                    mr = re[pm];
                    mi = im[pm];
                }
                const double xr = er[b] + mr, xi = ei[b] - mi;  // 2 X = A + B
                const double yr = ei[b] + mi, yi = mr - er[b];  // 2 Y = (A - B) / i
                acc[4 * b] += xr * xr + xi * xi;
                acc[4 * b + 1] += yr * yr + yi * yi;
                acc[4 * b + 2] += xr * yr + xi * yi;            // conj(X) Y
                acc[4 * b + 3] += xr * yi - xi * yr;
            }
        }
        if (W == 1) __syncthreads();                            // one wavefront: no barrier in the mean, so one here
    }

    // the sums by bin: plane q at zz[q L/2 ..), bin k = rev(2j) of butterfly j; then the record in coalesced rows
    __syncthreads();
#pragma unroll
    for (int b = 0; b < B; ++b) {
        const int j = t + b * T;
        if (j < L / 2) {
            const int k = (int)(__brev((unsigned)(2 * j)) >> (32 - LOG2L));
#pragma unroll
            for (int q = 0; q < 4; ++q) zz[q * (L / 2) + k] = 0.25 * acc[4 * b + q];
        }
    }
    __syncthreads();
    const double nan = __builtin_nan("");
    double* rec = records + (pidx * nparts + part) * (int64_t)(kCsdPlanes * NB);
    for (int i = t; i < 4 * (L / 2); i += T) {
        const int q = i / (L / 2), k = i - q * (L / 2);
        double v = zz[i];
        if (q == 3 && k == 0) v = 0.0;                          // X and Y of bin 0 are real
        rec[q * NB + k] = bad ? nan : v;
    }
    if (t == 0) {
        rec[L / 2] = bad ? nan : edge[0];
        rec[NB + L / 2] = bad ? nan : edge[1];
        rec[2 * NB + L / 2] = bad ? nan : edge[2];
        rec[3 * NB + L / 2] = bad ? nan : 0.0;
    }
}

__global__ void __launch_bounds__(256)
csd_finish_kernel(const double* __restrict__ records, int32_t nparts, int32_t nbins, int32_t npairs, double scale, double* __restrict__ out) {
    finish_planes<kCsdPlanes>(records, nparts, nbins, npairs, scale, out);
}

}  // namespace

hipError_t launch_csd_parts(const double* x, int64_t series_stride, const int32_t* pairs, int32_t npairs, int32_t D, int32_t window,
                            int32_t detrend, const PsdShape& s, double* records, hipStream_t st) {
    const int32_t nparts = (int32_t)s.nparts;                   // at most kPsdMaxParts: the glue has refused the rest
    return for_segment_length<kCsdMaxLog2>(s.log2L, [&](auto length) {
        constexpr int L = length;
        static_assert(csd_lds_bytes(L) <= 160 * 1024, "the workgroup's LDS");
        hipLaunchKernelGGL(csd_part_kernel<L>, dim3(nparts, npairs), dim3(Geom<L>::T), 0, st, x, series_stride, pairs, D, window,
                           detrend, s.segments, s.segs_per_part, nparts, records);
        return hipGetLastError();
    });
}

hipError_t launch_csd_finish(const double* records, int32_t npairs, const PsdShape& s, double scale, double* out, hipStream_t st) {
    hipLaunchKernelGGL(csd_finish_kernel, dim3((kCsdPlanes * s.nbins + 255) / 256, npairs), dim3(256), 0, st, records,
                       (int32_t)s.nparts, s.nbins, npairs, scale, out);
    return hipGetLastError();
}

}  // namespace ginsim
