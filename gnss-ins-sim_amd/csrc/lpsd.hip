// One level of the decimating octave cascade (include/ginsim_lpsd.h): a half-band low-pass with a stride of two,
//
//     y[i] = h[M] x[2i + M] + sum_{m = 1, 3, .. 13} h[M + m] (x[2i + M - m] + x[2i + M + m]),   i = 0 .. n_out - 1,   M = 13
//
// with the 27 taps of halfband_table.inc, of which the 12 at even m != 0 are zero and are not evaluated: 15 samples per output.
// Only valid outputs are made, n_out = (n - 27) / 2 + 1.  The pair is added first, the terms are then added in ascending m onto
// the centre term, each as one fused multiply-add that the source spells: no compiler flag decides an output's bits, and they
// depend on its 27 inputs alone -- not on the tile, the series' neighbours, nseries or the launch.  No atomics.
//
// A workgroup owns one series (blockIdx.y) and one tile of kDecTile = 1024 outputs.  Its 256 lanes load the tile's 2 * 1024 + 25
// consecutive inputs, lane t the inputs t, t + 256, ..: every load instruction of a wavefront is 512 consecutive bytes.  The
// inputs go to LDS split by parity, input j to plane[j & 1][j >> 1], because the filter's stride of two would otherwise be the
// lanes' stride: output i reads the odd plane once, at i + 6 (the centre), and the even plane at i + 6 - q and i + 7 + q,
// q = 0 .. 6 -- consecutive lanes read consecutive doubles in all 15 reads.
// LDS banks (MI355X: an 8-byte read is served in two groups of 32 lanes over 64 banks of 4 bytes, an 8-byte write in four groups
// of 16 lanes over 32): 32 consecutive doubles are 64 consecutive banks, each once, whatever the first address: every read is
// conflict-free.  A write group is 16 consecutive inputs from a multiple of 16: 8 consecutive doubles of the even plane and 8 of
// the odd one, 16 banks each; the odd plane begins kPlaneE = 1048 doubles after the even one, 16 banks (mod 32) further, so the
// two runs never share a bank: every write is conflict-free as well.  (Unsplit, lanes 16 bytes apart put a read group's 32 lanes
// on 128 banks' worth of addresses: 2-way on every one of the 15 reads.)
// The kernel is bound by HBM: 8 bytes read and 4 written per input sample (the 25 inputs two tiles share come from L2), against
// 15 LDS reads and 8 flops per output.
#include "lpsd.hpp"

namespace ginsim {

namespace {

#include "halfband_table.inc"

constexpr int kTileInputs = 2 * kDecTile + kHalfbandTaps - 2;               // 2073
constexpr int kLoads = (kTileInputs + kDecThreads - 1) / kDecThreads;       // 9 per lane
constexpr int kPlaneE = 1048;                                               // even inputs 0 .. 2072: 1037 doubles, padded
constexpr int kPlaneO = 1040;                                               // odd inputs 1 .. 2071: 1036 doubles
static_assert(kPlaneE >= kDecTile + kHalfbandM && kPlaneE % 16 == 8, "the odd plane sits 16 banks (mod 32) after the even one");
static_assert(kPlaneO >= kDecTile + kHalfbandM - 1, "the odd plane");
static_assert(kDecTile % kDecThreads == 0, "outputs per lane");

__global__ void __launch_bounds__(kDecThreads)
decimate2_kernel(const double* __restrict__ x, int64_t n, int64_t n_out, int64_t series_stride, double* __restrict__ y,
                 int64_t y_stride) {
    __shared__ double plane[kPlaneE + kPlaneO];
    const int t = threadIdx.x;
    const int64_t sidx = blockIdx.y;
    const int64_t o0 = (int64_t)blockIdx.x * kDecTile;          // the tile's first output; its first input is 2 o0
    const double* xs = x + sidx * series_stride + 2 * o0;
    const int64_t left = n - 2 * o0;                            // inputs from there to the series' end: nothing past it is read
    double v[kLoads];
#pragma unroll
    for (int k = 0; k < kLoads; ++k) {
        const int j = t + k * kDecThreads;
        v[k] = (j < kTileInputs && j < left) ? xs[j] : 0.0;
    }
#pragma unroll
    for (int k = 0; k < kLoads; ++k) {
        const int j = t + k * kDecThreads;
        if (j < kTileInputs) plane[(j & 1) * kPlaneE + (j >> 1)] = v[k];
    }
    __syncthreads();
    double* ys = y + sidx * y_stride + o0;
    const int64_t outs = n_out - o0;                            // valid outputs from the tile's first: output i reads the inputs
                                                                // 2i .. 2i + 26 <= 2 (outs - 1) + 26 < left
#pragma unroll
    for (int k = 0; k < kDecTile / kDecThreads; ++k) {
        const int i = t + k * kDecThreads;
        if (i < outs) {
            const double* e = plane + i;
            double acc = kHalfbandCentre * plane[kPlaneE + i + 6];
            acc = __builtin_fma(kHalfbandPair[0], e[6] + e[7], acc);
            acc = __builtin_fma(kHalfbandPair[1], e[5] + e[8], acc);
            acc = __builtin_fma(kHalfbandPair[2], e[4] + e[9], acc);
            acc = __builtin_fma(kHalfbandPair[3], e[3] + e[10], acc);
            acc = __builtin_fma(kHalfbandPair[4], e[2] + e[11], acc);
            acc = __builtin_fma(kHalfbandPair[5], e[1] + e[12], acc);
            acc = __builtin_fma(kHalfbandPair[6], e[0] + e[13], acc);
            ys[i] = acc;
        }
    }
}

// out[s][k] = dens[s][first + k], k = 0 .. bins - 1: a level's reported bins from its finished densities (rows of `full`) to
// their columns of the call's output (rows of `pitch`; pinned host memory, written once)
__global__ void __launch_bounds__(256)
lpsd_report_kernel(const double* __restrict__ dens, int32_t full, int32_t first, int32_t bins, double* __restrict__ out, int32_t pitch) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= bins) return;
    const int64_t sidx = blockIdx.y;
    out[sidx * pitch + k] = dens[sidx * full + first + k];
}

}  // namespace

hipError_t launch_lpsd_report(const double* dens, int32_t nseries, int32_t full, int32_t first, int32_t bins, double* out, int32_t pitch,
                              hipStream_t st) {
    if (bins < 1 || first < 0 || first + bins > full || bins > pitch || nseries < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(lpsd_report_kernel, dim3((bins + 255) / 256, nseries), dim3(256), 0, st, dens, full, first, bins, out, pitch);
    return hipGetLastError();
}

hipError_t launch_decimate2(const double* x, int64_t n, int64_t series_stride, int32_t nseries, double* y, int64_t y_stride,
                            hipStream_t st) {
    const int64_t n_out = decimate2_outputs(n);
    const int64_t tiles = decimate2_tiles(n_out);
    if (tiles < 1 || tiles > kDecMaxTiles || nseries < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(decimate2_kernel, dim3((unsigned)tiles, nseries), dim3(kDecThreads), 0, st, x, n, n_out, series_stride, y, y_stride);
    return hipGetLastError();
}

}  // namespace ginsim
