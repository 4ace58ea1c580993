// Device self-test patterns (ABI 9, include/ginsim.h "memory self-test"): a fill that writes a word unique to (tag, offset), a
// check that counts the words that differ from it, and an order-independent digest of a region.  They let a test hold every
// live region of the placed arena (csrc/placed.hip) to exactly its own bytes through growths and rebuilds: a word found in the
// wrong place names where it came from (another region's tag and offset: an alias; 0: a zero fill; a repeated byte: a memset).
// Plain global loads and stores, 64-bit indices, grid-stride loops; oracle/pattern.py spells out the same two formulas.
#include <hip/hip_runtime.h>

#include <cstdint>
#include "launch.hpp"

// The probe of ginsim_stream_first_xcc: where the FIRST workgroup of a launch on a stream lands, the accelerator complex die (XCD)
// of an MI300 / MI355X.  C linkage, outside the namespace: the recorded profiles and kernel traces know it by this plain name.
extern "C" __global__ void first_xcc_kernel(uint32_t* out) {
    if (threadIdx.x == 0) out[0] = __builtin_amdgcn_s_getreg((31 << 11) | 20) & 0xf;      // HW_REG_XCC_ID, bits 3:0
}

namespace ginsim {

namespace {

constexpr int TB = 256;
constexpr unsigned MAX_BLOCKS = 4096;

__device__ __forceinline__ uint64_t pattern_word(uint32_t tag, uint64_t i) { return ((uint64_t)tag << 40) | i; }

// the standard splitmix64 finaliser
__device__ __forceinline__ uint64_t splitmix64(uint64_t z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

unsigned blocks_for(uint64_t words) {
    const uint64_t b = (words + TB - 1) / TB;
    return (unsigned)(b < MAX_BLOCKS ? (b ? b : 1) : MAX_BLOCKS);
}

}  // namespace

__global__ void __launch_bounds__(TB) pattern_fill_kernel(uint64_t* __restrict__ p, uint64_t words, uint32_t tag) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < words; i += stride) p[i] = pattern_word(tag, i);
}

// out[0]: number of bad words (atomicAdd), out[1]: lowest bad word index (atomicMin; starts at ~0)
__global__ void __launch_bounds__(TB) pattern_check_kernel(const uint64_t* __restrict__ p, uint64_t words, uint32_t tag,
                                                           unsigned long long* __restrict__ out) {
    __shared__ unsigned long long s_bad, s_first;
    if (threadIdx.x == 0) { s_bad = 0; s_first = ~0ull; }
    __syncthreads();
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    unsigned long long bad = 0, first = ~0ull;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < words; i += stride) {
        if (p[i] != pattern_word(tag, i)) {
            ++bad;
            if (i < first) first = i;
        }
    }
    if (bad) {
        atomicAdd(&s_bad, bad);
        atomicMin(&s_first, first);
    }
    __syncthreads();
    if (threadIdx.x == 0 && s_bad) {
        atomicAdd(&out[0], s_bad);
        atomicMin(&out[1], s_first);
    }
}

// out[2] = the word at index out[1] (when a bad word was found)
__global__ void pattern_fetch_kernel(const uint64_t* __restrict__ p, unsigned long long* __restrict__ out) {
    if (threadIdx.x == 0 && blockIdx.x == 0 && out[0]) out[2] = p[out[1]];
}

// out[0] += sum over i of splitmix64(w_i ^ (i * 0x9E3779B97F4A7C15)) mod 2^64
__global__ void __launch_bounds__(TB) digest_kernel(const uint64_t* __restrict__ p, uint64_t words, unsigned long long* __restrict__ out) {
    __shared__ unsigned long long s_sum;
    if (threadIdx.x == 0) s_sum = 0;
    __syncthreads();
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    unsigned long long sum = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < words; i += stride)
        sum += splitmix64(p[i] ^ (i * 0x9E3779B97F4A7C15ull));
    atomicAdd(&s_sum, sum);
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(&out[0], s_sum);
}

__global__ void selftest_reset_kernel(unsigned long long* out) {
    if (threadIdx.x == 0 && blockIdx.x == 0) { out[0] = 0; out[1] = ~0ull; out[2] = 0; }
}

hipError_t launch_pattern_fill(void* p, uint64_t words, uint32_t tag, hipStream_t s) {
    hipLaunchKernelGGL(pattern_fill_kernel, dim3(blocks_for(words)), dim3(TB), 0, s, (uint64_t*)p, words, tag);
    return hipGetLastError();
}

// out: 3 device words (see the kernels); the results stay on the device until the caller copies them
hipError_t launch_pattern_check(const void* p, uint64_t words, uint32_t tag, unsigned long long* out, hipStream_t s) {
    hipLaunchKernelGGL(selftest_reset_kernel, dim3(1), dim3(64), 0, s, out);
    hipLaunchKernelGGL(pattern_check_kernel, dim3(blocks_for(words)), dim3(TB), 0, s, (const uint64_t*)p, words, tag, out);
    hipLaunchKernelGGL(pattern_fetch_kernel, dim3(1), dim3(64), 0, s, (const uint64_t*)p, out);
    return hipGetLastError();
}

hipError_t launch_digest(const void* p, uint64_t words, unsigned long long* out, hipStream_t s) {
    hipLaunchKernelGGL(selftest_reset_kernel, dim3(1), dim3(64), 0, s, out);
    hipLaunchKernelGGL(digest_kernel, dim3(blocks_for(words)), dim3(TB), 0, s, (const uint64_t*)p, words, out);
    return hipGetLastError();
}

// out: one device word, the die's number
hipError_t launch_first_xcc(uint32_t* out, hipStream_t s) {
    hipLaunchKernelGGL(first_xcc_kernel, dim3(1), dim3(64), 0, s, out);
    return hipGetLastError();
}

}  // namespace ginsim
