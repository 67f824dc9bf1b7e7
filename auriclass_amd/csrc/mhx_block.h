// mhx_block.h -- device-only workgroup helpers shared by the kernel files (no host+device rule lives here: those are in
// mhx_tile.h, mhx_tighten.h, mhx_screen.h, mhx_dist.h, where the CPU emulators of the tests can include them).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mhx {

// exclusive prefix sum over the THREADS threads of a workgroup (wave shuffles + one partial per wave through LDS,
// wave_sums[THREADS / 64]); every thread also gets the workgroup total.  One barrier.
template <int THREADS> __device__ __forceinline__ uint32_t block_scan_excl(uint32_t value, uint32_t *wave_sums, uint32_t &total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t v = value;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t t = __shfl_up(v, o);
        if (lane >= o) v += t;
    }
    if (lane == 63) wave_sums[wave] = v;
    __syncthreads();
    uint32_t base = 0, all = 0;
#pragma unroll
    for (int w = 0; w < THREADS / 64; ++w) {
        const uint32_t x = wave_sums[w];
        if (w < wave) base += x;
        all += x;
    }
    total = all;
    return base + v - value;
}

} // namespace mhx
