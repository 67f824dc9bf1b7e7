// mhx_block.h -- device-only workgroup helpers shared by the kernel files (no host+device rule lives here: those are in
// mhx_tile.h, mhx_tighten.h, mhx_screen.h, mhx_dist.h, where the CPU emulators of the tests can include them).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mhx {

// inclusive prefix sum over the 64 lanes of a wave.  PRECONDITION: all 64 lanes are active (a DPP row operation reads
// the registers of its source lanes as they stand, whether those lanes run or not).
//   default          six v_add_u32_dpp: row_shr:1/2/4/8 scan each row of 16 lanes, row_bcast:15 adds the sum of row 0 to
//                    row 1 and of row 2 to row 3, row_bcast:31 adds the sum of rows 0 and 1 to rows 2 and 3.  A lane
//                    without a source (the first lanes of a row, the rows a row mask leaves out) adds `old` = 0.
//   -DMHX_SCAN_SHFL  the shuffle form, six __shfl_up steps of eight instructions and one LDS round trip (ds_bpermute_b32)
//                    each: the reference and the A/B build (profiles/parse_front_ab.txt)
__device__ __forceinline__ uint32_t wave_scan_incl(uint32_t v)
{
#ifdef MHX_SCAN_SHFL
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t t = __shfl_up(v, o);
        if (lane >= o) v += t;
    }
#else
    v += __builtin_amdgcn_update_dpp(0u, v, 0x111, 0xf, 0xf, false); // row_shr:1
    v += __builtin_amdgcn_update_dpp(0u, v, 0x112, 0xf, 0xf, false); // row_shr:2
    v += __builtin_amdgcn_update_dpp(0u, v, 0x114, 0xf, 0xf, false); // row_shr:4
    v += __builtin_amdgcn_update_dpp(0u, v, 0x118, 0xf, 0xf, false); // row_shr:8  -> every row scanned
    v += __builtin_amdgcn_update_dpp(0u, v, 0x142, 0xa, 0xf, false); // row_bcast:15 into rows 1 and 3
    v += __builtin_amdgcn_update_dpp(0u, v, 0x143, 0xc, 0xf, false); // row_bcast:31 into rows 2 and 3
#endif
    return v;
}

// exclusive prefix sum over the THREADS threads of a workgroup (wave_scan_incl + one partial per wave through LDS,
// wave_sums[THREADS / 64]); every thread also gets the workgroup total.  One barrier.
// PRECONDITION: entered by the whole workgroup, THREADS a multiple of 64, with all 64 lanes of every wave active -- the
// barrier inside asks for the first, the wave scan for the second.
template <int THREADS> __device__ __forceinline__ uint32_t block_scan_excl(uint32_t value, uint32_t *wave_sums, uint32_t &total)
{
    static_assert(THREADS % 64 == 0, "whole waves");
    const int lane = threadIdx.x & 63;
    const uint32_t v = wave_scan_incl(value);
#ifdef MHX_SCAN_SHFL
    const int wave = threadIdx.x >> 6;
#else
    // wave-uniform, and told so: the sums in front of this wave are then picked on the scalar unit
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
#endif
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
