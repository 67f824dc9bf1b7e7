// tests/emul/resample_emul.cpp -- CPU emulator of the jackknife kernels (mhx_resample.hip, test tool).  Runs the host+device
// functions of auriclass_amd/csrc/mhx_resample.h themselves over whole calls, phase by phase as a workgroup of 256 threads
// runs them: per chunk of a row every thread's keep flag, the four 64-lane ballots, the waves' totals (what goes through
// LDS), every kept item's place from the set bits below its lane and the totals before its wave, and the stores; then the
// count, the minimum over the full rows, and the second launch that cuts every row and zeroes the rest up to the stride.
// The threads of a phase run in descending order: nothing in a phase may depend on the order.  Not part of the product;
// built by tests/test_resample_emulation.py with g++.
#include <cstdint>
#include "../../auriclass_amd/csrc/mhx_resample.h"

using namespace mhx;

extern "C" uint64_t emul_resample_mix(uint64_t h, uint64_t seed, uint32_t r) { return resample_mix(h, seed, r); }
extern "C" int emul_resample_keeps(uint64_t h, uint64_t seed, uint32_t r, uint64_t T) { return resample_keeps(h, seed, r, T) ? 1 : 0; }
extern "C" int emul_resample_threshold(double keep, uint64_t *T) { return resample_threshold(keep, T) ? 1 : 0; }

// One replicate of rows [n][stride] / len [n] into out_rows / out_len, which the caller has filled with anything; *s_r as the
// kernels leave it.  Returns the number of stores of the first launch that fell outside their row (0 when all is well).
extern "C" uint64_t emul_resample_call(const uint64_t *rows, const uint32_t *len, uint32_t n, uint32_t stride, uint32_t s, uint64_t seed, uint32_t replicate,
                                       uint64_t T, uint64_t *out_rows, uint32_t *out_len, uint32_t *s_r)
{
    uint64_t outside = 0;
    *s_r = s; // the memset in front of the first launch
    for (uint32_t i = n; i-- > 0;) { // one workgroup per row, in any order
        const uint32_t full_len = len[i], row_len = full_len < stride ? full_len : stride;
        const uint64_t *row = rows + (uint64_t)i * stride;
        uint64_t *out = out_rows + (uint64_t)i * stride;
        uint32_t kept = 0;
        for (uint32_t c0 = 0; c0 < row_len; c0 += kResampleThreads) {
            uint64_t h[kResampleThreads], ballot[kResampleWaves] = {};
            bool keep[kResampleThreads];
            uint32_t wave_total[kResampleWaves];
            for (uint32_t x = kResampleThreads; x-- > 0;) { // loads and flags
                const uint32_t j = c0 + x;
                h[x] = j < row_len ? row[j] : 0;
                keep[x] = j < row_len && resample_keeps(h[x], seed, replicate, T);
            }
            for (uint32_t x = kResampleThreads; x-- > 0;) // the vote of every wave
                if (keep[x]) ballot[x >> 6] |= 1ull << (x & 63u);
            for (uint32_t w = kResampleWaves; w-- > 0;) wave_total[w] = resample_popcount(ballot[w]); // lane 0 of every wave, to LDS
            uint32_t total = 0;
            for (uint32_t x = kResampleThreads; x-- > 0;) { // behind the barrier: places and stores
                const uint32_t before = resample_wave_base(wave_total, x >> 6, &total);
                if (!keep[x]) continue;
                const uint32_t at = kept + before + resample_lane_rank(ballot[x >> 6], x & 63u);
                if (at >= stride) { ++outside; continue; }
                out[at] = h[x];
            }
            kept += total;
        }
        out_len[i] = kept;
        if (resample_full(full_len, s) && kept < *s_r) *s_r = kept; // atomicMin
    }
    for (uint32_t i = 0; i < n; ++i) { // the second launch
        const uint32_t cut = out_len[i] < *s_r ? out_len[i] : *s_r;
        uint64_t *out = out_rows + (uint64_t)i * stride;
        for (uint32_t j = stride; j-- > cut;) out[j] = 0;
        out_len[i] = cut;
    }
    return outside;
}
