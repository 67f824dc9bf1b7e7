// mhx_resample.h -- the rule of the JACKKNIFE over the hashes of a sketch set (mhx_resample_rows, mhx_dist_nj_support) that does
// not depend on how a GPU runs it, as host+device functions: which hashes a replicate keeps, the threshold of a keep rate, and
// the steps of the order-preserving compaction of one chunk of a row.  The kernels in mhx_resample.hip call these functions;
// tests/emul/resample_emul.cpp runs the same text on the CPU.
//
// The rule.  A hash h is kept in replicate r (0-based) of a call with seed `seed` iff (z >> 32) < T, all arithmetic mod 2^64:
//     z = h + seed + (r + 1) * 0x9E3779B97F4A7C15
//     z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9
//     z = (z ^ (z >> 27)) * 0x94D049BB133111EB
//     z ^= z >> 31
// T = floor(keep * 2^32), computed once on the host from the double keep, 0 < keep <= 1; T may be 2^32 (everything is kept),
// and the product is exact.  The decision depends on the value of the hash alone: a hash that two lists share is kept in
// both or in neither, so every replicate is an honest sketch of the same random part of k-mer space.
// List i of a replicate is the kept hashes of list i, in order.  A list with len[i] == s is "full", a shorter one is a
// complete set, as Mash treats it.  s_r is the smallest kept count among the full lists, or s when no list is full; s_r == 0
// fails.  Every list is then cut to its first min(kept, s_r) hashes: without the cut the lists would be compared beyond the
// point to which each was sampled, with it every list is a bottom-s_r sketch.  The replicate's distances are those of the
// triangle over these lists at sketch size s_r, with the same k.
//
// The compaction.  A row is taken in chunks of kResampleThreads hashes, item x of a chunk by thread x.  A wave of 64 threads
// votes its keep flags into one 64-bit ballot; an item's place among the kept of its wave is the number of set bits below its
// lane, a wave's place in the chunk the sum of the totals of the waves before it, the chunk's place in the row the sum of the
// totals of the chunks before it.
#pragma once
#include "mhx_hd.h"

namespace mhx {

constexpr uint64_t kResampleGamma = 0x9E3779B97F4A7C15ull;
constexpr uint64_t kResampleMul1 = 0xBF58476D1CE4E5B9ull;
constexpr uint64_t kResampleMul2 = 0x94D049BB133111EBull;
constexpr uint32_t kResampleThreads = 256; // threads of a workgroup, hashes of a chunk
constexpr uint32_t kResampleWaves = kResampleThreads / 64;
constexpr uint32_t kResampleMaxReplicates = 10000;

MHX_HD uint64_t resample_mix(uint64_t h, uint64_t seed, uint32_t r)
{
    uint64_t z = h + seed + ((uint64_t)r + 1u) * kResampleGamma;
    z = (z ^ (z >> 30)) * kResampleMul1;
    z = (z ^ (z >> 27)) * kResampleMul2;
    return z ^ (z >> 31);
}
// T: 1 .. 2^32
MHX_HD bool resample_keeps(uint64_t h, uint64_t seed, uint32_t r, uint64_t T) { return (resample_mix(h, seed, r) >> 32) < T; }

// T of a keep rate; false: keep is outside (0, 1] or not a number.  Host.  (keep * 2^32 is exact: a scaling by a power of two)
inline bool resample_threshold(double keep, uint64_t *T)
{
    if (!(keep > 0.0) || !(keep <= 1.0)) return false;
    *T = (uint64_t)(keep * 4294967296.0);
    return true;
}

// ---- the compaction of one chunk ----------------------------------------------------------------------------------------------
MHX_HD uint32_t resample_popcount(uint64_t v) { return (uint32_t)__builtin_popcountll(v); }
// the kept items of the wave that lie below `lane`
MHX_HD uint32_t resample_lane_rank(uint64_t ballot, uint32_t lane) { return resample_popcount(ballot & ((1ull << lane) - 1ull)); }
// the kept items of the chunk in the waves before `wave`, and (*total) in all of them
MHX_HD uint32_t resample_wave_base(const uint32_t *wave_total, uint32_t wave, uint32_t *total)
{
    uint32_t before = 0, all = 0;
    for (uint32_t w = 0; w < kResampleWaves; ++w) {
        if (w < wave) before += wave_total[w];
        all += wave_total[w];
    }
    *total = all;
    return before;
}
// whether a list of `len` hashes takes part in s_r
MHX_HD bool resample_full(uint32_t len, uint32_t s) { return len == s; }

} // namespace mhx
