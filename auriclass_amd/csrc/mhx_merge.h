// mhx_merge.h -- what the sharded path's merge computes per element, as host+device inline functions: the kernels of
// mhx_merge.hip and merge_slabs_impl (mhx_engine.cpp) call these and keep no copy of their own, and the CPU emulator
// tests/emul/merge_emul.cpp runs the very same text over whole calls.  The rule they implement:
//   an entry (hash, count) of slab r counts when its index < n_r, hash <= T_min = min_r T_r and hash != 2^64-1 (the value
//   no table can hold: it travels in header word 3); counts of equal hashes are summed and clamped at 2^32-1; sums >= m,
//   ascending, first s are the sketch of the union.
#pragma once
#include <math.h>
#include <stdint.h>
#include "mhx_device_consts.h"
#include "mhx_hd.h"

namespace mhx {

constexpr uint32_t kMaxMergeRanks = 64;   // ranks per launch (more: the table path, several launches)
constexpr uint32_t kMergeMaxBins = 16384, kMergeMaxSlots = 4096; // LDS: 2 x 4 bytes per bin in the scatter pass, 12 per slot in the bin pass
constexpr uint32_t kMergeMaxQual = 1024;  // qualifying entries a bin can rank in LDS
// flags word of the binned merge; any of them sends the call on to the table path
constexpr uint32_t kMergeFlagRegion = 1;  // a bin's region overflowed
constexpr uint32_t kMergeFlagTable = 2;   // a bin's LDS table would be more than 3/4 full (guard)
constexpr uint32_t kMergeFlagQual = 4;    // more than kMergeMaxQual entries qualify in one bin
constexpr uint32_t kMergeFlagWrap = 8;    // a summed count passed 2^32-1: the 32-bit add wrapped, the table path saturates instead
// which path produced the answer of the last merge (mhx_sketcher_merge_info)
constexpr uint32_t kMergePathNone = 0, kMergePathBinned = 1, kMergePathTable = 2, kMergePathHost = 3;

// ---- atomics: HIP's in device code, plain read-modify-write on the host (the emulator runs one virtual thread at a time)
#if defined(__HIP_DEVICE_COMPILE__)
__device__ __forceinline__ uint32_t merge_atomic_add(uint32_t *p, uint32_t v) { return atomicAdd(p, v); }
__device__ __forceinline__ uint32_t merge_atomic_cas(uint32_t *p, uint32_t expect, uint32_t v) { return atomicCAS(p, expect, v); }
__device__ __forceinline__ unsigned long long merge_atomic_cas(unsigned long long *p, unsigned long long expect, unsigned long long v) { return atomicCAS(p, expect, v); }
#else
inline uint32_t merge_atomic_add(uint32_t *p, uint32_t v) { const uint32_t o = *p; *p = o + v; return o; }
inline uint32_t merge_atomic_cas(uint32_t *p, uint32_t expect, uint32_t v) { const uint32_t o = *p; if (o == expect) *p = v; return o; }
inline unsigned long long merge_atomic_cas(unsigned long long *p, unsigned long long expect, unsigned long long v) { const unsigned long long o = *p; if (o == expect) *p = v; return o; }
#endif

// ---- geometry of the binned merge ------------------------------------------------------------------------------------
struct MergeGeometry {
    uint32_t nbins;        // power of two, 256 .. kMergeMaxBins: 1024 entries per bin on average when all bins are used
    uint32_t shift;        // bin of a hash = hash >> shift (< nbins for every hash <= t_min)
    uint32_t region;       // entries a bin's region holds: the average fill, six standard deviations and 64
    uint32_t table_slots;  // LDS table of the bin pass: power of two, region <= 3/4 of it
    uint64_t bins_used;    // bins that hashes <= t_min can fall into: nbins/2 + 1 .. nbins, fewer for t_min < nbins
};

// false: not the binned path (too many ranks, nothing to merge, more entries than kMergeMaxBins bins of 1024 take, or a
// region beyond the largest LDS table -- few bins in use under a tiny t_min)
inline bool merge_geometry(uint64_t total, uint64_t t_min, uint32_t n_ranks, MergeGeometry &g)
{
    g.nbins = g.shift = g.region = g.table_slots = 0;
    g.bins_used = 0;
    if (n_ranks > kMaxMergeRanks || total == 0 || total > (uint64_t)kMergeMaxBins * 1024) return false;
    uint32_t nbins = 256;
    while ((uint64_t)nbins * 1024 < total) nbins <<= 1;
    const uint32_t lg = (uint32_t)__builtin_ctz(nbins);
    const uint32_t bits = 64u - (uint32_t)__builtin_clzll(t_min | 1ull);
    g.nbins = nbins;
    g.shift = bits > lg ? bits - lg : 0u;
    g.bins_used = (t_min >> g.shift) + 1;
    const double avg = (double)total / (double)g.bins_used;
    g.region = (uint32_t)(avg + 6.0 * sqrt(avg) + 64.0);
    g.table_slots = 256;
    while ((uint64_t)g.table_slots * 3 / 4 < g.region) g.table_slots <<= 1;
    return g.table_slots <= kMergeMaxSlots;
}

// dynamic LDS of the scatter pass ([nbins] counts | [nbins] bases) and of the bin pass ([slots] keys | [slots] u32 counts |
// [kMergeMaxQual] keys | [kMergeMaxQual] u32 counts)
MHX_HD size_t merge_scatter_lds_bytes(uint32_t nbins) { return 2 * (size_t)nbins * sizeof(uint32_t); }
MHX_HD size_t merge_bin_lds_bytes(uint32_t table_slots) { return (size_t)table_slots * 12 + (size_t)kMergeMaxQual * 12; }

// ---- per element -----------------------------------------------------------------------------------------------------
// a slab entry is evidence of the union: above T_min a shard's list is incomplete, and 2^64-1 marks a vacant slot
MHX_HD bool merge_takes(uint64_t h, uint64_t t_min) { return h <= t_min && h != kEmptyKey; }
MHX_HD uint32_t merge_bin(uint64_t h, uint32_t shift) { return (uint32_t)(h >> shift); }
// LDS table of one bin: the bits below the bin index tell the entries of one bin apart
MHX_HD uint32_t merge_home_slot(uint64_t h, uint32_t mask) { return (uint32_t)((h * 0x9E3779B97F4A7C15ull) >> 40) & mask; }
MHX_HD uint32_t merge_next_slot(uint32_t sl, uint32_t mask) { return (sl + 1) & mask; }
// the bin pass's guard: at most 3/4 of the table is ever filled
MHX_HD bool merge_table_guard(uint32_t n, uint32_t table_slots) { return n > (table_slots * 3u) / 4u; }

// one entry of a bin into the bin's LDS table: the key claimed by CAS (or found), the count added.  Returns true when the
// 32-bit sum wrapped (every add sees the true sum before it, so a wrap never goes unseen): kMergeFlagWrap.
MHX_HD bool merge_lds_insert(unsigned long long *keys, uint32_t *cnts, uint32_t mask, uint64_t h, uint32_t c)
{
    uint32_t sl = merge_home_slot(h, mask);
    for (;;) {
        unsigned long long cur = keys[sl];
        if (cur == kEmptyKey) cur = merge_atomic_cas(&keys[sl], (unsigned long long)kEmptyKey, (unsigned long long)h);
        if (cur == kEmptyKey || cur == h) {
            const uint32_t old = merge_atomic_add(&cnts[sl], c);
            return old + c < old;
        }
        sl = merge_next_slot(sl, mask);
    }
}

MHX_HD bool merge_qualifies(uint64_t key, uint32_t cnt, uint32_t min_mult) { return key != kEmptyKey && cnt >= min_mult; }

// qualifier t of the q in (qk, qc) goes to its rank among them -- the keys of a table are distinct -- at the head of the
// bin's region, if the region has such a place
MHX_HD void merge_rank_write(const unsigned long long *qk, const uint32_t *qc, uint32_t q, uint32_t t, uint32_t region, uint64_t *ok, uint32_t *oc)
{
    const unsigned long long mine = qk[t];
    uint32_t rank = 0;
    for (uint32_t j = 0; j < q; ++j) rank += qk[j] < mine ? 1u : 0u;
    if (rank < region) { ok[rank] = mine; oc[rank] = qc[t]; }
}

// compaction: s_off[0 .. 256] are the output offsets of a workgroup's 256 bins (s_off[256]: the end of the last).  The
// bin of output entry e (s_off[0] <= e < s_off[256]) is the LAST i with s_off[i] <= e -- empty bins share an offset with
// their successor --; returns the entry's place in the scatter arrays.
MHX_HD uint64_t merge_source(const uint32_t *s_off, uint32_t e, uint32_t first, uint32_t region)
{
    uint32_t x = 0, y = 256;
    while (y - x > 1) {
        const uint32_t mid = (x + y) >> 1;
        if (s_off[mid] <= e) x = mid; else y = mid;
    }
    return (uint64_t)(first + x) * region + (e - s_off[x]);
}

// ---- the table path: one foreign entry into the sketcher's candidate table --------------------------------------------
// slab_insert_kernel takes kMaxMergeRanks slabs per launch, the ranks r0 .. r0 + launch_ranks - 1 of the call: the index,
// within that launch, of the slab to pass over (this rank's own, already in the table); kMaxMergeRanks: none of them
MHX_HD uint32_t merge_launch_ranks(uint32_t n_ranks, uint32_t r0) { return n_ranks - r0 < kMaxMergeRanks ? n_ranks - r0 : kMaxMergeRanks; }
MHX_HD uint32_t merge_launch_own(uint32_t own_rank, uint32_t r0, uint32_t launch_ranks)
{
    return own_rank >= r0 && own_rank - r0 < launch_ranks ? own_rank - r0 : kMaxMergeRanks;
}

constexpr int kSlabInsertProbes = 8192;
// false: no slot within the probe limit (kFlagTableFull).  The count is added with a clamp at 2^32-1, the host rule's
// (mhx_merge_partials): a clamped sum does not depend on the order of the adds.
MHX_HD bool merge_table_insert(unsigned long long *keys, uint32_t *cnts, uint64_t slot_mask, uint64_t h, uint32_t c)
{
    uint64_t slot = h & slot_mask;
    for (int probe = 0; probe < kSlabInsertProbes; ++probe) {
        // a slot only ever goes from vacant to a key: a plain load that shows this hash (or another one) is final,
        // one that shows a vacant slot is settled by the CAS
        unsigned long long cur = keys[slot];
        if (cur == kEmptyKey) cur = merge_atomic_cas(&keys[slot], (unsigned long long)kEmptyKey, (unsigned long long)h);
        if (cur == kEmptyKey || cur == h) {
            uint32_t old = cnts[slot];
            for (;;) {
                const uint32_t sum = old + c < old ? 0xFFFFFFFFu : old + c;
                const uint32_t seen = merge_atomic_cas(&cnts[slot], old, sum);
                if (seen == old) break;
                old = seen;
            }
            return true;
        }
        slot = (slot + 1) & slot_mask;
    }
    return false;
}

} // namespace mhx
