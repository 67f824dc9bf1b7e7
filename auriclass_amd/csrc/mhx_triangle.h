// mhx_triangle.h -- the rules of the all-pairs distance within ONE sketch set (`mash triangle`) that do not depend on how a
// GPU runs them, as host+device functions: the packed index of a pair, the geometry rule (value ranges from the longest
// list), the schedule (slices of 32 references, query batches, which pairs of a block count), the finish walk for fewer
// than 1024 ranges and the prefilter of the edge mode.  The kernels in mhx_triangle.hip call these functions;
// tests/emul/triangle_emul.cpp runs the same functions sequentially on the CPU.  The range pass itself, the range table
// and the scan functions of the walk are those of mhx_dist.h.
#pragma once
#include <math.h>
#include "mhx_dist.h"

namespace mhx {

// ---- packed lower triangle ----------------------------------------------------------------------------------------------
// pair (i, j), j < i, of n lists: rows in Mash's print order (row i holds j = 0 .. i - 1)
MHX_HD uint64_t tri_index(uint32_t i, uint32_t j) { return (uint64_t)i * (i - 1u) / 2u + j; }
constexpr uint32_t kTriMaxLists = 65536; // n (n - 1) / 2 <= 2^31 - 1 pairs up to here

// ---- geometry -----------------------------------------------------------------------------------------------------------
// The smallest power of two R with longest <= kTriSliceTarget * R, clamped to [kTriMinRanges, kTriMaxRanges]; from the
// LENGTH of the longest list alone, like dist_windows.  16 entries per (list, range) slice, not 64: the "references" of a
// triangle are usually independent genomes, so the 32 lists of a slice put 32 x 16 different keys into a range's table,
// 1024 with the rounding of the scale (half of the ranges in use), below kDistTableLimit.  s = 1000 -> 64 ranges,
// 8193 .. 16 384 hashes -> 1024, 20 000 -> 2048, from 262 145 on 16 384 (slices grow again and the overflow flag takes
// over); lists of more than 2^20 hashes have no geometry (0) and go to the generic pair kernel.
constexpr uint32_t kTriSliceTarget = 16;
constexpr uint32_t kTriMinRanges = 16, kTriMaxRanges = 16384;
constexpr uint64_t kTriLongest = 1ull << 20;
static_assert(32u * 2u * kTriSliceTarget < kDistTableLimit, "a slice of independent lists fits a range's table");

MHX_HD uint32_t tri_ranges(uint64_t longest)
{
    if (longest > kTriLongest) return 0;
    uint32_t R = kTriMinRanges;
    while (R < kTriMaxRanges && longest > (uint64_t)kTriSliceTarget * R) R <<= 1;
    return R;
}
// the geometry of mhx_dist_batch for the same lists (MHX_TRI_GEOMETRY=dist): never fewer than 1024 ranges
MHX_HD uint32_t tri_ranges_dist(uint64_t longest) { return (uint32_t)kDistRanges * dist_windows(longest); }

// ---- schedule -----------------------------------------------------------------------------------------------------------
// The set is cut into slices of 32 consecutive lists, the "references" of a block (one bit each in the range table's
// masks); the queries of the slice that begins at r0 are the lists r0 + 1 .. n - 1, in batches of at most `qbatch`.  A pair
// (q, r) of a block counts when r < q: the few others inside a slice's own lists are computed and thrown away.
constexpr uint32_t kTriSlice = 32;
struct TriBlock { uint32_t r0, nr, q0, nq; };

// the block at or behind (slice r0, query q0), false when there is none
MHX_HD bool tri_block_at(uint32_t n, uint32_t qbatch, uint32_t r0, uint32_t q0, TriBlock &b)
{
    for (; r0 < n; r0 += kTriSlice, q0 = 0) {
        if (q0 < r0 + 1u) q0 = r0 + 1u;
        if (q0 >= n) continue;
        b.r0 = r0; b.nr = n - r0 < kTriSlice ? n - r0 : kTriSlice;
        b.q0 = q0; b.nq = n - q0 < qbatch ? n - q0 : qbatch;
        return true;
    }
    return false;
}
MHX_HD bool tri_first_block(uint32_t n, uint32_t qbatch, TriBlock &b) { return tri_block_at(n, qbatch, 0, 0, b); }
MHX_HD bool tri_next_block(uint32_t n, uint32_t qbatch, TriBlock &b) { return tri_block_at(n, qbatch, b.r0, b.q0 + b.nq, b); }
// pair (query ql, reference rl) of block b, both counted from the block's first
MHX_HD bool tri_pair_counts(const TriBlock &b, uint32_t ql, uint32_t rl) { return rl < b.nr && ql < b.nq && b.r0 + rl < b.q0 + ql; }

// Queries per block: the byte counters [q][R][32], the window totals of the windowed finish (R >= 2048) and the block-local
// results [q][32] x 2 stay below kDistWideWorkLimit, which also keeps every q * (R + 1) index of the kernels below 2^32.
// The offsets of the whole set, [n][R + 1], are not part of a block: they are written once per call.
MHX_HD uint32_t tri_max_queries(uint32_t ranges)
{
    uint64_t per_query = (uint64_t)ranges * kTriSlice + 2ull * 4 * kTriSlice;
    if (ranges > (uint32_t)kDistRanges) per_query += (uint64_t)(ranges / kDistWindowRanges) * kTriSlice * 4;
    const uint64_t n = (kDistWideWorkLimit - 4 * 256) / per_query;
    return n < 1 ? 1u : (n > kTriMaxLists ? kTriMaxLists : (uint32_t)n);
}

// ---- short-range finish walk (R < 1024) -----------------------------------------------------------------------------------
// dist_finish_kernel has 1024 ranges at compile time and dist_finish_wide_kernel groups of 1024: with fewer ranges the 16
// threads of a pair each sum a segment of rps = R / 16 ranges (>= 1), then one thread walks the 16 segment totals to the
// cut segment, its ranges to the cut range, and finishes that range with the two-pointer rule.
MHX_HD void tri_segment_total(const DistPair &x, uint32_t seg, uint32_t rps, uint32_t &uni, uint32_t &com)
{
    uint32_t c = 0;
    for (uint32_t p = seg * rps; p < (seg + 1) * rps; ++p) c += x.cp[(uint64_t)p * x.cstride];
    com = c;
    uni = dist_range_union(x, seg * rps, (seg + 1) * rps, c);
}
// seg_uni / seg_com: the kDistSegs totals of this pair, `stride` words apart
MHX_HD void tri_finish_walk(const DistPair &x, const uint32_t *seg_uni, const uint32_t *seg_com, uint32_t stride, uint32_t rps,
                            uint32_t &common, uint32_t &denom)
{
    uint32_t uni = 0;
    common = 0;
    const uint32_t sg = dist_scan_totals(seg_uni, seg_com, stride, 0, kDistSegs, x.S, uni, common);
    if (sg == (uint32_t)kDistSegs) { denom = uni; return; } // union smaller than s: everything counts
    const uint32_t p = dist_scan_ranges(x, sg * rps, (sg + 1) * rps, uni, common); // the cut range is inside this segment
    dist_two_pointer(x, p, uni, common);
    denom = x.S; // this range holds enough further union elements by construction
}

// ---- edge mode ------------------------------------------------------------------------------------------------------------
// The device keeps a pair when its Jaccard index reaches jmin, the index of the distance bound lowered by 2^-30 relative
// (tri_jmin, host): every pair the exact rule keeps -- the libm distance <= max_dist, the double that is printed, whose
// rounding is ~1e-16 -- passes, a few more may, and the host drops those.
MHX_HD bool tri_keep(uint32_t common, uint32_t denom, double jmin) { return common == denom || (double)common >= jmin * (double)denom; }

// host: the Jaccard index below which the device drops a pair (0: max_dist >= 1 keeps everything).  No distance is
// negative, so a bound below 0 is the bound 0 to the prefilter: it keeps the identical pairs (common == denom), which the
// exact rule of the host forms then drops.  (Taken as it is, 2 exp(k max_dist) - 1 falls to 0 and below at max_dist <=
// -ln 2 / k, and the index of the bound with it: the prefilter would keep every pair.)
MHX_HD double tri_jmin(double max_dist, int k)
{
    if (max_dist >= 1.0) return 0.0;
    const double d = max_dist < 0.0 ? 0.0 : max_dist;
    return (1.0 / (2.0 * exp((double)k * d) - 1.0)) * (1.0 - 0x1p-30);
}

// the Mash distance of a pair (the arithmetic of dist_store and of the host forms)
MHX_HD double tri_distance(uint32_t common, uint32_t denom, int k)
{
    if (common == denom) return 0.0;
    if (common == 0) return 1.0;
    const double jac = (double)common / (double)denom;
    const double d = -log(2.0 * jac / (1.0 + jac)) / (double)k;
    return d > 1.0 ? 1.0 : d;
}

} // namespace mhx
