// mhx_search.h -- the rules of the reference-set search (for every query the `top` closest references within a distance
// bound) that do not depend on how a GPU runs them, as host+device functions: the exact order of two pairs by their
// Jaccard index, the insertion that keeps a query's best list sorted, and the schedule of (query batch, reference slice)
// blocks.  The take-out kernel of mhx_search.hip does wave-wide what search_insert does one candidate after the other;
// tests/emul/search_emul.cpp runs these functions sequentially on the CPU.  Geometry, prefilter and distance are those of
// the triangle (mhx_triangle.h: tri_ranges, tri_keep, tri_jmin, tri_distance), the passes those of mhx_dist.h.
#pragma once
#include "mhx_triangle.h"

namespace mhx {

constexpr uint32_t kSearchMaxTop = 64; // one entry per lane of a wave64

struct SearchHit { uint32_t ref, common, denom; };

// ---- the order ----------------------------------------------------------------------------------------------------------
// a is better than b: the larger Jaccard index common / denom, compared exactly as a cross product in 64 bits (both factors
// are below 2^32); common == denom counts as 1/1, which gives 0/0 -- two empty lists, distance 0 in Mash -- its place at the
// top; equal indices (1/2 and 2/4) go by the lower reference.  References are distinct, so this is a total order and a best
// list does not depend on the order in which its candidates arrive.
MHX_HD bool search_better(const SearchHit &a, const SearchHit &b)
{
    const uint64_t ac = a.common == a.denom ? 1u : a.common, ad = a.common == a.denom ? 1u : a.denom;
    const uint64_t bc = b.common == b.denom ? 1u : b.common, bd = b.common == b.denom ? 1u : b.denom;
    const uint64_t l = ac * bd, r = bc * ad;
    return l != r ? l > r : a.ref < b.ref;
}

// list[0 .. n) is sorted best first and holds at most `top` entries: put `cand` in its place, drop the last entry when the
// list is full; returns the new n.  A full list costs a candidate that is not better than its last entry one comparison.
MHX_HD uint32_t search_insert(SearchHit *list, uint32_t n, uint32_t top, const SearchHit &cand)
{
    if (n == top && !search_better(cand, list[top - 1])) return n;
    uint32_t pos = 0;
    while (pos < n && search_better(list[pos], cand)) ++pos;
    const uint32_t last = n < top ? n : top - 1;
    for (uint32_t i = last; i > pos; --i) list[i] = list[i - 1];
    list[pos] = cand;
    return n < top ? n + 1 : top;
}

// ---- schedule -----------------------------------------------------------------------------------------------------------
// The references go through in slices of kTriSlice (32) lists, the queries in batches of at most `qbatch`: block b of
// ceil(nq / qbatch) * ceil(nr / 32), the slices of one batch one after the other.  64-bit: nq * nr is not limited.
struct SearchBlock { uint32_t r0, nr, q0, nq; };
MHX_HD uint64_t search_blocks(uint32_t nq, uint32_t nr, uint32_t qbatch)
{
    return (uint64_t)((nq + (uint64_t)qbatch - 1) / qbatch) * ((nr + (uint64_t)kTriSlice - 1) / kTriSlice);
}
MHX_HD SearchBlock search_block(uint32_t nq, uint32_t nr, uint32_t qbatch, uint64_t b)
{
    const uint64_t nslices = (nr + (uint64_t)kTriSlice - 1) / kTriSlice;
    SearchBlock x;
    x.q0 = (uint32_t)(b / nslices) * qbatch;
    x.r0 = (uint32_t)(b % nslices) * kTriSlice;
    x.nq = nq - x.q0 < qbatch ? nq - x.q0 : qbatch;
    x.nr = nr - x.r0 < kTriSlice ? nr - x.r0 : kTriSlice;
    return x;
}

} // namespace mhx
