// mhx_within.h -- the rules of the bounded neighbourhood call (mhx_dist_within: for every query ALL references within a
// distance, as CSR) that do not depend on how a GPU runs them, as host+device functions: the schedule (the search's blocks
// inside super-batches of queries), the cell record of one (query, slice), the per-query scan of the cells into row_off and
// the address a hit is gathered to.  The kernels of mhx_within.hip do wave- and workgroup-wide what these functions do one
// cell after the other; tests/emul/within_emul.cpp runs them sequentially on the CPU, blocks and arrivals in any order.
// The hit test is the clustering's exact integer rule (mhx_cluster.h: cluster_cmin_build on the host, cluster_keep on the
// device), blocks and slices are the search's (mhx_search.h), geometry and distance the triangle's (mhx_triangle.h).
#pragma once
#include "mhx_cluster.h"
#include "mhx_search.h"

namespace mhx {

// ---- schedule -----------------------------------------------------------------------------------------------------------
// A slice of kTriSlice (32) references is exactly one 32-bit word per (query, slice): bit b of a cell's mask says that
// reference 32 * slice + b is a hit of the query.  The cells of a call would be nq * ceil(nr / 32) words twice over (mask and
// base), so the queries go through in super-batches of at most within_super_queries(nr, limit) queries: the cells of one
// super-batch stay at or below `limit` (kWithinCells by default; one query's cells when a single row is longer), and
// everything below -- blocks, fallback, scan, gather -- happens per super-batch.  Inside one the blocks are search_block's.
constexpr uint64_t kWithinCells = 1ull << 22; // cells of a super-batch: 2 x 16 MiB of workspace

MHX_HD uint32_t within_slices(uint32_t nr) { return (uint32_t)((nr + (uint64_t)kTriSlice - 1) / kTriSlice); }
MHX_HD uint32_t within_super_queries(uint32_t nq, uint32_t nr, uint64_t limit)
{
    const uint64_t nslices = within_slices(nr);
    const uint64_t n = nslices ? limit / nslices : nq;
    return n < 1 ? 1u : (n > nq ? nq : (uint32_t)n);
}
// the cell of query `ql` (counted from the super-batch's first) and the slice that begins at reference r0
MHX_HD uint64_t within_cell(uint32_t ql, uint32_t r0, uint32_t nslices) { return (uint64_t)ql * nslices + r0 / kTriSlice; }

// ---- the cell record ------------------------------------------------------------------------------------------------------
// What the take-out pass leaves of one (query, slice): the ballot of cluster_keep over the slice's references, and where its
// keepers -- (common, denom), in reference order -- begin in the arrival list.  `start` is whatever the arrival counter held
// when the cell's wave added its keepers: it depends on the order in which blocks finish and is read by the gather alone.
// Keeper `rank` of the cell lies at start + rank; entries at or beyond `room` are counted and not stored.
MHX_HD uint32_t within_ballot(const uint32_t *loc_common, const uint32_t *loc_denom, uint32_t nr, const uint32_t *cmin, uint32_t s)
{
    uint32_t word = 0;
    for (uint32_t rl = 0; rl < nr && rl < kTriSlice; ++rl)
        if (cluster_keep(loc_common[rl], loc_denom[rl], cmin, s)) word |= 1u << rl;
    return word;
}
MHX_HD uint32_t within_popc(uint32_t v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return (uint32_t)__popc(v);
#else
    return (uint32_t)__builtin_popcount(v);
#endif
}
MHX_HD uint32_t within_rank(uint32_t word, uint32_t rl) { return within_popc(word & ((1u << rl) - 1u)); }
// the rank-th set bit of word (rank < popcount): the reference of a gathered hit, counted from its slice's first
MHX_HD uint32_t within_nth_bit(uint32_t word, uint32_t rank)
{
    for (uint32_t i = 0; i < rank; ++i) word &= word - 1u;
    uint32_t b = 0;
    while (!((word >> b) & 1u)) ++b;
    return b;
}
MHX_HD void within_cell_record(uint32_t *mask, uint32_t *base, uint64_t cell, uint32_t word, uint32_t start)
{
    mask[cell] = word;
    if (base) base[cell] = start; // (the counting form keeps no arrival list and no base)
}

// ---- the per-query scan -----------------------------------------------------------------------------------------------------
// hits of a query = the set bits of its row of cells; row_off of the call is the running sum over the queries in index order,
// row_off[0] = 0.  Neither depends on `base`, so arrival order never shows in it.
MHX_HD uint64_t within_row_count(const uint32_t *mask_row, uint32_t nslices)
{
    uint64_t n = 0;
    for (uint32_t i = 0; i < nslices; ++i) n += within_popc(mask_row[i]);
    return n;
}

// ---- the gather address -------------------------------------------------------------------------------------------------------
// Hit `rank` of the cell (query q, slice sl) goes to row_off[q] + (set bits of the query's cells before sl) + rank: the hits
// of a query ascend by reference whatever order they arrived in.  `before` is that middle term.
MHX_HD uint64_t within_dest(uint64_t row_start, uint64_t before, uint32_t rank) { return row_start + before + rank; }

} // namespace mhx
