// mhx_contain_within.h -- the rules of the unbounded containment call (mhx_dist_contain_within: for every query ALL references
// it holds, as CSR) that do not depend on how a GPU runs them, as host+device functions.  Nearly all of them exist already:
// the hit test is the containment search's (mhx_contain_search.h: contain_need_build on the host, contain_keep on the device),
// the super-batches, the cell record of one (query, slice), the scan into row_off and the address a hit is gathered to are
// the bounded neighbourhood call's (mhx_within.h: within_super_queries, within_cell, within_cell_record, within_rank,
// within_row_count, within_dest).  What is added here is the ballot of the one over a block's slice, which is a cell's mask.
// The kernels of mhx_contain_within.hip do wave- and workgroup-wide what these functions do one cell after the other;
// tests/emul/contain_within_emul.cpp runs them sequentially on the CPU, blocks and arrivals in any order.
#pragma once
#include "mhx_contain_search.h"
#include "mhx_within.h"

namespace mhx {

// The mask of one (query, slice): bit rl says that reference r0 + rl of the block is a hit of the query.  loc_shared and
// loc_n_ref are the query's 32 block-local counts, of which the first nr are written.  A cell's keepers go to the arrival
// list as (shared, n_ref, n_qry), in reference order from the cell's start on (within_rank).
MHX_HD uint32_t contain_within_ballot(const uint32_t *loc_shared, const uint32_t *loc_n_ref, uint32_t nr, const uint32_t *need, uint32_t need_limit)
{
    uint32_t word = 0;
    for (uint32_t rl = 0; rl < nr && rl < kTriSlice; ++rl)
        if (contain_keep(loc_shared[rl], loc_n_ref[rl], need, need_limit)) word |= 1u << rl;
    return word;
}

} // namespace mhx
