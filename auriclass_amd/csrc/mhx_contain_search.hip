// mhx_contain_search.hip -- containment search on the device (mhx_dist_contain_search): the pass that takes a block's up to 32
// candidates per query out of its block-local arrays and merges them into that query's running best list.  The bounds, the
// finish pass and the pair kernel are those of mhx_contain.hip, writing block-local; the range pass is that of mhx_dist.hip;
// the rules are the host+device functions of mhx_contain_search.h.
#include "mhx_device.h"
#include "mhx_contain_search.h"

namespace mhx {

__device__ __forceinline__ ContainHit wave_read(const ContainHit &h, int lane)
{
    return ContainHit{(uint32_t)__shfl((int)h.ref, lane), (uint32_t)__shfl((int)h.shared, lane), (uint32_t)__shfl((int)h.n_ref, lane),
                      (uint32_t)__shfl((int)h.n_qry, lane)};
}

// One wave64 per query, no atomics: lane i holds entry i of the query's best list (top <= 64), lanes 0 .. 31 load the
// block's candidates (three coalesced reads), a ballot of the hit test selects the ones to insert.  For every set bit --
// the loop is wave-uniform: the ballot, n and the worst entry are the same in all lanes -- the candidate is broadcast, its
// place is the number of entries that are better (popcount of a ballot), the lanes behind it take their left neighbour's
// entry, the lane at it takes the candidate and the last entry falls off.  This is contain_insert, entry for entry: the order is total, so there is
// exactly one place, and blocks may arrive in any order.
__global__ __launch_bounds__(256) void contain_take_kernel(const ContainSearchOut o)
{
    if (*o.flag != 0) return; // the range pass gave this block up: the pair kernel redoes it, its take-out runs then
    const uint32_t lane = threadIdx.x & 63u, ql = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (ql >= o.nq) return;
    const uint64_t q = (uint64_t)o.q0 + ql, at = q * o.top + lane;
    uint32_t n = o.n_hits[q];
    ContainHit mine{0, 0, 0, 0};
    if (lane < n) mine = ContainHit{o.hit_ref[at], o.hit_shared[at], o.hit_n_ref[at], o.hit_n_qry[at]};
    ContainHit cand{o.r0 + lane, 0, 0, 0};
    bool keep = false;
    if (lane < o.nr) {
        cand.shared = o.loc_shared[ql * kTriSlice + lane];
        cand.n_ref = o.loc_n_ref[ql * kTriSlice + lane];
        cand.n_qry = o.loc_n_qry[ql * kTriSlice + lane];
        keep = contain_keep(cand.shared, cand.n_ref, o.need, o.need_limit);
    }
    unsigned long long votes = __ballot(keep);
    if (votes == 0) return;
    while (votes) {
        const int b = __ffsll((long long)votes) - 1;
        votes &= votes - 1;
        const ContainHit c = wave_read(cand, b);
        if (n == o.top && !contain_better(c, wave_read(mine, (int)o.top - 1))) continue;
        const uint32_t pos = (uint32_t)__popcll(__ballot(lane < n && contain_better(mine, c)));
        const ContainHit left{(uint32_t)__shfl_up((int)mine.ref, 1), (uint32_t)__shfl_up((int)mine.shared, 1), (uint32_t)__shfl_up((int)mine.n_ref, 1),
                              (uint32_t)__shfl_up((int)mine.n_qry, 1)};
        if (lane > pos) mine = left;
        else if (lane == pos) mine = c;
        if (n < o.top) ++n;
    }
    if (lane < n) {
        o.hit_ref[at] = mine.ref;
        o.hit_shared[at] = mine.shared;
        o.hit_n_ref[at] = mine.n_ref;
        o.hit_n_qry[at] = mine.n_qry;
    }
    if (lane == 0) o.n_hits[q] = n;
}

hipError_t launch_contain_take(const ContainSearchOut &o, hipStream_t st)
{
    if (o.nq == 0) return hipSuccess;
    hipLaunchKernelGGL(contain_take_kernel, dim3((o.nq + 3) / 4), dim3(256), 0, st, o);
    return hipGetLastError();
}

} // namespace mhx
