// mhx_search.hip -- reference-set search on the device: the pass that takes a block's up to 32 candidates per query out
// of its block-local arrays and merges them into that query's running best list, and the distances of the finished lists.
// The range pass and the finish passes are those of mhx_dist.hip and mhx_triangle.hip; the rules are the host+device
// functions of mhx_search.h.
#include "mhx_device.h"
#include "mhx_search.h"

namespace mhx {

__device__ __forceinline__ SearchHit wave_read(const SearchHit &h, int lane)
{
    return SearchHit{(uint32_t)__shfl((int)h.ref, lane), (uint32_t)__shfl((int)h.common, lane), (uint32_t)__shfl((int)h.denom, lane)};
}

// One wave64 per query, no atomics: lane i holds entry i of the query's best list (top <= 64), lanes 0 .. 31 load the
// block's candidates (two coalesced reads), a ballot of the prefilter selects the ones to insert.  For every set bit --
// the loop is wave-uniform: the ballot, n and the worst entry are the same in all lanes -- the candidate is broadcast, its
// place is the number of entries that are better (popcount of a ballot), the lanes at or behind it take their left
// neighbour's entry and the last entry falls off.  This is search_insert, entry for entry: the order is total, so there is
// exactly one place, and blocks may arrive in any order.
__global__ __launch_bounds__(256) void search_take_kernel(const SearchOut o)
{
    if (*o.flag != 0) return; // the range pass gave this block up: the generic kernel redoes it, its take-out runs then
    const uint32_t lane = threadIdx.x & 63u, ql = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (ql >= o.nq) return;
    const uint64_t q = (uint64_t)o.q0 + ql, at = q * o.top + lane;
    uint32_t n = o.n_hits[q];
    SearchHit mine{0, 0, 0};
    if (lane < n) mine = SearchHit{o.hit_ref[at], o.hit_common[at], o.hit_denom[at]};
    SearchHit cand{o.r0 + lane, 0, 0};
    bool keep = false;
    if (lane < o.nr) {
        cand.common = o.loc_common[ql * kTriSlice + lane];
        cand.denom = o.loc_denom[ql * kTriSlice + lane];
        keep = tri_keep(cand.common, cand.denom, o.jmin);
    }
    unsigned long long votes = __ballot(keep);
    if (votes == 0) return;
    while (votes) {
        const int b = __ffsll((long long)votes) - 1;
        votes &= votes - 1;
        const SearchHit c = wave_read(cand, b);
        if (n == o.top && !search_better(c, wave_read(mine, (int)o.top - 1))) continue;
        const uint32_t pos = (uint32_t)__popcll(__ballot(lane < n && search_better(mine, c)));
        const SearchHit left{(uint32_t)__shfl_up((int)mine.ref, 1), (uint32_t)__shfl_up((int)mine.common, 1), (uint32_t)__shfl_up((int)mine.denom, 1)};
        if (lane > pos) mine = left;
        else if (lane == pos) mine = c;
        if (n < o.top) ++n;
    }
    if (lane < n) {
        o.hit_ref[at] = mine.ref;
        o.hit_common[at] = mine.common;
        o.hit_denom[at] = mine.denom;
    }
    if (lane == 0) o.n_hits[q] = n;
}

__global__ __launch_bounds__(256) void search_dist_kernel(const SearchOut o)
{
    const uint64_t id = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint64_t ql = id / o.top;
    if (ql >= o.nq) return;
    const uint64_t q = (uint64_t)o.q0 + ql, at = q * o.top + id % o.top;
    if (id % o.top < o.n_hits[q]) o.hit_dist[at] = tri_distance(o.hit_common[at], o.hit_denom[at], o.k);
}

hipError_t launch_search_take(const SearchOut &o, hipStream_t st)
{
    if (o.nq == 0) return hipSuccess;
    hipLaunchKernelGGL(search_take_kernel, dim3((o.nq + 3) / 4), dim3(256), 0, st, o);
    return hipGetLastError();
}

hipError_t launch_search_dist(const SearchOut &o, hipStream_t st)
{
    if (o.nq == 0 || !o.hit_dist) return hipSuccess;
    const uint64_t cells = (uint64_t)o.nq * o.top;
    hipLaunchKernelGGL(search_dist_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, st, o);
    return hipGetLastError();
}

} // namespace mhx
