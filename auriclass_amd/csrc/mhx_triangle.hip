// mhx_triangle.hip -- all pairs within ONE sketch set on the device (`mash triangle`): the finish pass for fewer than 1024
// value ranges, and the two passes that take a block's results out of its block-local arrays -- into the packed lower
// triangle (dense mode) or, filtered, into an edge list (edge mode).  The range pass and the finish passes for 1024
// ranges and more are those of mhx_dist.hip (launch_dist_offsets / _range_pass / _finish); the rules are the host+device
// functions of mhx_triangle.h.
#include "mhx_device.h"
#include "mhx_triangle.h"

namespace mhx {

// 16 pairs per workgroup, the layout of dist_finish_kernel: thread (seg, pair) sums its R / 16 ranges, then the 16
// threads of segment 0 walk the segment totals, the cut segment's ranges and the cut range (tri_finish_walk).
__global__ __launch_bounds__(256) void tri_finish_small_kernel(const DistArgs a, DistWork w)
{
    __shared__ uint32_t seg_uni[kDistSegs][16], seg_com[kDistSegs][16];
    if (w.params[1] != 0) return; // the range pass gave this block up: the generic kernel redoes it (see dist_finish_kernel)
    const uint32_t R = w.ranges, rps = R / kDistSegs, per = R + 1;
    const uint32_t pl = threadIdx.x & 15, seg = threadIdx.x >> 4;
    const uint32_t pair = blockIdx.x * 16 + pl;
    const bool live = pair < a.nq * a.nr;
    const uint32_t q = live ? pair / a.nr : 0, r = live ? pair % a.nr : 0;
    const uint32_t cstride = 4 * ((a.nr + 3) / 4);
    const DistPair x{w.cpart + (uint64_t)q * R * cstride + r, cstride, w.offs_q + q * per, w.offs_r + r * per,
                     a.r + (uint64_t)r * a.stride, a.q + (uint64_t)q * a.stride, a.s};
    tri_segment_total(x, seg, rps, seg_uni[seg][pl], seg_com[seg][pl]);
    __syncthreads();
    if (seg != 0 || !live) return;
    uint32_t common, denom;
    tri_finish_walk(x, &seg_uni[0][pl], &seg_com[0][pl], 16, rps, common, denom);
    const uint64_t out = (uint64_t)q * a.out_stride + a.out_off + r;
    a.common[out] = common;
    a.denom[out] = denom;
}

hipError_t launch_tri_finish_small(const DistArgs &a, const DistWork &w, hipStream_t st)
{
    const uint32_t pairs = a.nq * a.nr;
    if (pairs == 0) return hipSuccess;
    hipLaunchKernelGGL(tri_finish_small_kernel, dim3((pairs + 15) / 16), dim3(256), 0, st, a, w);
    return hipGetLastError();
}

// dense mode: one thread per (query, reference) cell of the block-local arrays, the reference fastest; the pairs that
// count go to their place in the packed triangle (row q of it is contiguous in r)
__global__ __launch_bounds__(256) void tri_scatter_kernel(const TriOut o)
{
    if (*o.flag != 0) return;
    const uint32_t id = blockIdx.x * 256 + threadIdx.x;
    const uint32_t ql = id / kTriSlice, rl = id % kTriSlice;
    const TriBlock b{o.r0, o.nr, o.q0, o.nq};
    if (!tri_pair_counts(b, ql, rl)) return;
    const uint32_t common = o.loc_common[id], denom = o.loc_denom[id];
    const uint64_t at = tri_index(o.q0 + ql, o.r0 + rl);
    o.common[at] = common;
    o.denom[at] = denom;
    if (o.dist) o.dist[at] = tri_distance(common, denom, o.k);
}

// edge mode: the same cells; a pair that counts and passes the prefilter is appended to the edge list.  A wave takes its
// places with ONE atomic (ballot, the first active lane adds the number of keepers, every keeper's place is the base
// plus the keepers below it); beyond cap the pairs are only counted.
__global__ __launch_bounds__(256) void tri_edges_kernel(const TriOut o)
{
    if (*o.flag != 0) return;
    const uint32_t id = blockIdx.x * 256 + threadIdx.x;
    const uint32_t ql = id / kTriSlice, rl = id % kTriSlice;
    const TriBlock b{o.r0, o.nr, o.q0, o.nq};
    uint32_t common = 0, denom = 0;
    bool keep = tri_pair_counts(b, ql, rl);
    if (keep) {
        common = o.loc_common[id];
        denom = o.loc_denom[id];
        keep = tri_keep(common, denom, o.jmin);
    }
    const unsigned long long votes = __ballot(keep);
    if (votes == 0) return;
    const uint32_t lane = threadIdx.x & 63u;
    const int leader = __ffsll((long long)votes) - 1;
    unsigned long long base = 0;
    if ((int)lane == leader) base = atomicAdd(o.count, (unsigned long long)__popcll(votes));
    base = __shfl(base, leader);
    if (!keep) return;
    const unsigned long long at = base + (unsigned long long)__popcll(votes & ((1ull << lane) - 1ull));
    if (at >= o.cap) return;
    o.edge_i[at] = o.q0 + ql;
    o.edge_j[at] = o.r0 + rl;
    o.common[at] = common;
    o.denom[at] = denom;
    if (o.dist) o.dist[at] = tri_distance(common, denom, o.k);
}

hipError_t launch_tri_scatter(const TriOut &o, hipStream_t st)
{
    if (o.nq == 0) return hipSuccess;
    hipLaunchKernelGGL(tri_scatter_kernel, dim3((o.nq * kTriSlice + 255) / 256), dim3(256), 0, st, o);
    return hipGetLastError();
}

hipError_t launch_tri_edges(const TriOut &o, hipStream_t st)
{
    if (o.nq == 0) return hipSuccess;
    hipLaunchKernelGGL(tri_edges_kernel, dim3((o.nq * kTriSlice + 255) / 256), dim3(256), 0, st, o);
    return hipGetLastError();
}

} // namespace mhx
