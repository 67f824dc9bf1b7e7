// mhx_linkage.hip -- complete- and average-linkage agglomeration of ONE sketch set on the device (mhx_dist_linkage): the init
// pass over the packed triangle of the dense mode and the three launches of a step -- pick, update, rescan -- over one 64-bit
// word per cluster pair, size [n] and the cached nearest partner nn [n].  The rules are the host+device functions of
// mhx_linkage.h.  Every hand-off between workgroups crosses a kernel boundary: within a launch no work item reads a word
// that another one writes (see link_update), so plain loads and stores do; the one atomic is the counter of the work list,
// which carries no value of the result.
#include "mhx_device.h"
#include "mhx_linkage.h"

namespace mhx {

namespace {

constexpr uint32_t kLinkPickThreads = 1024; // one workgroup of 16 waves reduces the rows
constexpr uint32_t kLinkScanBlocks = 1024;  // workgroups of the rescan, each takes list entries blockIdx.x, + gridDim.x, ...

__device__ __forceinline__ LinkState link_state(const LinkArgs &a) { return LinkState{a.words, a.size, a.nn, a.n, a.linkage}; }

// the first candidate, in the candidate order, among the 64 lanes of a wave; every lane calls this
__device__ __forceinline__ LinkCand link_wave_best(int linkage, LinkCand c)
{
    for (int off = 32; off > 0; off >>= 1) {
        LinkCand o;
        o.w = (uint64_t)__shfl_xor((unsigned long long)c.w, off, 64);
        o.den = (uint64_t)__shfl_xor((unsigned long long)c.den, off, 64);
        o.lo = (uint32_t)__shfl_xor((int)c.lo, off, 64);
        o.hi = (uint32_t)__shfl_xor((int)c.hi, off, 64);
        c = link_cand_better(linkage, c, o);
    }
    return c;
}
// ... among the WAVES waves of a workgroup; every thread calls this, the result is valid in wave 0.  lds: WAVES entries,
// free for the next call once the caller has passed a barrier
template <uint32_t WAVES> __device__ __forceinline__ LinkCand link_block_best(int linkage, LinkCand c, LinkCand *lds)
{
    static_assert(WAVES <= 64, "one wave reduces the waves' results");
    c = link_wave_best(linkage, c);
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (lane == 0) lds[wave] = c;
    __syncthreads();
    if (wave == 0) c = link_wave_best(linkage, lane < WAVES ? lds[lane] : link_no_cand());
    return c;
}

} // namespace

// the words of all pairs from the triangle's common / denom (the same packed index); every list a cluster of one, every
// row but row 0 on the work list: the first rescan gives nn
__global__ __launch_bounds__(256) void link_init_kernel(const LinkArgs a, const uint32_t *common, const uint32_t *denom, uint64_t pairs)
{
    const uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (p < pairs) a.words[p] = link_init_word(a.linkage, common[p], denom[p], a.k);
    if (p < a.n) {
        a.size[p] = 1;
        a.nn[p] = kLinkNone;
        if (p) a.list[p - 1] = (uint32_t)p;
    }
    if (p == 0) {
        a.ctl[0] = a.ctl[1] = kLinkNone; a.ctl[2] = a.ctl[3] = 0;
        a.ctl[4] = a.n - 1;
        a.ctl[5] = 0;
        *a.total = 0;
    }
}

// step t, pick: ONE workgroup reduces the active rows by (V(i, nn[i]), nn[i], i), writes merge record t and the pair with
// its sizes for the update, and takes the work list of the step before off the books
__global__ __launch_bounds__(kLinkPickThreads) void link_pick_kernel(const LinkArgs a, uint32_t t)
{
    __shared__ LinkCand lds[kLinkPickThreads / 64];
    const LinkState s = link_state(a);
    LinkCand mine = link_no_cand();
    for (uint32_t i = threadIdx.x; i < a.n; i += kLinkPickThreads) mine = link_cand_better(a.linkage, mine, link_row_candidate(s, i));
    mine = link_block_best<kLinkPickThreads / 64>(a.linkage, mine, lds);
    if (threadIdx.x != 0) return;
    if (t != 0) *a.total += a.ctl[4]; // (the scans of the init pass are not rescans)
    a.ctl[4] = 0;
    if (mine.hi >= a.n || mine.lo >= mine.hi) { // no pair although clusters are left: the update does nothing, the host reports it
        a.ctl[0] = a.ctl[1] = kLinkNone;
        a.ctl[5] = 1;
        return;
    }
    const uint32_t sa = a.size[mine.hi], sb = a.size[mine.lo];
    a.ctl[0] = mine.hi; a.ctl[1] = mine.lo; a.ctl[2] = sa; a.ctl[3] = sb;
    uint64_t num, den;
    link_record(a.linkage, mine, num, den);
    a.merge_a[t] = mine.hi; a.merge_b[t] = mine.lo; a.size_out[t] = sa + sb;
    a.num[t] = num; a.den[t] = den;
    if (a.dist) a.dist[t] = link_height(a.linkage, num, den, a.k);
}

// step t, update: one thread per cluster c (link_update); the rows to scan again go to the work list
__global__ __launch_bounds__(256) void link_update_kernel(const LinkArgs a)
{
    const uint32_t c = blockIdx.x * 256 + threadIdx.x;
    const LinkPick p{a.ctl[0], a.ctl[1], a.ctl[2], a.ctl[3]};
    if (c >= a.n || p.a >= a.n || p.b >= p.a) return;
    if (!link_update(link_state(a), p, c)) return;
    const uint32_t at = atomicAdd(a.ctl + 4, 1u);
    if (at < a.n) a.list[at] = c;
}

// step t, rescan: a workgroup per row of the work list; its threads stride over the partners j < i, the first candidate in
// the candidate order is the row's new nn
__global__ __launch_bounds__(256) void link_rescan_kernel(const LinkArgs a)
{
    __shared__ LinkCand lds[4];
    const LinkState s = link_state(a);
    const uint32_t count = a.ctl[4] < a.n ? a.ctl[4] : a.n;
    for (uint32_t w = blockIdx.x; w < count; w += gridDim.x) {
        const uint32_t i = a.list[w];
        if (i >= a.n) continue; // (uniform in the workgroup)
        LinkCand mine = link_no_cand();
        for (uint32_t j = threadIdx.x; j < i; j += 256) mine = link_cand_better(a.linkage, mine, link_scan_candidate(s, i, j));
        mine = link_block_best<4>(a.linkage, mine, lds);
        if (threadIdx.x == 0) a.nn[i] = mine.hi == kLinkNone ? kLinkNone : mine.lo;
        __syncthreads();
    }
}

hipError_t launch_link_init(const LinkArgs &a, const uint32_t *common, const uint32_t *denom, hipStream_t st)
{
    const uint64_t pairs = (uint64_t)a.n * (a.n - 1) / 2, items = pairs > a.n ? pairs : a.n;
    hipLaunchKernelGGL(link_init_kernel, dim3((uint32_t)((items + 255) / 256)), dim3(256), 0, st, a, common, denom, pairs);
    return hipGetLastError();
}
hipError_t launch_link_pick(const LinkArgs &a, uint32_t t, hipStream_t st)
{
    hipLaunchKernelGGL(link_pick_kernel, dim3(1), dim3(kLinkPickThreads), 0, st, a, t);
    return hipGetLastError();
}
hipError_t launch_link_update(const LinkArgs &a, hipStream_t st)
{
    hipLaunchKernelGGL(link_update_kernel, dim3((a.n + 255) / 256), dim3(256), 0, st, a);
    return hipGetLastError();
}
hipError_t launch_link_rescan(const LinkArgs &a, hipStream_t st)
{
    hipLaunchKernelGGL(link_rescan_kernel, dim3(a.n < kLinkScanBlocks ? a.n : kLinkScanBlocks), dim3(256), 0, st, a);
    return hipGetLastError();
}

} // namespace mhx
