// mhx_mst.hip -- the single-linkage tree of ONE sketch set on the device (mhx_dist_mst): the passes of a Boruvka round over
// best[n] / winner[n] / parent[n] -- reset, propose (from the packed triangle, mst_scan_kernel, or as a fourth take-out pass
// of the triangle's blocks, tri_mst_kernel), choose and hook.  The flatten pass between rounds is mhx_cluster.hip's.  The
// rules are the host+device functions of mhx_mst.h; every access to a word that others write in the same launch goes
// through the agent-scope atomics of its access layer, what a launch only reads was written by an earlier launch.
#include "mhx_device.h"
#include "mhx_mst.h"

namespace mhx {

// step 1: nobody has proposed
__global__ __launch_bounds__(256) void mst_reset_kernel(uint64_t *best, uint32_t *winner, uint32_t n)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    best[i] = 0;
    winner[i] = kMstNobody;
}

// the best word among the `width` (32 or 64) consecutive lanes that share a vertex; every lane of the wave calls this
__device__ __forceinline__ uint64_t mst_lanes_best(uint64_t w, int width)
{
    for (int off = width / 2; off > 0; off >>= 1) {
        const uint64_t other = (uint64_t)__shfl_xor((unsigned long long)w, off, width);
        w = mst_word_better(w, other);
    }
    return w;
}

// step 2, recomputed source: the cells of tri_scatter_kernel, tri_edges_kernel and tri_cluster_kernel, the same mapping and
// the same early return.  The 32 lanes of a cell row share the query i: they reduce their proposals among themselves and
// one lane proposes to best[i]; every lane whose pair is live proposes to best[j] of its own reference.
__global__ __launch_bounds__(256) void tri_mst_kernel(const MstOut o)
{
    if (*o.flag != 0) return;
    const uint32_t id = blockIdx.x * 256 + threadIdx.x;
    const uint32_t ql = id / kTriSlice, rl = id % kTriSlice;
    const TriBlock b{o.r0, o.nr, o.q0, o.nq};
    const uint32_t i = o.q0 + ql, j = o.r0 + rl;
    bool live = tri_pair_counts(b, ql, rl);
    if (live) live = o.comp[i] != o.comp[j];
    if (__ballot(live) == 0) return;
    uint32_t common = 0, denom = 0;
    if (live) { common = o.loc_common[id]; denom = o.loc_denom[id]; }
    const uint64_t mine = mst_lanes_best(live ? mst_pack(common, denom, j) : 0ull, (int)kTriSlice);
    if (rl == 0 && mst_valid(mine)) mst_propose(o.best, i, mine);
    if (live) mst_propose(o.best, j, mst_pack(common, denom, i));
}

// step 2, stored source: one workgroup per row i = 1 .. n - 1 of the packed triangle, its threads stride over j < i.  All
// lanes share i: a thread keeps the best of its own pairs, a wave reduces, one lane per wave proposes to best[i].
__global__ __launch_bounds__(256) void mst_scan_kernel(const MstScan o)
{
    const uint32_t i = blockIdx.x + 1u;
    const uint32_t ci = o.comp[i];
    const uint64_t row = tri_index(i, 0);
    uint64_t mine = 0;
    for (uint32_t j = threadIdx.x; j < i; j += 256) {
        if (o.comp[j] == ci) continue;
        const uint32_t common = o.common[row + j], denom = o.denom[row + j];
        mine = mst_word_better(mine, mst_pack(common, denom, j));
        mst_propose(o.best, j, mst_pack(common, denom, i));
    }
    mine = mst_lanes_best(mine, 64);
    if ((threadIdx.x & 63u) == 0 && mst_valid(mine)) mst_propose(o.best, i, mine);
}

// step 3: every vertex that has a best edge stands for its component
__global__ __launch_bounds__(256) void mst_choose_kernel(const uint64_t *best, const uint32_t *comp, uint32_t *winner, uint32_t n)
{
    const uint32_t v = blockIdx.x * 256 + threadIdx.x;
    if (v >= n || !mst_valid(best[v])) return;
    mst_choose(winner, best, v, comp[v]);
}

// step 4: every root with a winner; the edges of the result are appended through one counter (never beyond `cap` = n - 1)
__global__ __launch_bounds__(256) void mst_hook_kernel(const MstHookArgs o)
{
    const uint32_t a = blockIdx.x * 256 + threadIdx.x;
    if (a >= o.n) return;
    const MstHook h = mst_hook(o.comp, o.winner, o.best, a);
    if (!h.picks) return;
    if (h.appends) {
        const unsigned long long at = atomicAdd(o.n_edges, 1ull);
        if (at < o.cap) {
            o.edge_i[at] = h.v > h.u ? h.v : h.u;
            o.edge_j[at] = h.v > h.u ? h.u : h.v;
            o.common[at] = h.common;
            o.denom[at] = h.denom;
            if (o.dist) o.dist[at] = tri_distance(h.common, h.denom, o.k);
        }
    }
    cluster_union(o.parent, h.v, h.u);
}

hipError_t launch_mst_reset(uint64_t *best, uint32_t *winner, uint32_t n, hipStream_t st)
{
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(mst_reset_kernel, dim3((n + 255) / 256), dim3(256), 0, st, best, winner, n);
    return hipGetLastError();
}

hipError_t launch_tri_mst(const MstOut &o, hipStream_t st)
{
    if (o.nq == 0) return hipSuccess;
    hipLaunchKernelGGL(tri_mst_kernel, dim3((o.nq * kTriSlice + 255) / 256), dim3(256), 0, st, o);
    return hipGetLastError();
}

hipError_t launch_mst_scan(const MstScan &o, hipStream_t st)
{
    if (o.n < 2) return hipSuccess;
    hipLaunchKernelGGL(mst_scan_kernel, dim3(o.n - 1), dim3(256), 0, st, o);
    return hipGetLastError();
}

hipError_t launch_mst_choose(const uint64_t *best, const uint32_t *comp, uint32_t *winner, uint32_t n, hipStream_t st)
{
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(mst_choose_kernel, dim3((n + 255) / 256), dim3(256), 0, st, best, comp, winner, n);
    return hipGetLastError();
}

hipError_t launch_mst_hook(const MstHookArgs &o, hipStream_t st)
{
    if (o.n == 0) return hipSuccess;
    hipLaunchKernelGGL(mst_hook_kernel, dim3((o.n + 255) / 256), dim3(256), 0, st, o);
    return hipGetLastError();
}

} // namespace mhx
