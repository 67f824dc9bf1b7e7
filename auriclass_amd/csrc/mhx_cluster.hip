// mhx_cluster.hip -- single-linkage clustering of ONE sketch set on the device (mhx_dist_cluster): the third pass that takes a
// block's results out of its block-local arrays -- not into a triangle or an edge list but into a lock-free union-find over
// parent[n] --, the pass that sets the arrays up and the flatten pass.  The blocks are the triangle's, computed by the passes
// of mhx_dist.hip and mhx_triangle.hip; the rules are the host+device functions of mhx_cluster.h.
#include "mhx_device.h"
#include "mhx_cluster.h"

namespace mhx {

// every list its own cluster, no neighbours yet
__global__ __launch_bounds__(256) void cluster_init_kernel(uint32_t *parent, uint32_t *degree, uint32_t n)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    parent[i] = i;
    if (degree) degree[i] = 0;
}

// The cells of tri_scatter_kernel and tri_edges_kernel, the same mapping and the same early return.  A pair that counts and
// passes the integer rule (cluster_keep: exact, no prefilter and no log) is an edge: the wave counts its edges with ONE
// atomic (the ballot of tri_edges_kernel), both ends get a neighbour, and the union joins their components.  Every access
// to `parent` in here is an agent-scope atomic (mhx_cluster.h).
__global__ __launch_bounds__(256) void tri_cluster_kernel(const ClusterOut o)
{
    if (*o.flag != 0) return;
    const uint32_t id = blockIdx.x * 256 + threadIdx.x;
    const uint32_t ql = id / kTriSlice, rl = id % kTriSlice;
    const TriBlock b{o.r0, o.nr, o.q0, o.nq};
    bool keep = tri_pair_counts(b, ql, rl);
    if (keep) keep = cluster_keep(o.loc_common[id], o.loc_denom[id], o.cmin, o.s);
    const unsigned long long votes = __ballot(keep);
    if (votes == 0) return;
    const uint32_t lane = threadIdx.x & 63u;
    if ((int)lane == __ffsll((long long)votes) - 1) atomicAdd(o.n_edges, (unsigned long long)__popcll(votes));
    if (!keep) return;
    const uint32_t i = o.q0 + ql, j = o.r0 + rl;
    if (o.degree) {
        atomicAdd(o.degree + i, 1u);
        atomicAdd(o.degree + j, 1u);
    }
    cluster_union(o.parent, i, j);
}

// one thread per list, a launch of its own (no union runs meanwhile); count != nullptr: the roots are counted, one atomic per wave
__global__ __launch_bounds__(256) void cluster_flatten_kernel(uint32_t *parent, uint32_t n, unsigned long long *count)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    const bool root = i < n && cluster_flatten(parent, i);
    if (!count) return;
    const unsigned long long votes = __ballot(root);
    if (votes == 0) return;
    if ((int)(threadIdx.x & 63u) == __ffsll((long long)votes) - 1) atomicAdd(count, (unsigned long long)__popcll(votes));
}

hipError_t launch_cluster_init(uint32_t *parent, uint32_t *degree, uint32_t n, hipStream_t st)
{
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(cluster_init_kernel, dim3((n + 255) / 256), dim3(256), 0, st, parent, degree, n);
    return hipGetLastError();
}

hipError_t launch_tri_cluster(const ClusterOut &o, hipStream_t st)
{
    if (o.nq == 0) return hipSuccess;
    hipLaunchKernelGGL(tri_cluster_kernel, dim3((o.nq * kTriSlice + 255) / 256), dim3(256), 0, st, o);
    return hipGetLastError();
}

hipError_t launch_cluster_flatten(uint32_t *parent, uint32_t n, unsigned long long *count, hipStream_t st)
{
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(cluster_flatten_kernel, dim3((n + 255) / 256), dim3(256), 0, st, parent, n, count);
    return hipGetLastError();
}

} // namespace mhx
