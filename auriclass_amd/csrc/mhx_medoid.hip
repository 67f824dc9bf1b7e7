// mhx_medoid.hip -- the medoid of every cluster of a partition of ONE sketch set on the device (mhx_dist_medoids) and the pair
// "a list against its target" (mhx_dist_to): the take-out pass that adds the in-cluster distances of a block to sum[n], the
// two passes of the pick, and the pair kernel.  The blocks are the triangle's, computed by the passes of mhx_dist.hip and
// mhx_triangle.hip; the rules are the host+device functions of mhx_medoid.h.
#include "mhx_device.h"
#include "mhx_block.h"
#include "mhx_medoid.h"

namespace mhx {

// The cells of tri_cluster_kernel, the same mapping and the same early return.  A pair that counts and whose ends carry one
// label adds its fixed-point distance to the sums of both ends: 64-bit integer adds, exact in any order of arrival.  The
// wave combines before it adds (mhx_medoid.h): one add per query row and one per reference.  label is an input of the call:
// plain loads.  MHX_MEDOID_PAIR_ATOMICS: two adds per pair instead, the form tools/medoid_rate.py measures the combine against.
__global__ __launch_bounds__(256) void tri_medoid_kernel(const MedoidOut o)
{
    if (*o.flag != 0) return;
    const uint32_t id = blockIdx.x * 256 + threadIdx.x;
    const uint32_t ql = id / kTriSlice, rl = id % kTriSlice;
    const TriBlock b{o.r0, o.nr, o.q0, o.nq};
    const bool in = medoid_cell_counts(b, ql, rl, o.label);
    const unsigned long long votes = __ballot(in);
    if (votes == 0) return;
    const unsigned long long v = in ? medoid_cell_value(o.loc_common[id], o.loc_denom[id], o.k) : 0ull;
    const uint32_t i = o.q0 + ql, j = o.r0 + rl;
#if defined(MHX_MEDOID_PAIR_ATOMICS)
    if (in && v) {
        atomicAdd(o.sum + i, v);
        atomicAdd(o.sum + j, v);
    }
#else
    const uint32_t lane = threadIdx.x & 63u;
    unsigned long long row = v;
#pragma unroll
    for (int x = (int)kMedoidRowLanes / 2; x >= 1; x >>= 1) row += __shfl_xor(row, x);
    const unsigned long long ref = v + __shfl_xor(v, (int)kMedoidRowLanes);
    if (medoid_row_adder(lane) && medoid_row_any(votes, lane) && row) atomicAdd(o.sum + i, row);
    if (medoid_ref_adder(lane) && medoid_ref_any(votes, lane) && ref) atomicAdd(o.sum + j, ref);
#endif
}

// one thread per list: its key to the best of its cluster
__global__ __launch_bounds__(256) void medoid_pick_kernel(const uint32_t *label, const unsigned long long *sum, unsigned long long *best, uint32_t n)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    atomicMin(best + label[i], (unsigned long long)medoid_key(sum[i], i));
}

// a launch of its own behind the pick: the index part of the cluster's best key
__global__ __launch_bounds__(256) void medoid_write_kernel(const uint32_t *label, const unsigned long long *best, uint32_t *medoid, uint32_t n)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    medoid[i] = medoid_key_index(best[label[i]]);
}

// One workgroup per list i: the pair rule of (i, target[i]), a share of the merged sequence per thread (mhx_medoid.h).  A
// list compared with itself, an empty list and len < s take the same path.  target is checked by the host: below n.
__global__ __launch_bounds__(kMedoidPairThreads) void dist_to_kernel(const DistToArgs a)
{
    __shared__ uint32_t wave_u[kMedoidPairThreads / 64], wave_c[kMedoidPairThreads / 64];
    const uint32_t i = blockIdx.x, t = a.target[i];
    const uint64_t *A = a.rows + (uint64_t)t * a.stride, *B = a.rows + (uint64_t)i * a.stride;
    const uint32_t nA = a.len[t] < a.stride ? a.len[t] : a.stride, nB = a.len[i] < a.stride ? a.len[i] : a.stride; // (a device-form length is not the host's to check)
    uint32_t distinct = 0, common = 0;
    const uint32_t u = medoid_walk_distinct(A, nA, B, nB, kMedoidPairThreads, threadIdx.x);
    const uint32_t start = block_scan_excl<(int)kMedoidPairThreads>(u, wave_u, distinct);
    const uint32_t c = medoid_walk_common(A, nA, B, nB, kMedoidPairThreads, threadIdx.x, start, a.s);
    block_scan_excl<(int)kMedoidPairThreads>(c, wave_c, common);
    if (threadIdx.x == 0) {
        a.common[i] = common;
        a.denom[i] = medoid_denom(distinct, a.s);
    }
}

hipError_t launch_tri_medoid(const MedoidOut &o, hipStream_t st)
{
    if (o.nq == 0) return hipSuccess;
    hipLaunchKernelGGL(tri_medoid_kernel, dim3((o.nq * kTriSlice + 255) / 256), dim3(256), 0, st, o);
    return hipGetLastError();
}

hipError_t launch_medoid_pick(const uint32_t *label, const unsigned long long *sum, unsigned long long *best, uint32_t *medoid, uint32_t n, hipStream_t st)
{
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(medoid_pick_kernel, dim3((n + 255) / 256), dim3(256), 0, st, label, sum, best, n);
    hipLaunchKernelGGL(medoid_write_kernel, dim3((n + 255) / 256), dim3(256), 0, st, label, best, medoid, n);
    return hipGetLastError();
}

hipError_t launch_dist_to(const DistToArgs &a, hipStream_t st)
{
    if (a.n == 0) return hipSuccess;
    hipLaunchKernelGGL(dist_to_kernel, dim3(a.n), dim3(kMedoidPairThreads), 0, st, a);
    return hipGetLastError();
}

} // namespace mhx
