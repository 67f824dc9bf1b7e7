// mhx_support.hip -- jackknife support of search hits on the device (mhx_dist_support): all replicates of a (query, candidate)
// pair in ONE walk over the two original lists, the replicates on the lanes of a wave.  The rule, the shares, the step of the
// walk and the order are the host+device functions of mhx_support.h.  Four launches per batch of queries:
//   support_count_kernel  one workgroup per (query, slot, 64 replicates): how many hashes of the query (slot 0) or of candidate
//                         slot - 1 every replicate keeps; the waves take contiguous shares, the totals go through LDS
//   support_s_kernel      one thread per (query, replicate): s_r, the smallest kept count among the full lists of the set
//   support_pair_kernel   one workgroup per (query, candidate, 64 replicates): walk 1 counts the kept distinct values of every
//                         wave's share, the totals through LDS give each wave its start, walk 2 counts the shared ones while
//                         u <= s_r; a wave whose lanes all stand at their s_r leaves
//   support_best_kernel   one thread per (query, replicate): the best candidate in the search's order, and first[] by integer
//                         atomics (exact, the same from run to run)
// Every hash load is the same for all lanes of a wave (the wave index is made uniform for the compiler), so the loads are
// scalar and the vector unit does the keep test alone.  An index or a length that lies is clamped before it is used: no load
// leaves the matrices.  Not tuned beyond that.
#include "mhx_device.h"
#include "mhx_support.h"

namespace mhx {

namespace {

// candidates of query q that are looked at: never more than `top`, none without a reference set
__device__ __forceinline__ uint32_t support_ncand(const SupportArgs &a, uint32_t q)
{
    if (a.nr == 0) return 0;
    const uint32_t n = a.cand ? a.n_cand[q] : a.top;
    return n < a.top ? n : a.top;
}
// the reference of candidate i of query q, inside the set
__device__ __forceinline__ uint32_t support_ref(const SupportArgs &a, uint32_t q, uint32_t i)
{
    const uint32_t ref = a.cand ? a.cand[(uint64_t)q * a.top + i] : i;
    return ref < a.nr ? ref : a.nr - 1;
}
// slot 0: the query, slot 1 + i: candidate i; *full_len as the caller gave it, the return value inside the row
__device__ __forceinline__ uint32_t support_slot(const SupportArgs &a, uint32_t q, uint32_t slot, const uint64_t **row, uint32_t *full_len)
{
    if (slot == 0) {
        *row = a.q + (uint64_t)q * a.stride;
        *full_len = a.q_len[q];
    } else {
        const uint32_t ref = support_ref(a, q, slot - 1);
        *row = a.r + (uint64_t)ref * a.stride;
        *full_len = a.r_len[ref];
    }
    return *full_len < a.stride ? *full_len : a.stride;
}

} // namespace

__global__ __launch_bounds__(kSupportThreads) void support_count_kernel(const SupportArgs a)
{
    __shared__ uint32_t wave_kept[kSupportWaves][64];
    const uint32_t group = blockIdx.x, slot = blockIdx.y, q = blockIdx.z;
    const uint32_t lane = threadIdx.x & 63u, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (slot > support_ncand(a, q)) return; // the whole workgroup
    const uint64_t *row;
    uint32_t full_len;
    const uint32_t len = support_slot(a, q, slot, &row, &full_len);
    const uint32_t r = group * 64u + lane;
    const uint64_t lane_const = support_lane_const(a.seed, r);
    uint32_t j0, j1;
    support_share(len, kSupportWaves, wave, &j0, &j1);
    uint32_t kept = 0;
    for (uint32_t j = j0; j < j1; ++j) support_step_count(kept, support_keeps(row[j], lane_const, a.threshold));
    wave_kept[wave][lane] = kept;
    __syncthreads();
    if (wave != 0 || r >= a.replicates) return;
    uint32_t all = 0;
    for (uint32_t w = 0; w < kSupportWaves; ++w) all += wave_kept[w][lane];
    a.kept[((uint64_t)q * (a.top + 1) + slot) * a.replicates + r] = all;
}

__global__ __launch_bounds__(256) void support_s_kernel(const SupportArgs a)
{
    const uint32_t r = blockIdx.x * 256u + threadIdx.x, q = blockIdx.y;
    if (r >= a.replicates) return;
    const uint32_t n = support_ncand(a, q);
    uint32_t s_r = a.s;
    for (uint32_t slot = 0; slot <= n; ++slot) {
        const uint32_t len = slot == 0 ? a.q_len[q] : a.r_len[support_ref(a, q, slot - 1)];
        s_r = support_fold_s(s_r, len, a.s, a.kept[((uint64_t)q * (a.top + 1) + slot) * a.replicates + r]);
    }
    a.s_r[(uint64_t)q * a.replicates + r] = s_r;
    if (s_r == 0) atomicMin(a.bad, ((unsigned long long)(a.q0 + q) << 32) | r);
}

__global__ __launch_bounds__(kSupportThreads) void support_pair_kernel(const SupportArgs a)
{
    __shared__ uint32_t wave_count[kSupportWaves][64]; // u of every wave's share, then its c
    const uint32_t group = blockIdx.x, i = blockIdx.y, q = blockIdx.z;
    const uint32_t lane = threadIdx.x & 63u, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (i >= support_ncand(a, q)) return; // the whole workgroup
    const uint64_t *A, *B;
    uint32_t full;
    const uint32_t nA = support_slot(a, q, 1 + i, &A, &full), nB = support_slot(a, q, 0, &B, &full);
    const uint32_t r = group * 64u + lane;
    const bool live = r < a.replicates;
    const uint64_t lane_const = support_lane_const(a.seed, r);
    const uint32_t s_r = live ? a.s_r[(uint64_t)q * a.replicates + r] : 0u; // a lane beyond the replicates stands at its s_r from the start
    const SupportWalk share = support_walk_begin(A, nA, B, nB, kSupportWaves, wave);
    uint64_t v;
    bool counts, shared;
    // walk 1: the kept distinct values of the share
    uint32_t u = 0;
    for (SupportWalk w = share; support_walk_next(w, &v, &counts, &shared);)
        if (counts) support_step_count(u, support_keeps(v, lane_const, a.threshold));
    wave_count[wave][lane] = u;
    __syncthreads();
    uint32_t before = 0, u_all = 0;
    for (uint32_t w = 0; w < kSupportWaves; ++w) {
        const uint32_t x = wave_count[w][lane];
        if (w < wave) before += x;
        u_all += x;
    }
    __syncthreads(); // the totals are read before the c of the waves replace them
    // walk 2: the shared ones among the first s_r
    uint32_t c = 0;
    u = before;
    for (SupportWalk w = share; !__all(u >= s_r) && support_walk_next(w, &v, &counts, &shared);)
        if (counts) support_step(u, c, support_keeps(v, lane_const, a.threshold), shared, s_r);
    wave_count[wave][lane] = c;
    __syncthreads();
    if (wave != 0 || !live) return;
    uint32_t common = 0;
    for (uint32_t w = 0; w < kSupportWaves; ++w) common += wave_count[w][lane];
    const uint64_t at = ((uint64_t)q * a.top + i) * a.replicates + r;
    a.common[at] = common;
    a.denom[at] = support_denom(u_all, s_r);
}

__global__ __launch_bounds__(256) void support_best_kernel(const SupportArgs a)
{
    const uint32_t r = blockIdx.x * 256u + threadIdx.x, q = blockIdx.y;
    if (r >= a.replicates) return;
    const uint32_t n = support_ncand(a, q);
    uint32_t bi = 0, b_ref = kSupportNone, b_common = 0, b_denom = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const uint64_t at = ((uint64_t)q * a.top + i) * a.replicates + r;
        const uint32_t ref = support_ref(a, q, i), common = a.common[at], denom = a.denom[at];
        if (i == 0 || support_better(common, denom, ref, b_common, b_denom, b_ref)) { bi = i; b_ref = ref; b_common = common; b_denom = denom; }
    }
    if (a.best) a.best[(uint64_t)q * a.replicates + r] = b_ref;
    if (n) atomicAdd(&a.first[(uint64_t)q * a.top + bi], 1u);
}

namespace {
uint32_t support_groups(const SupportArgs &a) { return (a.replicates + 63u) / 64u; }
} // namespace

hipError_t launch_support_count(const SupportArgs &a, hipStream_t st)
{
    hipLaunchKernelGGL(support_count_kernel, dim3(support_groups(a), a.top + 1, a.nq), dim3(kSupportThreads), 0, st, a);
    return hipGetLastError();
}
hipError_t launch_support_s(const SupportArgs &a, hipStream_t st)
{
    hipLaunchKernelGGL(support_s_kernel, dim3((a.replicates + 255u) / 256u, a.nq), dim3(256), 0, st, a);
    return hipGetLastError();
}
hipError_t launch_support_pairs(const SupportArgs &a, hipStream_t st)
{
    hipLaunchKernelGGL(support_pair_kernel, dim3(support_groups(a), a.top, a.nq), dim3(kSupportThreads), 0, st, a);
    return hipGetLastError();
}
hipError_t launch_support_best(const SupportArgs &a, hipStream_t st)
{
    hipLaunchKernelGGL(support_best_kernel, dim3((a.replicates + 255u) / 256u, a.nq), dim3(256), 0, st, a);
    return hipGetLastError();
}

} // namespace mhx
