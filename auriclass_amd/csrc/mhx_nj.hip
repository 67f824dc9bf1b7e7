// mhx_nj.hip -- neighbour joining over ONE sketch set on the device (mhx_dist_nj): the init pass over the packed triangle of
// the dense mode and the three launches of a join -- scan, join, update -- over one 64-bit distance word per pair of nodes,
// the row sums r [n] and the compacted list of active ids.  The rules are the host+device functions of mhx_nj.h.  Every
// hand-off between workgroups crosses a kernel boundary.  Within a launch no work item reads a word that another one
// writes; the two atomics are 64-bit INTEGER adds (the new r[b], the count of clamped updates), whose sums do not depend on
// the order of arrival.  No floating point decides anything: the two divisions of nj_lengths are the only doubles.
#include "mhx_device.h"
#include "mhx_nj.h"

namespace mhx {

namespace {

constexpr uint32_t kNjJoinThreads = kNjMaxBlocks; // one workgroup, one candidate per thread
constexpr uint32_t kNjScanUnroll = 4;

__device__ __forceinline__ NjState nj_state(const NjArgs &a) { return NjState{a.words, a.r, a.n}; }

// the first candidate, in the candidate order, among the 64 lanes of a wave; every lane calls this
__device__ __forceinline__ NjCand nj_wave_best(NjCand c)
{
    for (int off = 32; off > 0; off >>= 1) {
        NjCand o;
        o.q = (int64_t)__shfl_xor((unsigned long long)c.q, off, 64);
        o.lo = (uint32_t)__shfl_xor((int)c.lo, off, 64);
        o.hi = (uint32_t)__shfl_xor((int)c.hi, off, 64);
        c = nj_cand_better(c, o);
    }
    return c;
}
// ... among the WAVES waves of a workgroup; every thread calls this, the result is valid in wave 0
template <uint32_t WAVES> __device__ __forceinline__ NjCand nj_block_best(NjCand c, NjCand *lds)
{
    static_assert(WAVES <= 64, "one wave reduces the waves' results");
    c = nj_wave_best(c);
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (lane == 0) lds[wave] = c;
    __syncthreads();
    if (wave == 0) c = nj_wave_best(lane < WAVES ? lds[lane] : nj_no_cand());
    return c;
}
// the sum of v over the 64 lanes of a wave, in every lane
__device__ __forceinline__ uint64_t nj_wave_sum(uint64_t v)
{
    for (int off = 32; off > 0; off >>= 1) v += (uint64_t)__shfl_xor((unsigned long long)v, off, 64);
    return v;
}

} // namespace

// the words of all pairs from the triangle's common / denom (the same packed index); every list an active node
__global__ __launch_bounds__(256) void nj_init_kernel(const NjArgs a, const uint32_t *common, const uint32_t *denom, uint64_t pairs)
{
    const uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (p < pairs) a.words[p] = linkage_fixed_distance(common[p], denom[p], a.k);
    if (p < a.n) a.act[0][p] = (uint32_t)p;
    if (p <= a.n) a.pre[0][p] = p ? p * (p - 1) / 2 : 0;
    if (p < 6) a.ctl[p] = 0;
}

// the first r: workgroup i adds row i (contiguous) and column i of the words
__global__ __launch_bounds__(256) void nj_rowsum_kernel(const NjArgs a)
{
    __shared__ uint64_t lds[4];
    const uint32_t i = blockIdx.x;
    uint64_t sum = 0;
    for (uint32_t j = threadIdx.x; j < i; j += 256) sum += a.words[tri_index(i, j)];
    for (uint32_t c = i + 1 + threadIdx.x; c < a.n; c += 256) sum += a.words[tri_index(c, i)];
    sum = nj_wave_sum(sum);
    if ((threadIdx.x & 63u) == 0) lds[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) a.r[i] = lds[0] + lds[1] + lds[2] + lds[3];
}

// join t, scan: the words of the active rows in equal spans, one per workgroup (nj_span); a workgroup walks the rows its
// span falls into, its threads stride over the columns -- 8-byte loads, neighbours in a wave at neighbouring addresses --,
// and its first candidate in the candidate order goes to cand[blockIdx.x]
__global__ __launch_bounds__(kNjScanThreads) void nj_scan_kernel(const NjArgs a, uint32_t t)
{
    __shared__ NjCand lds[kNjScanThreads / 64];
    NjCand mine = nj_no_cand();
    if (a.ctl[5] == 0) {
        const uint32_t m = a.n - t;
        const uint32_t *act = a.act[t & 1u];
        const uint64_t *pre = a.pre[t & 1u];
        uint64_t w0, w1;
        nj_span(pre[m], gridDim.x, blockIdx.x, w0, w1);
        if (w0 < w1)
            for (uint32_t p = nj_first_row(pre, m, w0); p < m && pre[p] < w1; ++p) {
                const uint32_t i = act[p];
                if (i >= a.n) break;
                uint32_t c0, c1;
                nj_row_part(pre, p, i, w0, w1, c0, c1);
                const uint64_t ri = a.r[i];
                const uint64_t *row = a.words + tri_index(i, 0);
                // kNjScanUnroll columns per thread and turn, their loads issued before the first comparison
                for (uint32_t j0 = c0 + threadIdx.x; j0 < c1; j0 += kNjScanUnroll * kNjScanThreads) {
                    uint64_t d[kNjScanUnroll], rj[kNjScanUnroll];
#pragma unroll
                    for (uint32_t u = 0; u < kNjScanUnroll; ++u) {
                        const uint32_t j = j0 + u * kNjScanThreads;
                        d[u] = j < c1 ? row[j] : 0;
                        rj[u] = j < c1 ? a.r[j] : kNjDead;
                    }
#pragma unroll
                    for (uint32_t u = 0; u < kNjScanUnroll; ++u) mine = nj_cand_better(mine, nj_word_candidate(m, i, ri, j0 + u * kNjScanThreads, d[u], rj[u]));
                }
            }
    }
    mine = nj_block_best<kNjScanThreads / 64>(mine, lds);
    if (threadIdx.x == 0) a.cand[blockIdx.x] = mine;
}

// join t: ONE workgroup reduces the candidates of the scan's `blocks` workgroups, writes record t with its lengths and
// leaves the pick for the update; with two nodes left there is nothing to pick
__global__ __launch_bounds__(kNjJoinThreads) void nj_join_kernel(const NjArgs a, uint32_t t, uint32_t blocks)
{
    __shared__ NjCand lds[kNjJoinThreads / 64];
    const uint32_t m = a.n - t;
    NjCand mine = m > 2u && threadIdx.x < blocks ? a.cand[threadIdx.x] : nj_no_cand();
    mine = nj_block_best<kNjJoinThreads / 64>(mine, lds);
    if (threadIdx.x != 0 || a.ctl[5] != 0) return;
    const NjState s = nj_state(a);
    const uint32_t *act = a.act[t & 1u];
    NjRecord rec;
    if (m > 2u) {
        NjPick k;
        if (!nj_join(s, act, m, mine, rec, k)) { a.ctl[5] = 1; return; }
        a.ctl[0] = k.a; a.ctl[1] = k.b; a.ctl[2] = k.pos_a; a.ctl[3] = k.d;
    } else {
        if (act[0] >= act[1] || act[1] >= a.n) { a.ctl[5] = 1; return; }
        rec = nj_last_record(s, act);
    }
    a.join_a[t] = rec.a; a.join_b[t] = rec.b;
    a.d[t] = rec.d; a.r_a[t] = rec.r_a; a.r_b[t] = rec.r_b;
    if (a.len_a && a.len_b) nj_lengths(rec, m, a.len_a[t], a.len_b[t]);
}

// join t, update: one thread per position p = 0 .. m of the active list.  It moves its entry of the list and of the running
// sums to the copy of the next join (a leaves), and -- its node c neither a nor b -- joins the words (a, c) and (b, c) into
// (b, c) and corrects r[c] (nj_update); the shares of the new r[b] are added per wave
__global__ __launch_bounds__(256) void nj_update_kernel(const NjArgs a, uint32_t t)
{
    const uint32_t m = a.n - t, p = blockIdx.x * 256 + threadIdx.x;
    if (a.ctl[5] != 0) return; // (uniform)
    const NjPick k{(uint32_t)a.ctl[0], (uint32_t)a.ctl[1], (uint32_t)a.ctl[2], a.ctl[3]};
    if (k.a >= a.n || k.b >= k.a || k.pos_a >= m) return; // (uniform)
    const uint32_t from = t & 1u, to = from ^ 1u;
    uint64_t share = 0, clamped = 0;
    uint32_t q;
    uint64_t sum;
    if (p <= m && nj_compact(k, a.pre[from], p, q, sum)) {
        a.pre[to][q] = sum;
        if (p < m) {
            const uint32_t c = a.act[from][p];
            a.act[to][q] = c;
            if (c != k.b && c != k.a && c < a.n) {
                const NjWord w = nj_update(nj_state(a), k, c);
                share = w.d;
                clamped = w.clamped ? 1 : 0;
            }
        }
    }
    share = nj_wave_sum(share);
    clamped = nj_wave_sum(clamped);
    if ((threadIdx.x & 63u) != 0) return;
    if (share) atomicAdd((unsigned long long *)(a.r + k.b), (unsigned long long)share);
    if (clamped) atomicAdd((unsigned long long *)(a.ctl + 4), (unsigned long long)clamped);
}

hipError_t launch_nj_init(const NjArgs &a, const uint32_t *common, const uint32_t *denom, hipStream_t st)
{
    const uint64_t pairs = (uint64_t)a.n * (a.n - 1) / 2, items = pairs > a.n + 1ull ? pairs : a.n + 1ull;
    hipLaunchKernelGGL(nj_init_kernel, dim3((uint32_t)((items + 255) / 256)), dim3(256), 0, st, a, common, denom, pairs);
    hipLaunchKernelGGL(nj_rowsum_kernel, dim3(a.n), dim3(256), 0, st, a);
    return hipGetLastError();
}
hipError_t launch_nj_scan(const NjArgs &a, uint32_t t, hipStream_t st)
{
    hipLaunchKernelGGL(nj_scan_kernel, dim3(nj_scan_blocks(a.n, a.n - t)), dim3(kNjScanThreads), 0, st, a, t);
    return hipGetLastError();
}
hipError_t launch_nj_join(const NjArgs &a, uint32_t t, hipStream_t st)
{
    hipLaunchKernelGGL(nj_join_kernel, dim3(1), dim3(kNjJoinThreads), 0, st, a, t, a.n - t > 2u ? nj_scan_blocks(a.n, a.n - t) : 0u);
    return hipGetLastError();
}
hipError_t launch_nj_update(const NjArgs &a, uint32_t t, hipStream_t st)
{
    hipLaunchKernelGGL(nj_update_kernel, dim3((a.n - t + 1 + 255) / 256), dim3(256), 0, st, a, t);
    return hipGetLastError();
}

} // namespace mhx
