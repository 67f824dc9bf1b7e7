// mhx_contain.hip -- containment of reference sketches in query sketches on the device (mhx_dist_contain): the bounds of
// every list, the finish pass of the range route over what the split and the range pass of mhx_dist.hip leave for a block,
// and the generic pair kernel.  The rules are the host+device functions of mhx_contain.h.
#include "mhx_device.h"
#include "mhx_block.h"
#include "mhx_contain.h"

namespace mhx {

// One thread per list of either set, once per call: the effective length (a length the caller could not check is clipped
// here, padding behind it never counts) and the bound.
__global__ __launch_bounds__(256) void contain_bounds_kernel(const ContainArgs a)
{
    const uint32_t id = blockIdx.x * 256 + threadIdx.x;
    if (id >= a.nq + a.nr) return;
    const bool isq = id < a.nq;
    const uint32_t li = isq ? id : id - a.nq, s = isq ? a.s_q : a.s_r;
    const uint64_t *row = (isq ? a.q : a.r) + (uint64_t)li * a.stride;
    const uint32_t n = contain_eff_len((isq ? a.q_len : a.r_len)[li], a.stride, s);
    (isq ? a.q_eff : a.r_eff)[li] = n;
    (isq ? a.q_bound : a.r_bound)[li] = contain_bound(row, n, s);
}

// 16 pairs per workgroup, the layout of dist_finish_kernel: thread (seg, pair) sums the byte counters of its R / 16 ranges
// below the range of tau, then the 16 threads of segment 0 add the sums and walk the two slices of that range up to tau
// (contain_finish_walk).  The three counts go to their place in the call's outputs, or, for the containment search, into its
// block-local arrays (ContainArgs: out_base).
__global__ __launch_bounds__(256) void contain_finish_kernel(const ContainArgs a, const DistWork w)
{
    __shared__ uint32_t seg_shared[kDistSegs][16];
    if (w.params[1] != 0) return; // the range pass gave this block up: cells of cpart are unwritten, the pair kernel redoes it
    const uint32_t R = w.ranges, rps = R / kDistSegs, per = R + 1;
    const uint32_t pl = threadIdx.x & 15, seg = threadIdx.x >> 4;
    const uint32_t pair = blockIdx.x * 16 + pl;
    const bool live = pair < a.bnq * a.bnr;
    const uint32_t ql = live ? pair / a.bnr : 0, rl = live ? pair % a.bnr : 0;
    const uint32_t qi = a.q0 + ql, ri = a.r0 + rl;
    const uint32_t cstride = 4 * ((a.bnr + 3) / 4);
    const DistPair x{w.cpart + (uint64_t)ql * R * cstride + rl, cstride, w.offs_q + ql * per, w.offs_r + rl * per,
                     a.r + (uint64_t)ri * a.stride, a.q + (uint64_t)qi * a.stride, 0u};
    const uint64_t tau = contain_tau(a.q_bound[qi], a.r_bound[ri]);
    const uint32_t p_tau = contain_tau_range(tau, *a.shift, R);
    seg_shared[seg][pl] = contain_segment_shared(x, seg, rps, p_tau);
    __syncthreads();
    if (seg != 0 || !live) return;
    uint32_t shared, n_qry, n_ref;
    contain_finish_walk(x, &seg_shared[0][pl], 16, p_tau, tau, shared, n_qry, n_ref);
    const uint64_t out = (uint64_t)qi * a.out_stride + ri - a.out_base;
    a.shared[out] = shared;
    a.n_qry[out] = n_qry;
    a.n_ref[out] = n_ref;
}

// One workgroup per pair of the block: the two prefixes <= tau by binary search (the same loads on every lane), the shared
// values of a share of their merged sequence per thread, and a workgroup sum.  Tiny batches, flagged blocks, lists without a
// geometry; a short list against a full one of a large genome, whose slices pass 255 entries, always comes here.
__global__ __launch_bounds__(kContainPairThreads) void contain_pairs_kernel(const ContainArgs a)
{
    __shared__ uint32_t wave_c[kContainPairThreads / 64];
    const uint32_t ql = blockIdx.x / a.bnr, rl = blockIdx.x % a.bnr;
    const uint32_t qi = a.q0 + ql, ri = a.r0 + rl;
    const uint64_t *A = a.r + (uint64_t)ri * a.stride, *B = a.q + (uint64_t)qi * a.stride;
    const uint64_t tau = contain_tau(a.q_bound[qi], a.r_bound[ri]);
    const uint32_t nA = contain_prefix(A, a.r_eff[ri], tau), nB = contain_prefix(B, a.q_eff[qi], tau);
    const uint32_t c = contain_walk_shared(A, nA, B, nB, kContainPairThreads, threadIdx.x);
    uint32_t shared = 0;
    block_scan_excl<(int)kContainPairThreads>(c, wave_c, shared);
    if (threadIdx.x == 0) {
        const uint64_t out = (uint64_t)qi * a.out_stride + ri - a.out_base;
        a.shared[out] = shared;
        a.n_qry[out] = nB;
        a.n_ref[out] = nA;
    }
}

hipError_t launch_contain_bounds(const ContainArgs &a, hipStream_t st)
{
    const uint64_t n = (uint64_t)a.nq + a.nr;
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(contain_bounds_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_contain_finish(const ContainArgs &a, const DistWork &w, hipStream_t st)
{
    const uint32_t pairs = a.bnq * a.bnr;
    if (pairs == 0) return hipSuccess;
    hipLaunchKernelGGL(contain_finish_kernel, dim3((pairs + 15) / 16), dim3(256), 0, st, a, w);
    return hipGetLastError();
}

hipError_t launch_contain_pairs(const ContainArgs &a, hipStream_t st)
{
    const uint64_t pairs = (uint64_t)a.bnq * a.bnr;
    if (pairs == 0) return hipSuccess;
    hipLaunchKernelGGL(contain_pairs_kernel, dim3((unsigned)pairs), dim3(kContainPairThreads), 0, st, a);
    return hipGetLastError();
}

} // namespace mhx
