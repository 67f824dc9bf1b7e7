// mhx_contain_winner.hip -- winner-take-all containment on the device (mhx_dist_contain_winner): over the three counts that the
// plain pass (mhx_contain.hip) has left for every pair, the claim pass credits every value a query shares with the reference
// set to the best-ranked reference it was found in, and the tally counts what every reference won.  The rules are the
// host+device functions of mhx_contain_winner.h.
#include "mhx_device.h"
#include "mhx_contain_winner.h"

namespace mhx {

constexpr uint32_t kContainClaimRows = 32768; // queries of a batch per launch of the claim kernel: the grid's y

// One workgroup per pair (x: the reference, y: the query of the batch, from ql0 on).  A pair that shares nothing is done
// after one load, the same on every lane.  Otherwise the two prefixes <= tau are known already -- n_ref and n_qry of the
// plain pass --, every thread walks a share of their merged sequence and proposes the reference to the word of every shared
// value (contain_claim_walk): a compare-and-swap loop that ends when the word holds this reference or a better one.
__global__ __launch_bounds__(kContainClaimThreads) void contain_claim_kernel(const ContainArgs a, const ContainWinnerArgs w, uint32_t ql0)
{
    const uint32_t ri = blockIdx.x, ql = ql0 + blockIdx.y, qi = a.q0 + ql;
    const uint64_t row = (uint64_t)qi * a.out_stride;
    if (a.shared[row + ri] == 0) return;
    const ContainRanks k{a.shared + row, a.n_ref + row, w.ref_length};
    contain_claim_walk(a.r + (uint64_t)ri * a.stride, a.n_ref[row + ri], a.q + (uint64_t)qi * a.stride, a.n_qry[row + ri], kContainClaimThreads, threadIdx.x,
                       w.words + (uint64_t)ql * w.width, k, ri);
    if (threadIdx.x == 0) atomicAdd(w.pairs, 1ull);
}

// One thread per word of the batch: a held word adds 1 to won[query][holder].  Integer adds on zeroed outputs: the sums are
// exact and the same from run to run.
__global__ __launch_bounds__(256) void contain_tally_kernel(const ContainArgs a, const ContainWinnerArgs w)
{
    const uint64_t id = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (id >= (uint64_t)a.bnq * w.width) return;
    const uint32_t ql = (uint32_t)(id / w.width);
    contain_tally(w.words[id], w.won + (uint64_t)(a.q0 + ql) * a.out_stride);
}

hipError_t launch_contain_claim(const ContainArgs &a, const ContainWinnerArgs &w, hipStream_t st)
{
    if (a.bnq == 0 || a.nr == 0) return hipSuccess;
    if (a.nr > 0x7FFFFFFFu) return hipErrorInvalidValue;
    for (uint32_t ql0 = 0; ql0 < a.bnq; ql0 += kContainClaimRows) {
        const uint32_t rows = a.bnq - ql0 < kContainClaimRows ? a.bnq - ql0 : kContainClaimRows;
        hipLaunchKernelGGL(contain_claim_kernel, dim3(a.nr, rows), dim3(kContainClaimThreads), 0, st, a, w, ql0);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t launch_contain_tally(const ContainArgs &a, const ContainWinnerArgs &w, hipStream_t st)
{
    const uint64_t n = (uint64_t)a.bnq * w.width;
    if (n == 0) return hipSuccess;
    if ((n + 255) / 256 > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(contain_tally_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, a, w);
    return hipGetLastError();
}

} // namespace mhx
