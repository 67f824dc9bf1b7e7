// mhx_contain.h -- the rules of the containment of one sketch in another (mhx_dist_contain: which share of a reference's
// hashes a query holds, read off the two bottom-s lists alone) that do not depend on how a GPU runs them, as host+device
// functions: the effective length and the bound of a list, tau, the pair walk of the generic kernel and the finish rule over
// the range data of a (query batch, reference slice) block.  The kernels in mhx_contain.hip call these functions;
// tests/emul/contain_emul.cpp runs the same text on the CPU.  The rule itself is restated in tests/contain_rule.py.
//
// The rule.  A list is the first min(len, stride, s) entries of its row, s the sketch size of ITS set.  A list of s entries
// is the complete hash set of its input up to its last entry, a shorter one is the complete set: bound = the last entry if
// the list holds s entries, 2^64 - 1 otherwise.  Below tau = min(bound(query), bound(reference)), tau included, both lists
// are complete, and
//     n_qry = #{x in query: x <= tau}, n_ref = #{x in reference: x <= tau}, shared = #{x in both: x <= tau}.
// 2^64 - 1 is a hash like any other.  Three integers per pair; no float is computed on the device.
#pragma once
#include "mhx_dist.h"
#include "mhx_support.h"

namespace mhx {

constexpr uint64_t kContainNoBound = ~0ull;    // the bound of a list that holds every hash of its input
constexpr uint32_t kContainPairThreads = 256;  // threads of a workgroup of contain_pairs_kernel: one share each

// ---- a list ---------------------------------------------------------------------------------------------------------------
MHX_HD uint32_t contain_eff_len(uint32_t len, uint32_t stride, uint32_t s)
{
    const uint32_t n = len < stride ? len : stride;
    return n < s ? n : s;
}
// n = contain_eff_len(.., s); s >= 1, so a full list has a last entry
MHX_HD uint64_t contain_bound(const uint64_t *row, uint32_t n, uint32_t s) { return n == s ? row[n - 1] : kContainNoBound; }
MHX_HD uint64_t contain_tau(uint64_t bound_q, uint64_t bound_r) { return bound_q < bound_r ? bound_q : bound_r; }
// entries <= tau of the ascending row[0 .. n)
MHX_HD uint32_t contain_prefix(const uint64_t *row, uint32_t n, uint64_t tau)
{
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (row[mid] <= tau) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// ---- the pair walk ----------------------------------------------------------------------------------------------------------
// The values both prefixes hold, A = reference[0 .. n_ref), B = query[0 .. n_qry): the merged sequence is cut into `shares`
// shares by merge-path diagonals (mhx_support.h); a shared value is counted where A's copy lies -- B's next hash equals it,
// whatever share that one lies in -- so the shares' counts add up to `shared`.
MHX_HD uint32_t contain_walk_shared(const uint64_t *A, uint32_t nA, const uint64_t *B, uint32_t nB, uint32_t shares, uint32_t share)
{
    uint32_t c = 0;
    uint64_t v;
    bool counts, shared;
    for (SupportWalk w = support_walk_begin(A, nA, B, nB, shares, share); support_walk_next(w, &v, &counts, &shared);) c += shared ? 1u : 0u;
    return c;
}

// ---- the finish rule over a block's range data ----------------------------------------------------------------------------------
// What the split and the range pass leave (mhx_dist.h): the offsets of every list per value range, the byte counters of the
// hashes shared per (query, range, reference), the call's shift.  The range of tau: every value of a lower range is below
// tau, every value of a higher one above it.  The shift comes from the largest VALUE of the call, so tau = 2^64 - 1 may lie
// above every range: the last range then takes its place, and all of it counts.
MHX_HD uint32_t contain_tau_range(uint64_t tau, uint32_t shift, uint32_t ranges)
{
    const uint64_t p = tau >> shift;
    return p < ranges - 1u ? (uint32_t)p : ranges - 1u;
}
// the 16 threads of a pair each sum a segment of rps = R / 16 ranges: the part of segment `seg` below range p_tau
MHX_HD uint32_t contain_segment_shared(const DistPair &x, uint32_t seg, uint32_t rps, uint32_t p_tau)
{
    const uint32_t end = (seg + 1) * rps < p_tau ? (seg + 1) * rps : p_tau;
    uint32_t c = 0;
    for (uint32_t p = seg * rps; p < end; ++p) c += x.cp[(uint64_t)p * x.cstride];
    return c;
}
// seg_shared: the kDistSegs sums of this pair, `stride` words apart.  The two slices of range p_tau are walked with two
// pointers up to tau; the offsets of that range are what lies below it.  x.A the reference, x.B the query (x.S is not read).
MHX_HD void contain_finish_walk(const DistPair &x, const uint32_t *seg_shared, uint32_t stride, uint32_t p_tau, uint64_t tau, uint32_t &shared,
                                uint32_t &n_qry, uint32_t &n_ref)
{
    uint32_t c = 0;
    for (uint32_t seg = 0; seg < (uint32_t)kDistSegs; ++seg) c += seg_shared[seg * stride];
    uint32_t i = x.orr[p_tau], j = x.oq[p_tau];
    const uint32_t ie = x.orr[p_tau + 1], je = x.oq[p_tau + 1];
    while (i < ie && j < je) {
        const uint64_t a = x.A[i], b = x.B[j];
        if (a > tau || b > tau) break;
        if (a < b) ++i;
        else if (b < a) ++j;
        else { ++i; ++j; ++c; }
    }
    while (i < ie && x.A[i] <= tau) ++i;
    while (j < je && x.B[j] <= tau) ++j;
    shared = c;
    n_ref = i;
    n_qry = j;
}

} // namespace mhx
