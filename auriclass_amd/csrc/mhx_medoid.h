// mhx_medoid.h -- the rules of the MEDOID of every cluster of a partition of ONE sketch set (mhx_dist_medoids) and of the pair
// "a list against its target" (mhx_dist_to) that do not depend on how a GPU runs them, as host+device functions: the pick key,
// the validity of a label array, which blocks of the triangle's schedule hold a pair of one cluster (host), the cell rule of
// the sum pass with the roles of a wave's lanes in its combine, and the walk of the pair kernel.  The kernels in
// mhx_medoid.hip call these functions; tests/emul/medoid_emul.cpp runs the same text on the CPU.  The rule itself is restated
// in tests/medoid_rule.py.
//
// The rule.  label[i] is the lowest index of i's cluster (what mhx_dist_cluster, mhx_mst_labels and mhx_linkage_labels
// return; any array with label[i] <= i and label[label[i]] == label[i] is one).  sum[i] is the sum of the fixed-point
// distances (linkage_fixed_distance, units of 2^-32) of i to the other members of its cluster; the medoid of a cluster is its
// member with the smallest (sum, index).  Limits: those of the tree (n <= 65 536, s < 2^20).
#pragma once
#include "mhx_linkage.h"
#include "mhx_support.h"

namespace mhx {

// ---- the pick key -------------------------------------------------------------------------------------------------------------
// sum << 16 | index: the smallest key of a cluster is its medoid, ties on the sum to the lower index.  A sum is at most
// n - 1 distances of at most 2^32 each.
constexpr uint32_t kMedoidIndexBits = 16;
constexpr uint64_t kMedoidMaxSum = (uint64_t)(kTriMaxLists - 1) * kLinkOne;
constexpr uint64_t kMedoidNoKey = ~0ull; // best[l] before the pick: above every key
static_assert(kTriMaxLists <= (1u << kMedoidIndexBits), "an index fits the low bits of the key");
static_assert(kMedoidMaxSum < (1ull << (64 - kMedoidIndexBits)), "the largest sum fits the high bits of the key");
static_assert(((kMedoidMaxSum << kMedoidIndexBits) | (kTriMaxLists - 1)) < kMedoidNoKey, "no key equals the empty word");

MHX_HD uint64_t medoid_key(uint64_t sum, uint32_t index) { return sum << kMedoidIndexBits | index; }
MHX_HD uint64_t medoid_key_sum(uint64_t key) { return key >> kMedoidIndexBits; }
MHX_HD uint32_t medoid_key_index(uint64_t key) { return (uint32_t)(key & ((1u << kMedoidIndexBits) - 1u)); }

// ---- labels -------------------------------------------------------------------------------------------------------------------
// the first i whose label is not a cluster's lowest member, n when the array is a partition
inline uint32_t medoid_first_bad_label(const uint32_t *label, uint32_t n)
{
    for (uint32_t i = 0; i < n; ++i)
        if (label[i] > i || label[label[i]] != label[i]) return i;
    return n;
}

// ---- the block predicate (host) -------------------------------------------------------------------------------------------------
// The members of every cluster in index order: those of the cluster with label l are member[start[l] .. start[l + 1]), an
// empty range when l is no label.  start [n + 1], member [n]; label a partition; O(n).
inline void medoid_members(const uint32_t *label, uint32_t n, uint32_t *start, uint32_t *member)
{
    for (uint32_t l = 0; l <= n; ++l) start[l] = 0;
    for (uint32_t i = 0; i < n; ++i) ++start[label[i]];
    uint32_t end = 0;
    for (uint32_t l = 0; l < n; ++l) { end += start[l]; start[l] = end; } // where l's members end
    start[n] = n;
    for (uint32_t i = n; i-- > 0;) member[--start[label[i]]] = i;        // and, filled from the back, where they begin
}
// A block is run iff it holds a pair that counts (tri_pair_counts) and has equal labels.  Exact: reference r of the slice
// counts with the queries max(q0, r + 1) .. q0 + nq - 1, and the first member of r's cluster at or above that bound -- one
// binary search -- is among them or no member is.  O(32 log n) per block.
inline bool medoid_block_runs(const TriBlock &b, const uint32_t *label, const uint32_t *start, const uint32_t *member)
{
    for (uint32_t rl = 0; rl < b.nr; ++rl) {
        const uint32_t r = b.r0 + rl, l = label[r], from = b.q0 > r + 1u ? b.q0 : r + 1u;
        uint32_t lo = start[l], hi = start[l + 1];
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if (member[mid] < from) lo = mid + 1; else hi = mid;
        }
        if (lo < start[l + 1] && member[lo] - b.q0 < b.nq) return true;
    }
    return false;
}

// ---- the sum pass ---------------------------------------------------------------------------------------------------------------
// The cells of tri_cluster_kernel: cell id of a block is (query ql = id / 32, reference rl = id % 32).  A cell contributes
// when its pair counts and both ends carry one label; what it contributes, to sum[i] and to sum[j], is the fixed-point
// distance of the pair.  The 40-step logarithm of that distance runs for such cells alone.
MHX_HD bool medoid_cell_counts(const TriBlock &b, uint32_t ql, uint32_t rl, const uint32_t *label)
{
    return tri_pair_counts(b, ql, rl) && label[b.q0 + ql] == label[b.r0 + rl];
}
MHX_HD uint64_t medoid_cell_value(uint32_t common, uint32_t denom, int k) { return linkage_fixed_distance(common, denom, k); }
// A wave holds 2 query rows x 32 references: lane l and lane l ^ 32 share a reference, the 32 lanes of a half share a query.
// The values of a half are summed by exchanges with the lanes l ^ 16, l ^ 8 .. l ^ 1 (every lane then holds the half's
// sum) and added once, by the half's first lane; the two values of a reference are summed by one exchange with lane l ^ 32
// and added once, by the lane of the lower half: 2 + 32 adds per wave at the most, whatever the partition.
constexpr uint32_t kMedoidRowLanes = kTriSlice;
MHX_HD bool medoid_row_adder(uint32_t lane) { return (lane & (kMedoidRowLanes - 1u)) == 0; }
MHX_HD bool medoid_ref_adder(uint32_t lane) { return lane < kMedoidRowLanes; }
// `votes`: bit l is set when lane l's cell contributes.  Whether any cell of the lane's query row / of its reference does:
// the adders add only then, so that no index outside the block is ever formed into an address.
MHX_HD bool medoid_row_any(uint64_t votes, uint32_t lane) { return ((votes >> (lane & kMedoidRowLanes)) & 0xFFFFFFFFull) != 0; }
MHX_HD bool medoid_ref_any(uint64_t votes, uint32_t lane) { return ((votes >> (lane & (kMedoidRowLanes - 1u))) & 0x100000001ull) != 0; }

// ---- the pick ---------------------------------------------------------------------------------------------------------------------
// best[l] starts at kMedoidNoKey; every list i proposes medoid_key(sum[i], i) to best[label[i]] with a 64-bit minimum.

// ---- the pair walk ----------------------------------------------------------------------------------------------------------------
// (common, denom) of two ascending duplicate-free lists at sketch size s by the pair rule of the distance path (mash's
// compareSketches): denom = min(s, distinct values of A u B), common = the values both lists hold among the first s distinct
// ones.  The walk of mhx_support.h without the keep test: the merged sequence -- A's copy of a shared value first -- is cut
// into `shares` shares by merge-path diagonals; a distinct value is counted where its first copy lies, and it is shared iff
// B's next hash equals it, whatever share that one lies in.  Walk 1 counts the distinct values of a share; an exclusive
// prefix sum over the shares gives every share the count it starts from; walk 2 counts the shared values while the running
// count is at most s and ends when it reaches s.
constexpr uint32_t kMedoidPairThreads = 256; // threads of a workgroup of dist_to_kernel: one share each

MHX_HD uint32_t medoid_walk_distinct(const uint64_t *A, uint32_t nA, const uint64_t *B, uint32_t nB, uint32_t shares, uint32_t share)
{
    uint32_t u = 0;
    uint64_t v;
    bool counts, shared;
    for (SupportWalk w = support_walk_begin(A, nA, B, nB, shares, share); support_walk_next(w, &v, &counts, &shared);) u += counts ? 1u : 0u;
    return u;
}
// start: the distinct values of the shares before this one
MHX_HD uint32_t medoid_walk_common(const uint64_t *A, uint32_t nA, const uint64_t *B, uint32_t nB, uint32_t shares, uint32_t share, uint32_t start,
                                   uint32_t s)
{
    uint32_t u = start, c = 0;
    uint64_t v;
    bool counts, shared;
    SupportWalk w = support_walk_begin(A, nA, B, nB, shares, share);
    while (u < s && support_walk_next(w, &v, &counts, &shared)) {
        if (!counts) continue;
        ++u;
        if (shared) ++c; // u <= s here
    }
    return c;
}
MHX_HD uint32_t medoid_denom(uint32_t distinct, uint32_t s) { return distinct < s ? distinct : s; }

} // namespace mhx
