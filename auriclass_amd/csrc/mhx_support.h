// mhx_support.h -- the rule of the JACKKNIFE SUPPORT OF SEARCH HITS (mhx_dist_support, mhx_search_files_support) that does not
// depend on how a GPU runs it, as host+device functions: the keep test of one replicate on top of its per-lane constant, the
// share of the merged sequence of two lists that one wave walks, the step of the walk, s_r from kept counts, and the order of
// two candidates.  The kernels in mhx_support.hip call these functions; tests/emul/support_emul.cpp runs the same text on the
// CPU.  The rule itself is restated in tests/support_rule.py.
//
// The rule.  For a query list Q and its candidate reference lists C_0 .. C_{m-1} (m <= 64), replicate r (0-based) of a call
// with `seed` and `keep` is replicate r of mhx_resample.h over the set [Q, C_0, ..]: the same keep function, "full" means
// len == s, s_r is the smallest kept count among the full lists of THIS set (s when none is full; 0 fails), every list is cut
// to its first min(kept, s_r) hashes.  (common, denom) of candidate i are those of the pair rule (mash's compareSketches) over
// the cut lists at sketch size s_r; the best candidate of the replicate is the first in the order of the search
// (mhx_search.h: search_better); first[i] is the number of replicates whose best candidate is i.
//
// The cut does not matter.  Given s_r, the pair rule over the cut lists equals the pair rule over the kept lists as they are:
// if a kept list holds at least s_r hashes, its cut lies at its s_r-th hash, and the s_r-th distinct value of the union of the
// two kept lists lies at or below that; so everything the rule counts -- the first s_r distinct values of the union -- lies
// below both cuts, and if neither list reaches s_r neither is cut.  So one ascending walk over the distinct values of A u B
// does it: per replicate u counts the kept distinct values, c those among them that both lists hold while u <= s_r; then
// common = c and denom = min(s_r, u).  A replicate keeps or drops a hash by its value alone, so all replicates take the same
// walk: the replicates lie on the lanes of a wave, every load is the same for all lanes, only the keep test and the counters
// differ.
//
// The walk.  The merged sequence of A (reference) and B (query) -- ascending, A's copy of a shared value first -- is cut into
// one share per wave by merge-path diagonals.  A distinct value is counted where its first copy lies: at A's copy when A holds
// it (it is shared iff B's next hash equals it, whatever share that one lies in), at B's copy otherwise; B's copy of a shared
// value counts nothing.  Walk 1 counts u over the share; the waves' totals give every wave the u its lanes start from; walk 2
// counts c while u <= s_r and ends when no lane is below its s_r any more.
//
// Memory.  The kept counts, s_r, the best reference and the pair results of a batch of queries are (3 top + 3) * 4 * replicates
// bytes per query; the engine cuts the queries into batches so that this stays below kSupportWorkLimit (256 MiB; MHX_SUPPORT_WORK_MB
// sets another bound in MiB, at least one query per batch).
#pragma once
#include "mhx_resample.h"
#include "mhx_search.h"

namespace mhx {

constexpr uint32_t kSupportThreads = 1024; // threads of a workgroup of the count and pair kernels
constexpr uint32_t kSupportWaves = kSupportThreads / 64;
constexpr uint32_t kSupportMaxTop = kSearchMaxTop; // candidates per query
constexpr uint32_t kSupportNone = 0xFFFFFFFFu;     // rep_best of a query without candidates
constexpr uint64_t kSupportWorkLimit = 256ull << 20;
constexpr uint32_t kSupportMaxBatch = 32768;       // queries of a batch: the z extent of a grid

// ---- keep -------------------------------------------------------------------------------------------------------------------
// the part of resample_mix that does not depend on the hash: one constant per lane
MHX_HD uint64_t support_lane_const(uint64_t seed, uint32_t r) { return seed + ((uint64_t)r + 1u) * kResampleGamma; }
// resample_keeps(h, seed, r, T) with lane_const = support_lane_const(seed, r)
MHX_HD bool support_keeps(uint64_t h, uint64_t lane_const, uint64_t T)
{
    uint64_t z = h + lane_const;
    z = (z ^ (z >> 30)) * kResampleMul1;
    z = (z ^ (z >> 27)) * kResampleMul2;
    return ((z ^ (z >> 31)) >> 32) < T;
}

// ---- shares -----------------------------------------------------------------------------------------------------------------
// number of A elements among the first `diag` merged elements (A first on ties); A and B ascending without duplicates
MHX_HD uint32_t support_merge_path(const uint64_t *A, uint32_t nA, const uint64_t *B, uint32_t nB, uint32_t diag)
{
    uint32_t lo = diag > nB ? diag - nB : 0, hi = diag < nA ? diag : nA;
    while (lo < hi) {
        const uint32_t i = (lo + hi) >> 1, j = diag - 1 - i;
        if (A[i] <= B[j]) lo = i + 1; else hi = i;
    }
    return lo;
}
// merged positions [d0, d1) of wave `wave` of `waves`; a share may be empty
MHX_HD void support_share(uint32_t total, uint32_t waves, uint32_t wave, uint32_t *d0, uint32_t *d1)
{
    const uint32_t per = (total + waves - 1) / waves;
    const uint64_t from = (uint64_t)wave * per;
    *d0 = from < total ? (uint32_t)from : total;
    *d1 = total - *d0 < per ? total : *d0 + per;
}

// One wave's share of a pair, and where its walk stands.  next() takes the next merged element: false when the share is
// done; otherwise `value`, whether it is the first copy of a distinct value (`counts`) and whether both lists hold it.
struct SupportWalk {
    const uint64_t *A, *B;
    uint32_t nA, nB, i, j, i1, j1;
};
MHX_HD SupportWalk support_walk_begin(const uint64_t *A, uint32_t nA, const uint64_t *B, uint32_t nB, uint32_t waves, uint32_t wave)
{
    uint32_t d0, d1;
    support_share(nA + nB, waves, wave, &d0, &d1);
    SupportWalk w{A, B, nA, nB, 0, 0, 0, 0};
    w.i = support_merge_path(A, nA, B, nB, d0);
    w.i1 = support_merge_path(A, nA, B, nB, d1);
    w.j = d0 - w.i;
    w.j1 = d1 - w.i1;
    return w;
}
MHX_HD bool support_walk_next(SupportWalk &w, uint64_t *value, bool *counts, bool *shared)
{
    if (w.i >= w.i1 && w.j >= w.j1) return false;
    if (w.i < w.i1 && (w.j >= w.j1 || w.A[w.i] <= w.B[w.j])) {
        const uint64_t v = w.A[w.i++];
        *value = v;
        *counts = true;
        *shared = w.j < w.nB && w.B[w.j] == v; // B's next hash, in this share or the next
    } else {
        const uint64_t v = w.B[w.j];
        *value = v;
        *counts = !(w.i > 0 && w.A[w.i - 1] == v); // the second copy of a shared value counts nothing
        *shared = false;
        ++w.j;
    }
    return true;
}

// ---- the step of one lane -----------------------------------------------------------------------------------------------------
// one distinct value that the lane's replicate keeps or not, walk 1: u alone
MHX_HD void support_step_count(uint32_t &u, bool keeps) { u += keeps ? 1u : 0u; }
// walk 2: u and c; a shared value counts while it is among the first s_r kept distinct values
MHX_HD void support_step(uint32_t &u, uint32_t &c, bool keeps, bool shared, uint32_t s_r)
{
    if (!keeps) return;
    ++u;
    if (shared && u <= s_r) ++c;
}
MHX_HD uint32_t support_denom(uint32_t u_all, uint32_t s_r) { return u_all < s_r ? u_all : s_r; }

// ---- s_r --------------------------------------------------------------------------------------------------------------------
// fold the kept count of one more list of a replicate's set into s_r, which starts at s
MHX_HD uint32_t support_fold_s(uint32_t s_r, uint32_t len, uint32_t s, uint32_t kept)
{
    return resample_full(len, s) && kept < s_r ? kept : s_r;
}

// ---- the order ----------------------------------------------------------------------------------------------------------------
// candidate a = (common, denom, reference index) is better than b: the search's order
MHX_HD bool support_better(uint32_t a_common, uint32_t a_denom, uint32_t a_ref, uint32_t b_common, uint32_t b_denom, uint32_t b_ref)
{
    return search_better(SearchHit{a_ref, a_common, a_denom}, SearchHit{b_ref, b_common, b_denom});
}

// ---- memory -------------------------------------------------------------------------------------------------------------------
// bytes of workspace per query of a batch: kept counts [top + 1], s_r and the best reference, common and denom [top], all x replicates
MHX_HD uint64_t support_query_bytes(uint32_t top, uint32_t replicates) { return 4ull * replicates * (3ull * top + 3ull); }
MHX_HD uint32_t support_batch(uint32_t top, uint32_t replicates, uint64_t limit)
{
    const uint64_t n = limit / support_query_bytes(top, replicates);
    return n < 1 ? 1u : n > kSupportMaxBatch ? kSupportMaxBatch : (uint32_t)n;
}

} // namespace mhx
