// mhx_contain_winner.h -- the rules of the winner-take-all containment (mhx_dist_contain_winner: every hash a query shares with
// the reference set is credited to ONE reference, the best-ranked of those it was found in) that do not depend on how a GPU
// runs them, as host+device functions: the ranking, the claim of one winner word, the walk of one pair that proposes, and
// the tally.  The kernels in mhx_contain_winner.hip call these functions; tests/emul/contain_winner_emul.cpp runs the same
// text on the CPU.  The rule itself is restated in tests/contain_winner_rule.py, on top of mhx_contain.h's.
//
// The rule, per query q.  found(q, r) = the values both lists hold up to tau(q, r); its size is the plain shared(q, r).
// r ranks before r' by the greater exact ratio shared / n_ref (compared as two 64-bit products: both factors are below 2^32),
// then the greater genome length, then the lower index.  winner(q, x) is the best-ranked r with x in found(q, r), and
// won(q, r) = #{x in found(q, r): winner(q, x) = r}.  A reference that found nothing never proposes, so n_ref == 0 never
// competes.
//
// The winner words.  One 32-bit word per position of the query's list, 0 = nobody: a found value is found AT a position
// of the query's prefix, so 2^64 - 1 needs no special case and no table is built.  A pair proposes r + 1 to the word of every
// value it found; the word is replaced only when the proposer ranks before its holder, so it rises along a total order and
// ends at the maximum whatever the order of arrival.  Nobody waits for anybody.
#pragma once
#include "mhx_cluster.h"
#include "mhx_contain.h"

namespace mhx {

constexpr uint32_t kContainClaimThreads = 256; // threads of a workgroup of contain_claim_kernel: one share of the pair's walk each

// the row of one query in the outputs of the plain pass, and the genome lengths (null: all equal)
struct ContainRanks {
    const uint32_t *shared, *n_ref; // [nr] of this query
    const uint64_t *ref_length;     // [nr] or null
};

// ---- the ranking ----------------------------------------------------------------------------------------------------------------
// a and b are distinct references that both found something for this query (so both n_ref > 0): does a rank before b
MHX_HD bool contain_ranks_before(const ContainRanks &k, uint32_t a, uint32_t b)
{
    const uint64_t x = (uint64_t)k.shared[a] * k.n_ref[b], y = (uint64_t)k.shared[b] * k.n_ref[a];
    if (x != y) return x > y;
    const uint64_t la = k.ref_length ? k.ref_length[a] : 0, lb = k.ref_length ? k.ref_length[b] : 0;
    if (la != lb) return la > lb;
    return a < b;
}

// ---- the claim of one word ------------------------------------------------------------------------------------------------------
// reference r proposes itself to `word` (0: nobody, else holder + 1).  The loop ends when r holds the word or somebody who
// ranks before r does; every exchange that succeeds moves the word up the order, so it runs at most as often as others do.
MHX_HD void contain_claim(uint32_t *word, const ContainRanks &k, uint32_t r)
{
    uint32_t held = cluster_load(word);
    while (held != r + 1 && (held == 0 || contain_ranks_before(k, r, held - 1))) {
        const uint32_t seen = cluster_cas(word, held, r + 1);
        if (seen == held) return;
        held = seen;
    }
}

// ---- the walk of one pair ---------------------------------------------------------------------------------------------------------
// A = reference[0 .. nA), B = query[0 .. nB), the two prefixes <= tau (n_ref and n_qry of the plain pass): share `share` of
// `shares` of their merged sequence (mhx_support.h), as contain_walk_shared cuts it.  A shared value is met where A's copy
// lies, B's copy is the walk's next entry of B: its position is the word.  Returns the values proposed.
MHX_HD uint32_t contain_claim_walk(const uint64_t *A, uint32_t nA, const uint64_t *B, uint32_t nB, uint32_t shares, uint32_t share, uint32_t *words,
                                   const ContainRanks &k, uint32_t r)
{
    uint32_t c = 0;
    uint64_t v;
    bool counts, shared;
    for (SupportWalk w = support_walk_begin(A, nA, B, nB, shares, share); support_walk_next(w, &v, &counts, &shared);)
        if (shared) { contain_claim(words + w.j, k, r); ++c; }
    return c;
}

// ---- won ------------------------------------------------------------------------------------------------------------------------
// the tally of one word: a held word adds 1 to won[holder] of its query's row (zeroed; integer adds, so any order gives the
// same sums)
MHX_HD void contain_tally(uint32_t word, uint32_t *won_row)
{
    if (word == 0) return;
#if defined(__HIP_DEVICE_COMPILE__)
    atomicAdd(won_row + (word - 1), 1u);
#else
    ++won_row[word - 1];
#endif
}

} // namespace mhx
