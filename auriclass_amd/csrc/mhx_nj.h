// mhx_nj.h -- the rules of NEIGHBOUR JOINING over ONE sketch set (mhx_dist_nj) that do not depend on how a GPU runs them, as
// host+device functions: Q of a pair, the candidate order (Q, lo, hi), the split of a pick scan into equal spans of words,
// the candidate of one word, the record of a join, the update of one node against a join, and the two length formulas.
// The kernels in mhx_nj.hip call these functions; tests/emul/nj_emul.cpp runs the same text on the CPU.
//
// Nodes carry the index of their lowest leaf.  One 64-bit word per pair of nodes lies at the triangle's packed index
// tri_index(hi, lo) of the two ids: d in units of 2^-32, 0 .. 2^32, at the start linkage_fixed_distance of the leaf pair.
// r[i] is the sum of d(i, c) over the active c != i, kNjDead once i is no node any more.  With m active nodes
//     Q(i, j) = (m - 2) d(i, j) - r[i] - r[j]      (signed 64 bits; |Q| < 2^50 for n <= 65 536)
// and the pair with the smallest Q joins, ties to the lower lo, then the lower hi.  The join of (a, b), b < a, reuses the row
// and column of b for the new node u, and a dies:
//     d(u, c) = max(0, (d(a, c) + d(b, c) - d(a, b)) >> 1)     (arithmetic shift: floor)
// The clamp at 0 is NOT textbook neighbour joining, which lets negative distances stand (and grow by 1.5 x per level): it keeps
// every word in 0 .. 2^32 for ever, so one uint64_t per pair does.  How often it changed a value is counted.
//     r[c] += d(u, c) - d(a, c) - d(b, c),   r[u] = sum of d(u, c)
// All of it is integer arithmetic: sums in any order give the same word, and nothing is decided by floating point.  The two
// branch lengths of a join are the only doubles: one exact conversion, one correctly rounded division, one exact scaling.
// Limits: those of the linkage (s < 2^20, n <= 65 536).
#pragma once
#include "mhx_linkage.h"

namespace mhx {

constexpr uint32_t kNjNone = 0xFFFFFFFFu;  // NjCand::hi: no candidate
constexpr uint64_t kNjDead = ~0ull;        // r[i] of an id that is no node (any more)
constexpr uint32_t kNjScanThreads = 256;   // threads of a workgroup of the pick scan
constexpr uint32_t kNjMaxBlocks = 1024;    // workgroups of the pick scan at most: one workgroup reduces their candidates
constexpr uint32_t kNjBlockWords = 2048;   // ... and each takes at least this many words, while there are as many

// ---- Q and the candidate order ---------------------------------------------------------------------------------------------
MHX_HD int64_t nj_q(uint32_t m, uint64_t d, uint64_t ri, uint64_t rj) { return (int64_t)(m - 2u) * (int64_t)d - (int64_t)ri - (int64_t)rj; }

// (q, lo, hi) ascending: total over distinct pairs, so every join's pick is unique.  hi == kNjNone: no candidate.
struct NjCand { int64_t q; uint32_t lo, hi; };
MHX_HD NjCand nj_no_cand() { return NjCand{0, kNjNone, kNjNone}; }
MHX_HD bool nj_cand_precedes(const NjCand &a, const NjCand &b)
{
    if (a.hi == kNjNone) return false;
    if (b.hi == kNjNone) return true;
    if (a.q != b.q) return a.q < b.q;
    return a.lo != b.lo ? a.lo < b.lo : a.hi < b.hi;
}
MHX_HD NjCand nj_cand_better(const NjCand &a, const NjCand &b) { return nj_cand_precedes(b, a) ? b : a; }

// ---- the state of a call ------------------------------------------------------------------------------------------------------
// words [n (n - 1) / 2]; r [n].  The active ids lie ascending in act [m]; pre [m + 1] are the running sums of the lengths of
// their rows (row i of the packed triangle holds i words): pre[p] = sum of act[q], q < p, so that pre[m] words are to be
// scanned.  Both lists exist twice: join t reads copy t & 1 and the update writes the other one.
struct NjState {
    uint64_t *words, *r;
    uint32_t n;
};
// what a join leaves for the update of the same step (ctl[0 .. 3] of the kernels)
struct NjPick {
    uint32_t a, b, pos_a; // pos_a: where a lies in act
    uint64_t d;           // d(a, b)
};
// record t of a call: the two nodes, their distance and their r as they were before the join
struct NjRecord {
    uint32_t a, b;
    uint64_t d, r_a, r_b;
};

// ---- the pick scan --------------------------------------------------------------------------------------------------------------
// The workgroups of the scan with m active nodes of n: the words of the m longest rows bound what is there to scan.  Host.
MHX_HD uint32_t nj_scan_blocks(uint32_t n, uint32_t m)
{
    const uint64_t below = n - m, most = (uint64_t)n * (n - 1u) / 2u - (below ? below * (below - 1u) / 2u : 0u);
    const uint64_t blocks = (most + kNjBlockWords - 1u) / kNjBlockWords;
    return blocks < 1u ? 1u : (blocks > kNjMaxBlocks ? kNjMaxBlocks : (uint32_t)blocks);
}
// workgroup b of `blocks` takes the words [w0, w1) of the total: equal spans of WORDS, whatever rows they fall into
MHX_HD void nj_span(uint64_t total, uint32_t blocks, uint32_t b, uint64_t &w0, uint64_t &w1)
{
    const uint64_t span = (total + blocks - 1u) / blocks;
    w0 = (uint64_t)b * span < total ? (uint64_t)b * span : total;
    w1 = w0 + span < total ? w0 + span : total;
}
// the row in which word w0 < pre[m] lies: the last p with pre[p] <= w0 (row 0 holds no word and is stepped over)
MHX_HD uint32_t nj_first_row(const uint64_t *pre, uint32_t m, uint64_t w0)
{
    uint32_t lo = 0, hi = m; // pre[lo] <= w0 < pre[hi]
    while (hi - lo > 1u) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (pre[mid] <= w0) lo = mid; else hi = mid;
    }
    return lo;
}
// the columns [c0, c1) of the row at position p, id i, that lie in the span [w0, w1)
MHX_HD void nj_row_part(const uint64_t *pre, uint32_t p, uint32_t i, uint64_t w0, uint64_t w1, uint32_t &c0, uint32_t &c1)
{
    const uint64_t base = pre[p];
    c0 = base < w0 ? (uint32_t)(w0 - base) : 0u;
    c1 = w1 - base < (uint64_t)i ? (uint32_t)(w1 - base) : i;
}
// what column j offers to the active row i, j < i: a dead column is read and skipped
MHX_HD NjCand nj_word_candidate(uint32_t m, uint32_t i, uint64_t ri, uint32_t j, uint64_t d, uint64_t rj)
{
    if (rj == kNjDead) return nj_no_cand();
    return NjCand{nj_q(m, d, ri, rj), j, i};
}
MHX_HD NjCand nj_scan_candidate(const NjState &s, uint32_t m, uint32_t i, uint64_t ri, uint32_t j)
{
    return nj_word_candidate(m, i, ri, j, s.words[tri_index(i, j)], s.r[j]);
}

// ---- the join ---------------------------------------------------------------------------------------------------------------------
// The record of the pick c among m > 2 active nodes, and what the update needs; a dies and the sum of b starts anew.
// One work item, behind the reduction of the candidates.  False: no pair although nodes are left.
MHX_HD bool nj_join(const NjState &s, const uint32_t *act, uint32_t m, const NjCand &c, NjRecord &rec, NjPick &p)
{
    if (c.hi >= s.n || c.lo >= c.hi) return false;
    const uint64_t d = s.words[tri_index(c.hi, c.lo)];
    rec = NjRecord{c.hi, c.lo, d, s.r[c.hi], s.r[c.lo]};
    uint32_t lo = 0, hi = m; // act ascends: act[lo] <= a < act[hi]
    while (hi - lo > 1u) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (act[mid] <= c.hi) lo = mid; else hi = mid;
    }
    p = NjPick{c.hi, c.lo, lo, d};
    s.r[c.hi] = kNjDead;
    s.r[c.lo] = 0;
    return act[lo] == c.hi;
}
// the last record: the two nodes that are left, no r
MHX_HD NjRecord nj_last_record(const NjState &s, const uint32_t *act) { return NjRecord{act[1], act[0], s.words[tri_index(act[1], act[0])], 0, 0}; }

// ---- the update ---------------------------------------------------------------------------------------------------------------------
struct NjWord { uint64_t d; bool clamped; };
MHX_HD NjWord nj_join_word(uint64_t dac, uint64_t dbc, uint64_t dab)
{
    const int64_t v = ((int64_t)(dac + dbc) - (int64_t)dab) >> 1; // arithmetic: floor
    return v < 0 ? NjWord{0, true} : NjWord{(uint64_t)v, false};
}
// Where position p of the list of join t goes in the list behind it (a leaves), and the running sum that goes with it;
// p = 0 .. m, position m carrying the total alone.  False: p is a's own position.
MHX_HD bool nj_compact(const NjPick &k, const uint64_t *pre, uint32_t p, uint32_t &q, uint64_t &sum)
{
    if (p == k.pos_a) return false;
    q = p > k.pos_a ? p - 1u : p;
    sum = p > k.pos_a ? pre[p] - k.a : pre[p];
    return true;
}
// Node c, active and neither a nor b, against the join k.  Work item c reads the words (a, c) and (b, c), writes the word
// (b, c) and r[c] of ITSELF only; what it returns is its share of the new r[b], which the caller adds (an integer sum: any
// order gives the same word).
MHX_HD NjWord nj_update(const NjState &s, const NjPick &k, uint32_t c)
{
    const uint64_t at_a = c < k.a ? tri_index(k.a, c) : tri_index(c, k.a), at_b = c < k.b ? tri_index(k.b, c) : tri_index(c, k.b);
    const uint64_t dac = s.words[at_a], dbc = s.words[at_b];
    const NjWord w = nj_join_word(dac, dbc, k.d);
    s.words[at_b] = w.d;
    s.r[c] = s.r[c] + w.d - dac - dbc;
    return w;
}

// ---- branch lengths ---------------------------------------------------------------------------------------------------------------
// of the node whose r is r_mine in a join among m > 2 nodes: the numerator is an integer below 2^53, so every host and the
// device give the same double
MHX_HD double nj_length(uint64_t d, uint32_t m, uint64_t r_mine, uint64_t r_other)
{
    const int64_t num = (int64_t)d * (int64_t)(m - 2u) + (int64_t)r_mine - (int64_t)r_other;
    return (double)num / (double)(2 * (int64_t)(m - 2u)) * (1.0 / 4294967296.0);
}
// both lengths of a record made with m nodes active; the last one (m == 2) gives a the whole distance
MHX_HD void nj_lengths(const NjRecord &rec, uint32_t m, double &len_a, double &len_b)
{
    if (m <= 2u) { len_a = (double)rec.d * (1.0 / 4294967296.0); len_b = 0.0; return; }
    len_a = nj_length(rec.d, m, rec.r_a, rec.r_b);
    len_b = nj_length(rec.d, m, rec.r_b, rec.r_a);
}

} // namespace mhx
