// mhx_linkage.h -- the rules of the COMPLETE- and AVERAGE-linkage agglomeration of ONE sketch set (mhx_dist_linkage) that do
// not depend on how a GPU runs them, as host+device functions: the fixed-point distance, the value word of a cluster pair
// with its combine and its order, the candidate order (value, lo, hi), the pieces of a step -- the candidate of a row, the
// update of one cluster against a merge, the candidate of one partner in a row scan -- and the cut of the finished merges.
// The kernels in mhx_linkage.hip call these functions; tests/emul/linkage_emul.cpp runs the same text on the CPU.
//
// Clusters carry the index of their lowest member.  One 64-bit word per cluster pair lies at the triangle's packed index
// tri_index(hi, lo) of the two ids; the merge of (a, b), b < a, reuses the row and column of b, and a dies.  Nothing here is
// combined with an atomic: every word has one writer per launch, so the result does not depend on the order of arrival.
//   complete: word = common << 32 | denom of the WORST leaf pair (the smallest Jaccard index, mst_index_cmp's exact
//             comparison; of two equal indices the one with the greater denom, so that the word is fully determined)
//   average:  word = num, the sum of the fixed-point distances of all leaf pairs; den = |A| |B| follows from size[]
// Limits: those of the tree (s < 2^20, n <= 65 536): den <= 2^30 and num <= 2^30 * 2^32 fit 64-bit words.
#pragma once
#include "mhx_mst.h"

namespace mhx {

constexpr int kLinkComplete = 1, kLinkAverage = 2;
constexpr uint32_t kLinkNone = 0xFFFFFFFFu;        // nn[i]: row i has no active partner below i; LinkCand::hi: no candidate
constexpr uint64_t kLinkOne = 1ull << 32;          // the fixed-point distance 1
constexpr uint64_t kLinkLn2 = 2977044471ull;       // floor(ln 2 * 2^32)

MHX_HD uint64_t link_mulhi(uint64_t a, uint64_t b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul64hi(a, b);
#else
    return (uint64_t)(((unsigned __int128)a * b) >> 64);
#endif
}

// ---- the fixed-point distance ---------------------------------------------------------------------------------------------
// q(common, denom, k) = min(1, -ln(2 j / (1 + j)) / k) in units of 2^-32, j = common / denom, in integers alone, so that the
// device, the host and the Python restatement (tests/linkage_rule.py) give the same word: log2 of y = (1 + j) / (2 j) >= 1 bit
// by bit -- the integer part from the position of y's top bit, 40 fraction bits by squaring the mantissa 40 times --, times
// ln 2, over k.  common <= denom < 2^21 (the caller's to see to): (common + denom) << 42 stays below 2^64.
MHX_HD uint64_t linkage_fixed_distance(uint32_t common, uint32_t denom, int k)
{
    if (common == denom) return 0;
    if (common == 0) return kLinkOne;
    const uint64_t y = (((uint64_t)common + denom) << 42) / (2ull * common); // (1 + j) / (2 j) in units of 2^-42, >= 2^42
    uint32_t e = 63;
    while (!(y >> e)) --e;
    uint64_t z = y << (63u - e); // the mantissa in [1, 2) in units of 2^-63
    uint64_t G = e - 42u;
    for (int it = 0; it < 40; ++it) {
        z = link_mulhi(z, z); // the square in [1, 4) in units of 2^-62
        if (z >> 63) G = 2 * G + 1;
        else { G = 2 * G; z <<= 1; }
    }
    // G = log2 y in units of 2^-40 (below 2^45); (G * ln2) >> 40 from the 128-bit product
    const uint64_t hi = link_mulhi(G, kLinkLn2), lo = G * kLinkLn2;
    const uint64_t q = (hi << 24 | lo >> 40) / (uint64_t)k;
    return q < kLinkOne ? q : kLinkOne;
}

// ---- the value of a cluster pair ------------------------------------------------------------------------------------------
// w: the word; den: |A| |B| (average; 1 and unused for complete)
struct LinkVal { uint64_t w, den; };

MHX_HD uint64_t link_complete_word(uint32_t common, uint32_t denom) { return (uint64_t)common << 32 | denom; }
// < 0: a is the smaller linkage value (the closer pair), 0: equal, > 0: b is
MHX_HD int link_cmp(int linkage, const LinkVal &a, const LinkVal &b)
{
    if (linkage == kLinkComplete) return -mst_index_cmp((uint32_t)(a.w >> 32), (uint32_t)a.w, (uint32_t)(b.w >> 32), (uint32_t)b.w);
    // num_a / den_a against num_b / den_b: the cross products in 128 bits
    const uint64_t lh = link_mulhi(a.w, b.den), ll = a.w * b.den, rh = link_mulhi(b.w, a.den), rl = b.w * a.den;
    if (lh != rh) return lh < rh ? -1 : 1;
    return ll < rl ? -1 : (ll > rl ? 1 : 0);
}
// V(A u B, C) from V(A, C) and V(B, C)
MHX_HD uint64_t link_combine(int linkage, uint64_t wa, uint64_t wb)
{
    if (linkage != kLinkComplete) return wa + wb;
    const int c = link_cmp(kLinkComplete, LinkVal{wa, 1}, LinkVal{wb, 1});
    if (c != 0) return c > 0 ? wa : wb;                 // the worse of the two
    return (uint32_t)wa >= (uint32_t)wb ? wa : wb;      // equal indices: the greater denom
}

// ---- the candidate order ----------------------------------------------------------------------------------------------------
// (value, lo, hi) ascending: total over distinct pairs, so every step's pick is unique.  hi == kLinkNone: no candidate.
struct LinkCand { uint64_t w, den; uint32_t lo, hi; };
MHX_HD LinkCand link_no_cand() { return LinkCand{0, 1, kLinkNone, kLinkNone}; }
MHX_HD bool link_cand_precedes(int linkage, const LinkCand &a, const LinkCand &b)
{
    if (a.hi == kLinkNone) return false;
    if (b.hi == kLinkNone) return true;
    const int c = link_cmp(linkage, LinkVal{a.w, a.den}, LinkVal{b.w, b.den});
    if (c != 0) return c < 0;
    return a.lo != b.lo ? a.lo < b.lo : a.hi < b.hi;
}
MHX_HD LinkCand link_cand_better(int linkage, const LinkCand &a, const LinkCand &b) { return link_cand_precedes(linkage, b, a) ? b : a; }

// ---- the state of a call ------------------------------------------------------------------------------------------------------
// words [n (n - 1) / 2]; size [n]: members of cluster i, 0 when i is not a cluster (any more); nn [n]: the best active
// partner j < i of row i -- the first of row i's pairs in the candidate order, i.e. ties to the lower j --, kLinkNone when
// there is none.  Row i of the packed triangle is contiguous, so a scan of it is coalesced.
struct LinkState {
    uint64_t *words;
    uint32_t *size, *nn;
    uint32_t n;
    int linkage;
};
// the record a pick leaves for the update of the same step: the pair and its sizes
struct LinkPick { uint32_t a, b, size_a, size_b; };

MHX_HD uint64_t link_den(const LinkState &s, uint32_t i, uint32_t j) { return s.linkage == kLinkComplete ? 1ull : (uint64_t)s.size[i] * s.size[j]; }
// the first word of a pair from the triangle's common / denom
MHX_HD uint64_t link_init_word(int linkage, uint32_t common, uint32_t denom, int k)
{
    return linkage == kLinkComplete ? link_complete_word(common, denom) : linkage_fixed_distance(common, denom, k);
}

// pick: what row i offers -- its cached best pair -- or nothing
MHX_HD LinkCand link_row_candidate(const LinkState &s, uint32_t i)
{
    if (i == 0 || s.size[i] == 0) return link_no_cand();
    const uint32_t j = s.nn[i];
    if (j == kLinkNone) return link_no_cand();
    return LinkCand{s.words[tri_index(i, j)], link_den(s, i, j), j, i};
}
// rescan: what partner j offers to row i (j < i, row i active)
MHX_HD LinkCand link_scan_candidate(const LinkState &s, uint32_t i, uint32_t j)
{
    if (s.size[j] == 0) return link_no_cand();
    return LinkCand{s.words[tri_index(i, j)], link_den(s, i, j), j, i};
}
// what a merge writes to the result: num / den of the step (complete: common / denom of the decisive pair)
MHX_HD void link_record(int linkage, const LinkCand &c, uint64_t &num, uint64_t &den)
{
    if (linkage == kLinkComplete) { num = c.w >> 32; den = c.w & 0xFFFFFFFFull; }
    else { num = c.w; den = c.den; }
}

// update: cluster c against the merge p of clusters a and b (b < a; a dies, b takes both).  Work item c reads the words
// (a, c) and (b, c), writes the word (b, c), size[c] and nn[c] of ITSELF only, and reads size[] of clusters other than a and
// b -- nothing another work item of the same step writes.  True: row c must be scanned again (its cached partner died, or
// was b and the pair with it got worse, or c is the merged cluster itself, whose whole row is new).
MHX_HD bool link_update(const LinkState &s, const LinkPick &p, uint32_t c)
{
    if (c == p.a) { s.size[c] = 0; return false; }
    if (c == p.b) { s.size[c] = p.size_a + p.size_b; return true; }
    if (s.size[c] == 0) return false;
    const uint64_t at_a = c < p.a ? tri_index(p.a, c) : tri_index(c, p.a), at_b = c < p.b ? tri_index(p.b, c) : tri_index(c, p.b);
    const uint64_t was = s.words[at_b];
    const uint64_t w = link_combine(s.linkage, s.words[at_a], was);
    s.words[at_b] = w;
    if (c < p.b) return false; // the pair lies in row b, which is scanned again anyway
    const uint32_t j = s.nn[c];
    if (j == p.a) return true;
    const bool complete = s.linkage == kLinkComplete;
    const uint64_t sc = s.size[c];
    const LinkCand fresh{w, complete ? 1ull : sc * ((uint64_t)p.size_a + p.size_b), p.b, c};
    // the cached partner is b itself: every partner below b was strictly worse than the old (b, c) and every one above it no
    // better, so b stays first unless the pair got worse (complete linkage never improves a pair; where all values tie,
    // nothing is scanned again but row b)
    if (j == p.b) return link_cmp(s.linkage, LinkVal{fresh.w, fresh.den}, LinkVal{was, complete ? 1ull : sc * p.size_b}) > 0;
    const LinkCand held = j == kLinkNone ? link_no_cand() : LinkCand{s.words[tri_index(c, j)], complete ? 1ull : sc * s.size[j], j, c};
    if (link_cand_precedes(s.linkage, fresh, held)) s.nn[c] = p.b;
    return false;
}

// ---- heights and the cut ----------------------------------------------------------------------------------------------------
// average: two conversions, one division and an exact scaling, so that every host reproduces the double bit for bit
MHX_HD double link_average_height(uint64_t num, uint64_t den) { return ((double)num / (double)den) * (1.0 / 4294967296.0); }
MHX_HD double link_height(int linkage, uint64_t num, uint64_t den, int k)
{
    return linkage == kLinkComplete ? tri_distance((uint32_t)num, (uint32_t)den, k) : link_average_height(num, den);
}

// The clusters at max_dist: the merges from the first one on while dist[t] <= max_dist, none behind the first that is not;
// label[i] = the lowest index of i's cluster.  Returns the number of clusters.  Host only: exported as mhx_linkage_labels.
inline uint32_t linkage_labels(const uint32_t *merge_a, const uint32_t *merge_b, const double *dist, uint32_t n, double max_dist, uint32_t *label)
{
    for (uint32_t i = 0; i < n; ++i) label[i] = i;
    for (uint32_t t = 0; t + 1 < n && dist[t] <= max_dist; ++t) cluster_union(label, merge_a[t], merge_b[t]);
    uint32_t roots = 0;
    for (uint32_t i = 0; i < n; ++i) roots += cluster_flatten(label, i) ? 1u : 0u;
    return roots;
}

} // namespace mhx
