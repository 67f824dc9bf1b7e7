// mhx_mst.h -- the rules of the single-linkage TREE of ONE sketch set (mhx_dist_mst: the minimum spanning tree of the
// distance graph, Boruvka on the device) that do not depend on how a GPU runs them, as host+device functions: the order of
// the edges, the packed "best edge of a vertex" word and the proposal to it, the choice of a component's vertex, the hook
// of a component and the cut of the finished tree at a distance.  The kernels in mhx_mst.hip call these functions;
// tests/emul/mst_emul.cpp runs the same text on the CPU, sequentially and interleaved access by access.  Pairs, geometry and
// schedule are the triangle's (mhx_triangle.h), the union-find and its access layer the clustering's (mhx_cluster.h).
//
// Every pair j < i of the set is an edge of the graph, so the tree spans the set and no distance bound applies.  Memory:
// best [n] 64-bit words, winner / parent / comp [n] 32-bit words and the n - 1 edges of the result.  The STORED pair source
// (mhx_engine_triangle.cpp: when 8 n (n - 1) / 2 bytes fit MHX_MST_STORE_MB) additionally holds the packed common / denom of
// mhx_dist_triangle's dense mode -- the one place where this call holds something of size n^2; the RECOMPUTED source runs
// the triangle's blocks again every round and holds O(n).
#pragma once
#include "mhx_cluster.h"

namespace mhx {

// ---- the edge order ---------------------------------------------------------------------------------------------------------
// Edge a precedes edge b iff its Jaccard index common / denom is greater, compared exactly as a cross product in 64 bits
// (search_better's comparison: common == denom counts as 1/1, which gives 0/0 -- two empty lists -- its place at the top);
// equal indices (1/2 and 2/4) go by the lower lo = min(i, j), then by the lower hi.  Edges are distinct pairs, so the order
// is total and strict and the minimum spanning tree is unique: Kruskal over the edges in this order.
// Seen from one vertex v, whose edges all have v as one end, "(lo, hi) ascending" is "the lower OTHER end": for other ends
// x < y the pairs are (v, x) < (v, y) when v < x, (x, v) < (v, y) when x < v < y, and (x, v) < (y, v) when y < v.
struct MstEdge { uint32_t common, denom, lo, hi; };

MHX_HD int mst_index_cmp(uint32_t a_common, uint32_t a_denom, uint32_t b_common, uint32_t b_denom) // > 0: a's index is greater
{
    const uint64_t ac = a_common == a_denom ? 1u : a_common, ad = a_common == a_denom ? 1u : a_denom;
    const uint64_t bc = b_common == b_denom ? 1u : b_common, bd = b_common == b_denom ? 1u : b_denom;
    const uint64_t l = ac * bd, r = bc * ad;
    return l > r ? 1 : (l < r ? -1 : 0);
}
MHX_HD bool mst_precedes(const MstEdge &a, const MstEdge &b)
{
    const int c = mst_index_cmp(a.common, a.denom, b.common, b.denom);
    if (c != 0) return c > 0;
    return a.lo != b.lo ? a.lo < b.lo : a.hi < b.hi;
}
MHX_HD MstEdge mst_edge(uint32_t common, uint32_t denom, uint32_t u, uint32_t v) { return MstEdge{common, denom, u < v ? u : v, u < v ? v : u}; }

// ---- best[v]: the best outgoing edge of vertex v, one 64-bit word ---------------------------------------------------------------
// bit 56: valid; bits 36 .. 55: common; bits 16 .. 35: denom; bits 0 .. 15: the other end.  Hence the limits of the call:
// s < 2^20 (common <= denom <= s) and n <= 65 536 (kTriMaxLists).  0 is "empty".
// Built: the compare-and-swap loop, not an order-preserving integer key with one atomicMax.  Such a key would have to be
// injective on the fractions that occur and still carry (common, denom) of the winner: 40 bits of (common, denom) do not
// sort by common / denom, and a fixed-point quotient in front of them needs 40 bits itself to tell fractions with denominators
// below 2^20 apart (they differ by 2^-40 and more), which leaves no room for them and the other end in one 64-bit word.
constexpr uint32_t kMstMaxS = 1u << 20;      // s must be below
constexpr uint32_t kMstNobody = 0xFFFFFFFFu; // winner[c]: no vertex of component c has proposed
constexpr uint64_t kMstValid = 1ull << 56;

MHX_HD uint64_t mst_pack(uint32_t common, uint32_t denom, uint32_t other) { return kMstValid | (uint64_t)common << 36 | (uint64_t)denom << 16 | other; }
MHX_HD bool mst_valid(uint64_t w) { return (w & kMstValid) != 0; }
MHX_HD uint32_t mst_common(uint64_t w) { return (uint32_t)(w >> 36) & 0xFFFFFu; }
MHX_HD uint32_t mst_denom(uint64_t w) { return (uint32_t)(w >> 16) & 0xFFFFFu; }
MHX_HD uint32_t mst_other(uint64_t w) { return (uint32_t)w & 0xFFFFu; }
// two words of the SAME vertex: a precedes b (an empty word precedes nothing, a valid one precedes the empty one)
MHX_HD bool mst_word_precedes(uint64_t a, uint64_t b)
{
    if (!mst_valid(a)) return false;
    if (!mst_valid(b)) return true;
    const int c = mst_index_cmp(mst_common(a), mst_denom(a), mst_common(b), mst_denom(b));
    return c != 0 ? c > 0 : mst_other(a) < mst_other(b);
}
// what the lanes of a wave that share a vertex reduce with before they touch memory
MHX_HD uint64_t mst_word_better(uint64_t a, uint64_t b) { return mst_word_precedes(b, a) ? b : a; }

// ---- access layer (64-bit words; the 32-bit ones are mhx_cluster.h's) ---------------------------------------------------------
MHX_HD uint64_t mst_load64(const uint64_t *p)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
    return *p;
#endif
}
MHX_HD uint64_t mst_cas64(uint64_t *p, uint64_t expect, uint64_t v) // returns what the word held
{
#if defined(__HIP_DEVICE_COMPILE__)
    return (uint64_t)atomicCAS((unsigned long long *)p, (unsigned long long)expect, (unsigned long long)v);
#else
    const uint64_t old = *p;
    if (old == expect) *p = v;
    return old;
#endif
}

// ---- step 2, propose --------------------------------------------------------------------------------------------------------
// A pair (i, j) that counts and whose ends lie in different components (comp: the flattened parent of the round before,
// read-only in this step, plain loads) proposes twice: (common, denom, j) to best[i] and (common, denom, i) to best[j].
// A proposal is a relaxed agent-scope load and a compare-and-swap loop that swaps only when the proposal precedes what the
// word holds:
//   - a word only ever changes to one that precedes it, so what a finished step leaves is the first proposal of all, whatever
//     order they arrive in;
//   - a step never waits for another thread: a failed compare-and-swap means somebody else improved the word in the meantime
//     (each of the proposals of a round improves a word at most once), and the loop goes on from the value the swap returned,
//     which it either still precedes or not.
// One step is ONE access to `best`, so that the emulator can interleave the steps of many proposals in any order.
struct MstPropose {
    uint64_t word, seen;
    uint32_t v;
    uint32_t phase; // 0: load, 1: swap
    uint32_t retries;
};
MHX_HD MstPropose mst_propose_begin(uint32_t v, uint64_t word) { return MstPropose{word, 0, v, 0u, 0u}; }
// true: the proposal is done (best[v] holds it or something that precedes it)
MHX_HD bool mst_propose_step(uint64_t *best, MstPropose &p)
{
    if (p.phase == 0) {
        p.seen = mst_load64(best + p.v);
        p.phase = 1;
        return !mst_word_precedes(p.word, p.seen);
    }
    const uint64_t old = mst_cas64(best + p.v, p.seen, p.word);
    if (old == p.seen) return true;
    ++p.retries;
    p.seen = old;
    return !mst_word_precedes(p.word, p.seen);
}
MHX_HD void mst_propose(uint64_t *best, uint32_t v, uint64_t word)
{
    MstPropose p = mst_propose_begin(v, word);
    while (!mst_propose_step(best, p)) {}
}

// ---- step 3, choose ---------------------------------------------------------------------------------------------------------
// A vertex v with a valid best[v] proposes itself to winner[comp[v]], a 32-bit word with its own compare-and-swap loop.  Two
// candidates are compared by the edge order of their best entries, which no one writes in this step (plain loads).  Two
// vertices of one component never hold the same edge -- both ends of an outgoing edge lie in different components -- so the
// comparison is strict; the argument that no step waits is the one above.
MHX_HD MstEdge mst_edge_of(const uint64_t *best, uint32_t v)
{
    const uint64_t w = best[v];
    return mst_edge(mst_common(w), mst_denom(w), v, mst_other(w));
}
struct MstChoose {
    uint32_t v, c, seen;
    uint32_t phase; // 0: load, 1: swap
    uint32_t retries;
};
MHX_HD MstChoose mst_choose_begin(uint32_t v, uint32_t c) { return MstChoose{v, c, kMstNobody, 0u, 0u}; }
MHX_HD bool mst_choose_wins(const uint64_t *best, uint32_t v, uint32_t seen) { return seen == kMstNobody || mst_precedes(mst_edge_of(best, v), mst_edge_of(best, seen)); }
MHX_HD bool mst_choose_step(uint32_t *winner, const uint64_t *best, MstChoose &x)
{
    if (x.phase == 0) {
        x.seen = cluster_load(winner + x.c);
        x.phase = 1;
        return !mst_choose_wins(best, x.v, x.seen);
    }
    const uint32_t old = cluster_cas(winner + x.c, x.seen, x.v);
    if (old == x.seen) return true;
    ++x.retries;
    x.seen = old;
    return !mst_choose_wins(best, x.v, x.seen);
}
MHX_HD void mst_choose(uint32_t *winner, const uint64_t *best, uint32_t v, uint32_t c)
{
    MstChoose x = mst_choose_begin(v, c);
    while (!mst_choose_step(winner, best, x)) {}
}

// ---- step 4, hook -----------------------------------------------------------------------------------------------------------
// Root a with a winner v takes v's edge e = (v, u) into the component of root b = comp[u].  best, winner and comp are not
// written in this step (comp is a COPY of the flattened parent, because the unions of this step move the roots of parent).
// The edge is appended to the result unless b's winner holds the same unordered pair and b < a: in a mutual pick the lower
// root appends.  Under a strict total order the mutual picks are the only cycles among the picks of a round -- along any
// other cycle every pick would have to precede the one before it --, so the appended edges of a round are as many as the
// components it loses, which the host asserts from the two counters.  cluster_union(parent, v, u) runs for every pick.
struct MstHook {
    bool picks;   // a is a root with a winner
    bool appends; // ... and its edge goes to the result
    uint32_t v, u; // the ends of the pick: v in a's component
    uint32_t common, denom;
};
MHX_HD MstHook mst_hook(const uint32_t *comp, const uint32_t *winner, const uint64_t *best, uint32_t a)
{
    MstHook h{false, false, 0u, 0u, 0u, 0u};
    if (comp[a] != a) return h;
    const uint32_t v = winner[a];
    if (v == kMstNobody) return h;
    const uint64_t w = best[v];
    h.picks = true;
    h.v = v; h.u = mst_other(w);
    h.common = mst_common(w); h.denom = mst_denom(w);
    const uint32_t b = comp[h.u], v2 = winner[b];
    const bool mutual = v2 == h.u && mst_other(best[v2]) == v; // (b has an outgoing edge -- this one --, so it has a winner, and v2 == u is a list)
    h.appends = !(mutual && b < a);
    return h;
}

// ---- the cut ----------------------------------------------------------------------------------------------------------------
// The clusters of mhx_dist_cluster at max_dist from the tree alone: a union-find over the tree edges that are edges of the
// clustering (cluster_is_edge: the HOST libm distance <= max_dist), label = the lowest index of the component.  Equal to
// mhx_dist_cluster's labels wherever the libm distance does not increase along the edge order, which
// tests/test_mst_rule.py checks fraction by fraction.  Host only: exported as mhx_mst_labels, which engine.mst_labels calls.
inline uint32_t mst_labels(const uint32_t *edge_i, const uint32_t *edge_j, const uint32_t *common, const uint32_t *denom, uint32_t n, int k,
                           double max_dist, uint32_t *label)
{
    for (uint32_t i = 0; i < n; ++i) label[i] = i;
    for (uint32_t e = 0; e + 1 < n; ++e)
        if (cluster_is_edge(common[e], denom[e], k, max_dist)) cluster_union(label, edge_i[e], edge_j[e]);
    uint32_t roots = 0;
    for (uint32_t i = 0; i < n; ++i) roots += cluster_flatten(label, i) ? 1u : 0u;
    return roots;
}

// rounds a call may take: the components at least halve per round, one more for good measure
MHX_HD uint32_t mst_max_rounds(uint32_t n)
{
    uint32_t r = 0;
    while ((1ull << r) < n) ++r;
    return r + 1;
}

} // namespace mhx
