// mhx_contain_search.h -- the rules of the containment search (mhx_dist_contain_search: for every query the `top` references
// it holds the largest share of) that do not depend on how a GPU runs them, as host+device functions: the exact order of two
// pairs by shared / n_ref, the insertion that keeps a query's best list sorted, the hit test against the need[] table, and
// the host function that turns the identity bound into that table.  The take-out kernel of mhx_contain_search.hip does
// wave-wide what contain_insert does one candidate after the other; tests/emul/contain_search_emul.cpp runs these functions
// sequentially on the CPU.  The three integers of a pair are mhx_contain.h's, the schedule is the search's (mhx_search.h:
// search_blocks, search_block).  The rule is restated in tests/contain_search_rule.py.
#pragma once
#include <math.h>

#include "mhx_contain.h"
#include "mhx_search.h"

namespace mhx {

struct ContainHit { uint32_t ref, shared, n_ref, n_qry; };

// ---- the order ----------------------------------------------------------------------------------------------------------
// a is better than b: the larger share shared / n_ref, compared exactly as a cross product in 64 bits (both factors are
// below 2^32); equal shares go by the larger `shared` (200/200 before 3/3: more evidence first), equal `shared` by the lower
// reference.  References are distinct, so this is a total order and a best list does not depend on the order in which its
// candidates arrive.  (A hit has n_ref >= shared >= 1; pairs with n_ref == 0 never get here.)
MHX_HD bool contain_better(const ContainHit &a, const ContainHit &b)
{
    const uint64_t l = (uint64_t)a.shared * b.n_ref, r = (uint64_t)b.shared * a.n_ref;
    if (l != r) return l > r;
    return a.shared != b.shared ? a.shared > b.shared : a.ref < b.ref;
}

// list[0 .. n) is sorted best first and holds at most `top` entries: put `cand` in its place, drop the last entry when the
// list is full; returns the new n.  A full list costs a candidate that is not better than its last entry one comparison.
MHX_HD uint32_t contain_insert(ContainHit *list, uint32_t n, uint32_t top, const ContainHit &cand)
{
    if (n == top && !contain_better(cand, list[top - 1])) return n;
    uint32_t pos = 0;
    while (pos < n && contain_better(list[pos], cand)) ++pos;
    const uint32_t last = n < top ? n : top - 1;
    for (uint32_t i = last; i > pos; --i) list[i] = list[i - 1];
    list[pos] = cand;
    return n < top ? n + 1 : top;
}

// ---- the hit rule -------------------------------------------------------------------------------------------------------
// A pair is a hit iff shared >= min_shared (>= 1) and identity(shared, n_ref, k) >= min_identity in HOST libm doubles, the
// identity as mhx_contain_files prints it (mhx_screen_identity: the same expression).  The device has neither that pow nor
// any use for an approximation (the result is promised exact), so the host turns the bound into integers once per call:
//     need[n], n = 0 .. limit: the least `shared` that is a hit at n_ref = n, n + 1 when there is none
// with limit = min(stride, s_r), which no n_ref exceeds, and the kernel keeps a pair iff shared >= need[n_ref].  An entry that
// is not n + 1 is never below min_shared; need[0] is 1, so a pair that shares nothing is never a hit.  That is the rule itself
// as long as the identity does not fall when `shared` rises, which tests/test_contain_search_rule.py checks value by value.
inline double contain_identity(uint32_t shared, uint32_t n_ref, int k)
{
    if (shared == n_ref) return 1.0;
    if (shared == 0) return 0.0;
    return pow((double)shared / (double)n_ref, 1.0 / (double)k);
}
inline bool contain_is_hit(uint32_t shared, uint32_t n_ref, int k, double min_identity, uint32_t min_shared)
{
    return shared >= min_shared && shared <= n_ref && contain_identity(shared, n_ref, k) >= min_identity; // min_shared >= 1
}
// need[0 .. limit].  Every entry starts from its predecessor -- the least share that passes is the same for every n, so
// need[n] is need[n - 1] or a little more -- and walks, in either direction, until the definition holds: O(limit) evaluations
// of pow.  The two bounds that need none take none: at min_identity <= 0 every identity passes (it is never negative) and
// the floor alone decides, above 1 nothing passes.
inline void contain_need_build(uint32_t limit, int k, double min_identity, uint32_t min_shared, uint32_t *need)
{
    const uint32_t floor = min_shared < 1 ? 1u : min_shared;
    if (min_identity <= 0.0 || min_identity > 1.0) {
        for (uint32_t n = 0; n <= limit; ++n) need[n] = min_identity <= 0.0 && floor <= n ? floor : n + 1;
        return;
    }
    uint32_t c = floor;
    for (uint32_t n = 0; n <= limit; ++n) {
        if (floor > n) { need[n] = n + 1; continue; }
        if (c > n) c = n;          // (the predecessor had none: n, its own "none", is a candidate here)
        if (c < floor) c = floor;
        while (c <= n && !contain_is_hit(c, n, k, min_identity, floor)) ++c;             // up to the first that passes, n + 1: none
        while (c > floor && c <= n && contain_is_hit(c - 1, n, k, min_identity, floor)) --c; // and down while the one below passes too
        need[n] = c;
    }
}
MHX_HD bool contain_keep(uint32_t shared, uint32_t n_ref, const uint32_t *need, uint32_t limit) { return n_ref <= limit && shared >= need[n_ref]; }

} // namespace mhx
