// mhx_cluster.h -- the rules of the single-linkage clustering of ONE sketch set (mhx_dist_cluster) that do not depend on how
// a GPU runs them, as host+device functions: the exact integer form of "distance <= max_dist" (the cmin table), the
// lock-free union over a parent array, one memory access per step, and the flatten pass.  The kernels in mhx_cluster.hip
// call these functions; tests/emul/cluster_emul.cpp runs the same text on the CPU, sequentially and interleaved access by
// access.  Pairs, geometry and schedule are the triangle's (mhx_triangle.h).
#pragma once
#include "mhx_triangle.h"

namespace mhx {

// ---- the edge rule ----------------------------------------------------------------------------------------------------------
// Lists i and j are neighbours iff tri_distance(common, denom, k) <= max_dist in HOST libm doubles, the rule of
// mhx_dist_triangle_edges' host form.  The device has neither that log nor any use for an approximate prefilter here (a
// wrong edge joins two clusters for good), so the host turns the bound into integers once per call:
//     cmin[d], d = 0 .. s: the smallest c in 0 .. d with tri_distance(c, d, k) <= max_dist, d + 1 when there is none
// and the kernel keeps a pair iff common >= cmin[denom] (denom <= s always).  That is the rule itself as long as the
// distance does not increase with `common`, which tests/test_cluster_rule.py checks value by value.
// The builder takes every entry from its predecessor: the Jaccard index (c + 1) / (d + 1) is not below c / d, so cmin[d] is
// cmin[d - 1] or one more -- it looks there first and walks, in either direction, until the definition holds, whatever the
// rounding does: O(s) evaluations in all (about 3 s of them; 10^6 entries in some tens of milliseconds).
inline bool cluster_is_edge(uint32_t common, uint32_t denom, int k, double max_dist) { return tri_distance(common, denom, k) <= max_dist; }

inline void cluster_cmin_build(uint32_t s, int k, double max_dist, uint32_t *cmin)
{
    uint32_t c = 0;
    for (uint32_t d = 0; d <= s; ++d) {
        if (c > d) c = d;                                                   // (the predecessor had none: d, its own "none", is a candidate here)
        while (c <= d && !cluster_is_edge(c, d, k, max_dist)) ++c;          // up to the first that passes, d + 1: none
        while (c > 0 && c <= d && cluster_is_edge(c - 1, d, k, max_dist)) --c; // and down while the one below passes too
        cmin[d] = c;
    }
}

MHX_HD bool cluster_keep(uint32_t common, uint32_t denom, const uint32_t *cmin, uint32_t s) { return denom <= s && common >= cmin[denom]; }

// ---- access layer -------------------------------------------------------------------------------------------------------------
// Every read and write of `parent` while unions run: agent-scope atomics on the device (a plain load may be served from a
// stale line of another XCD's L2, and a stale parent[x] == x would make the compare-and-swap below fail for ever), plain
// accesses on the host, where one thread of control runs the steps.
MHX_HD uint32_t cluster_load(const uint32_t *p)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
    return *p;
#endif
}
MHX_HD void cluster_store(uint32_t *p, uint32_t v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
    *p = v;
#endif
}
// compare-and-swap: returns what the word held
MHX_HD uint32_t cluster_cas(uint32_t *p, uint32_t expect, uint32_t v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return atomicCAS(p, expect, v);
#else
    const uint32_t old = *p;
    if (old == expect) *p = v;
    return old;
#endif
}

// ---- union ----------------------------------------------------------------------------------------------------------------
// parent[x] == x marks a root.  A union finds the roots of both ends and hooks the HIGHER root under the lower one with one
// compare-and-swap that succeeds only while the higher one still is a root:
//   - only a root is ever hooked, always under a smaller index: parent[x] <= x throughout, no cycles, and the root of a
//     finished component is its lowest index -- the label, whatever order the pairs arrive in;
//   - a step never waits for another thread: a failed compare-and-swap means somebody else hooked that root in the
//     meantime (one of at most n - 1 hooks of the whole call), and the union goes on from the two nodes it holds, which
//     still belong to the components of its ends.
// One step is ONE access to `parent`, so that the emulator can interleave the steps of many unions in any order.
struct ClusterUnion {
    uint32_t a, b;   // a node of each end's component, walking up
    uint32_t phase;  // 0: a walks, 1: b walks, 2: both are roots (as last seen), hook
    uint32_t retries;
};
MHX_HD ClusterUnion cluster_union_begin(uint32_t i, uint32_t j) { return ClusterUnion{i, j, 0u, 0u}; }
// true: the union is done (both ends are in one component)
MHX_HD bool cluster_union_step(uint32_t *parent, ClusterUnion &u)
{
    if (u.a == u.b) return true;
    if (u.phase == 0) {
        const uint32_t p = cluster_load(parent + u.a);
        if (p == u.a) u.phase = 1; else u.a = p;
        return u.a == u.b;
    }
    if (u.phase == 1) {
        const uint32_t p = cluster_load(parent + u.b);
        if (p == u.b) u.phase = 2; else u.b = p;
        return u.a == u.b;
    }
    const uint32_t hi = u.a > u.b ? u.a : u.b, lo = u.a > u.b ? u.b : u.a;
    if (cluster_cas(parent + hi, hi, lo) == hi) return true;
    ++u.retries;
    u.phase = 0;
    return false;
}
MHX_HD void cluster_union(uint32_t *parent, uint32_t i, uint32_t j)
{
    ClusterUnion u = cluster_union_begin(i, j);
    while (!cluster_union_step(parent, u)) {}
}

// ---- flatten ----------------------------------------------------------------------------------------------------------------
MHX_HD uint32_t cluster_find(const uint32_t *parent, uint32_t x)
{
    for (;;) {
        const uint32_t p = cluster_load(parent + x);
        if (p == x) return x;
        x = p;
    }
}
// work item i of n, no union running: parent[i] = its root (others may store theirs meanwhile: every value a walk meets is
// an ancestor, and the roots do not move).  True when i is a root -- after the last block these are the clusters.
MHX_HD bool cluster_flatten(uint32_t *parent, uint32_t i)
{
    const uint32_t root = cluster_find(parent, i);
    if (root != i) cluster_store(parent + i, root);
    return root == i;
}

} // namespace mhx
