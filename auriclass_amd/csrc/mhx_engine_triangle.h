// mhx_engine_triangle.h -- what the host side of the tree (mhx_engine_mst.cpp) takes from the triangle's
// (mhx_engine_triangle.cpp): the inputs of a call and their staging, the dense mode as the stored pair source, and the
// blocks run once per round as the recomputed one; and what the calls that keep the dense mode's result share (the linkage,
// neighbour joining and its jackknife too): budget, owner and clock of the stored triangle.  Internal.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "mhx_mst.h"
#include "mhx_engine_sets.h"
#include "mhx_internal.h"

namespace mhx {

struct TriCall { // the inputs of a call, everything on the device
    const uint64_t *rows;
    const uint32_t *len;
    uint32_t n, stride, s, longest;
    int k;
};

// what all calls check first; *done: nothing to compute (n <= 1)
int triangle_check(const uint64_t *rows, const uint32_t *len, uint32_t n, uint32_t stride, int k, uint32_t s, int device_ptrs, bool *done);
// the inputs of a call and the regions `in` of the staging area, which the caller has declared, at *base, see there
int stage_rows(const uint64_t *rows, const uint32_t *len, uint32_t n, uint32_t stride, int k, uint32_t s, int device_ptrs, Carve in, uint8_t **base, TriCall &c);
// the dense mode: every pair into the packed triangle [n (n - 1) / 2]; dist may be null
int run_dense(const TriCall &c, uint32_t *common, uint32_t *denom, double *dist);

// ---- the stored triangle: what the calls that keep the dense mode's result share (the tree when stored, the linkage,
// neighbour joining and its jackknife)
// the budget of such a call in MB: `env` (MHX_MST_STORE_MB, MHX_LINKAGE_STORE_MB), 4096 without it
inline uint64_t store_budget_mb(const char *env)
{
    uint64_t budget_mb = 4096;
    if (const char *e = getenv(env)) { const long long v = atoll(e); if (v >= 0) budget_mb = (uint64_t)v; }
    return budget_mb;
}
// the pair words of n lists, 8 bytes a pair, against that budget
inline int store_fits(const char *env, uint32_t n)
{
    const uint64_t pairs = (uint64_t)n * (n - 1) / 2, budget_mb = store_budget_mb(env);
    if (8 * pairs > budget_mb << 20)
        return fail(MHX_E_CAPACITY, "the pair words of %u lists (%llu bytes) do not fit %s = %llu", n, (unsigned long long)(8 * pairs), env, (unsigned long long)budget_mb);
    return MHX_OK;
}
// The owner of the packed triangle, common and denom [pairs] each in one allocation, and of the pair words [pairs] of the calls
// that have them; released when the call returns, the triangle by reset() already (behind an init pass that has read it).
struct StoredTriangle {
    DevArray<uint64_t> words;
    DevArray<uint8_t> packed;
    uint32_t *common = nullptr, *denom = nullptr;
    int alloc(uint64_t pairs, const char *of, bool pair_words) // of: the call in the messages, "the linkage"
    {
        if (pair_words && words.grow(pairs, g.stream) != hipSuccess)
            return fail(MHX_E_HIP, "hipMalloc failed for the pair words of %s (%llu bytes)", of, (unsigned long long)(8 * pairs));
        const size_t bp = up256((size_t)pairs * 4);
        if (packed.grow(2 * bp, g.stream) != hipSuccess) return fail(MHX_E_HIP, "hipMalloc failed for the stored pairs of %s (%zu bytes)", of, 2 * bp);
        common = (uint32_t *)(uint8_t *)packed; denom = (uint32_t *)((uint8_t *)packed + bp);
        return MHX_OK;
    }
    void reset() { packed.reset(); common = denom = nullptr; }
};
// The clock of the steps that follow run_dense: started behind it, stop() behind the last launch, note() after the device is
// done -- g.last_dist_ms is then the triangle plus the steps.
struct StepsClock {
    const double tri_ms = g.last_dist_ms;
    StepsClock() { hipEventRecord(g.ev0, g.stream); }
    void stop() { hipEventRecord(g.ev1, g.stream); }
    void note()
    {
        float ms = 0.f;
        hipEventElapsedTime(&ms, g.ev0, g.ev1);
        g.last_dist_ms = tri_ms + ms;
    }
};

// The medoid mode (mhx_medoid.h), everything on the device but h_label, the host's copy of label, which it has checked: the
// blocks that hold a pair of one cluster add to sum [n], the pick writes medoid [n] through best [n], and with common / denom
// (both or neither) the pair kernel compares every list with its medoid.  n >= 1; n == 1 runs no block.
struct MedoidRun {
    const uint32_t *h_label, *label;
    unsigned long long *sum, *best;
    uint32_t *medoid, *common, *denom;
};
int run_medoid(const TriCall &c, const MedoidRun &m);

// The state of a single-linkage tree call (mhx_mst.h) between its rounds, everything on the device: what the five steps of
// a round read and write, and the counters that come back once per round.
struct MstRun {
    uint64_t *best; // [n]
    uint32_t *winner, *parent, *comp; // [n] each
    unsigned long long *counters; // [0] edges appended so far, [1] roots of the last flatten pass
    uint32_t *edge_i, *edge_j, *common, *denom; // [n - 1] the result
    double *dist;             // may be null
    uint32_t n;
    int k;
    uint32_t components, rounds; // host: after the last round closed
    uint64_t appended;
};

hipError_t mst_round_open(MstRun &m); // step 1; the proposals of step 2 follow, from either pair source
int mst_round_close(MstRun &m);       // steps 3 to 5 and the one small readback of a round

// The rounds of a tree until one component is left (mst_max_rounds bounds them): a round opens, `propose(round)` runs step 2
// from its pair source, the round closes.  Nothing synchronises between the rounds but mst_round_close.  le: the first
// launch error, the caller's to report; nothing is launched after it.
template <class Propose> int mst_rounds(MstRun &m, hipError_t &le, Propose propose)
{
    for (uint32_t round = 0; le == hipSuccess && m.components > 1; ++round) {
        if (round == mst_max_rounds(m.n)) return fail(MHX_E_INTERNAL, "the tree is not finished after %u rounds (%u components)", round, m.components);
        le = mst_round_open(m);
        int rc = le == hipSuccess ? propose(round) : MHX_OK;
        if (rc == MHX_OK && le == hipSuccess) rc = mst_round_close(m);
        if (rc) return rc;
    }
    return MHX_OK;
}

// the tree from the recomputed pair source: every round's proposals from the triangle's blocks.  The caller has run mst_begin.
int run_mst_recomputed(const TriCall &c, MstRun &m);

} // namespace mhx
