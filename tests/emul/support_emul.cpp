// tests/emul/support_emul.cpp -- CPU emulator of the support kernels (mhx_support.hip, test tool).  Runs the host+device
// functions of auriclass_amd/csrc/mhx_support.h themselves, phase by phase as a workgroup of `waves` waves of 64 lanes runs
// them: the kept counts of a list from the waves' contiguous shares, s_r folded over the lists of a set, and for a pair the
// merge-path shares, walk 1 (u of every share), the totals that go through LDS and give every wave its start, walk 2 (c while
// u <= s_r, a wave leaves when all its lanes stand at their s_r) and the sum of the waves' c.  The number of waves is the
// caller's, so that a test can put a share's border wherever it likes.  The waves and lanes of a phase run in descending order:
// nothing in a phase may depend on the order.  Not part of the product; built by tests/test_support_emulation.py with g++.
#include <cstdint>
#include <vector>
#include "../../auriclass_amd/csrc/mhx_support.h"

using namespace mhx;

extern "C" int emul_support_keeps(uint64_t h, uint64_t seed, uint32_t r, uint64_t T) { return support_keeps(h, support_lane_const(seed, r), T) ? 1 : 0; }
extern "C" int emul_resample_keeps(uint64_t h, uint64_t seed, uint32_t r, uint64_t T) { return resample_keeps(h, seed, r, T) ? 1 : 0; }
extern "C" uint32_t emul_support_threads() { return kSupportThreads; }
extern "C" uint32_t emul_support_batch(uint32_t top, uint32_t replicates, uint64_t limit) { return support_batch(top, replicates, limit); }
extern "C" uint64_t emul_support_query_bytes(uint32_t top, uint32_t replicates) { return support_query_bytes(top, replicates); }

// the shares of a pair: d[2 w], d[2 w + 1] the merged positions of wave w, ij[4 w ..] its i, i1, j, j1
extern "C" void emul_support_shares(const uint64_t *A, uint32_t nA, const uint64_t *B, uint32_t nB, uint32_t waves, uint32_t *d, uint32_t *ij)
{
    for (uint32_t w = 0; w < waves; ++w) {
        support_share(nA + nB, waves, w, &d[2 * w], &d[2 * w + 1]);
        const SupportWalk x = support_walk_begin(A, nA, B, nB, waves, w);
        ij[4 * w] = x.i; ij[4 * w + 1] = x.i1; ij[4 * w + 2] = x.j; ij[4 * w + 3] = x.j1;
    }
}

// support_count_kernel for one (list, group): kept[lane] of the lanes below `replicates`, the others untouched
extern "C" void emul_support_count(const uint64_t *row, uint32_t len, uint32_t waves, uint32_t group, uint32_t replicates, uint64_t seed, uint64_t T, uint32_t *kept)
{
    std::vector<uint32_t> wave_kept((size_t)waves * 64);
    for (uint32_t w = waves; w-- > 0;)
        for (uint32_t lane = 64; lane-- > 0;) {
            uint32_t j0, j1, n = 0;
            support_share(len, waves, w, &j0, &j1);
            const uint64_t lane_const = support_lane_const(seed, group * 64u + lane);
            for (uint32_t j = j0; j < j1; ++j) support_step_count(n, support_keeps(row[j], lane_const, T));
            wave_kept[(size_t)w * 64 + lane] = n;
        }
    for (uint32_t lane = 64; lane-- > 0;) { // behind the barrier: wave 0
        if (group * 64u + lane >= replicates) continue;
        uint32_t all = 0;
        for (uint32_t w = 0; w < waves; ++w) all += wave_kept[(size_t)w * 64 + lane];
        kept[lane] = all;
    }
}

// support_s_kernel for one replicate: len [n] and kept [n] of the lists of its set
extern "C" uint32_t emul_support_s(const uint32_t *len, const uint32_t *kept, uint32_t n, uint32_t s)
{
    uint32_t s_r = s;
    for (uint32_t i = 0; i < n; ++i) s_r = support_fold_s(s_r, len[i], s, kept[i]);
    return s_r;
}

// support_pair_kernel for one (pair, group): A the reference, B the query, s_r [64] per lane as the kernel holds it (0 for a
// lane beyond the replicates); common [64], denom [64] of the lanes below `replicates`, the others untouched.  Returns the
// number of steps of walk 2 that all waves took together (a wave that leaves early takes fewer).
extern "C" uint64_t emul_support_pair(const uint64_t *A, uint32_t nA, const uint64_t *B, uint32_t nB, uint32_t waves, uint32_t group, uint32_t replicates,
                                      uint64_t seed, uint64_t T, const uint32_t *s_r_in, uint32_t *common, uint32_t *denom)
{
    std::vector<uint32_t> wave_count((size_t)waves * 64), start((size_t)waves * 64), u_all(64, 0);
    uint32_t s_r[64];
    uint64_t lane_const[64];
    for (uint32_t lane = 0; lane < 64; ++lane) {
        const uint32_t r = group * 64u + lane;
        s_r[lane] = r < replicates ? s_r_in[lane] : 0u;
        lane_const[lane] = support_lane_const(seed, r);
    }
    uint64_t v;
    bool counts, shared;
    for (uint32_t w = waves; w-- > 0;) // walk 1
        for (uint32_t lane = 64; lane-- > 0;) {
            uint32_t u = 0;
            for (SupportWalk x = support_walk_begin(A, nA, B, nB, waves, w); support_walk_next(x, &v, &counts, &shared);)
                if (counts) support_step_count(u, support_keeps(v, lane_const[lane], T));
            wave_count[(size_t)w * 64 + lane] = u;
        }
    for (uint32_t w = waves; w-- > 0;) // behind the barrier: every wave reads the totals
        for (uint32_t lane = 64; lane-- > 0;) {
            uint32_t before = 0, all = 0;
            for (uint32_t x = 0; x < waves; ++x) {
                if (x < w) before += wave_count[(size_t)x * 64 + lane];
                all += wave_count[(size_t)x * 64 + lane];
            }
            start[(size_t)w * 64 + lane] = before;
            u_all[lane] = all;
        }
    uint64_t steps = 0;
    for (uint32_t w = waves; w-- > 0;) { // walk 2, behind the second barrier: the lanes of a wave step together
        uint32_t u[64], c[64] = {};
        for (uint32_t lane = 0; lane < 64; ++lane) u[lane] = start[(size_t)w * 64 + lane];
        SupportWalk x = support_walk_begin(A, nA, B, nB, waves, w);
        for (;;) {
            bool all_done = true; // __all(u >= s_r)
            for (uint32_t lane = 0; lane < 64; ++lane) all_done = all_done && u[lane] >= s_r[lane];
            if (all_done || !support_walk_next(x, &v, &counts, &shared)) break;
            ++steps;
            if (!counts) continue;
            for (uint32_t lane = 64; lane-- > 0;) support_step(u[lane], c[lane], support_keeps(v, lane_const[lane], T), shared, s_r[lane]);
        }
        for (uint32_t lane = 0; lane < 64; ++lane) wave_count[(size_t)w * 64 + lane] = c[lane];
    }
    for (uint32_t lane = 64; lane-- > 0;) { // behind the third barrier: wave 0
        if (group * 64u + lane >= replicates) continue;
        uint32_t sum = 0;
        for (uint32_t w = 0; w < waves; ++w) sum += wave_count[(size_t)w * 64 + lane];
        common[lane] = sum;
        denom[lane] = support_denom(u_all[lane], s_r[lane]);
    }
    return steps;
}

// support_best_kernel for one (query, replicate): the position of the best of n candidates (ref, common, denom), n >= 1
extern "C" uint32_t emul_support_best(const uint32_t *ref, const uint32_t *common, const uint32_t *denom, uint32_t n)
{
    uint32_t bi = 0;
    for (uint32_t i = 1; i < n; ++i)
        if (support_better(common[i], denom[i], ref[i], common[bi], denom[bi], ref[bi])) bi = i;
    return bi;
}
