// mhx_engine_contain.cpp -- host side of the containment of reference sketches in query sketches (mhx_dist_contain): what it
// gives the schedule and the staging of mhx_engine_sets.h -- its geometry, the bounds and effective lengths of every list, a
// finish pass and a pair kernel that write straight into the outputs.
// Rules: mhx_contain.h; kernels: mhx_contain.hip and the passes of mhx_dist.hip.
// The winner-take-all form (mhx_dist_contain_winner) is the same call with two more passes behind the plain one, per query
// batch over all references: the claim pass and the tally (rules: mhx_contain_winner.h; kernels: mhx_contain_winner.hip).
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "mhx_device.h"
#include "mhx_contain_winner.h"
#include "mhx_search.h"
#include "mhx_engine_sets.h"
#include "mhx_internal.h"

using namespace mhx;

namespace mhx {
// The geometry of the range route: the search's (tri_ranges, 16 entries per slice) up to kDistRanges, and kDistRanges itself
// as far as the base form of the distance path goes (65 536 entries).  Longer lists have none here: the windowed form is
// not built, the pair kernel takes them.  MHX_SEARCH_GEOMETRY=dist takes kDistRanges from the first entry on, as the search.
// (The containment search, mhx_engine_contain_search.cpp, takes its geometry here too.)
uint32_t contain_ranges(uint32_t longest)
{
    const char *geo = getenv("MHX_SEARCH_GEOMETRY");
    const uint32_t R = geo && strcmp(geo, "dist") == 0 ? 0u : tri_ranges(longest);
    if (R != 0 && R <= (uint32_t)kDistRanges) return R;
    return dist_windows(longest) == 1 ? (uint32_t)kDistRanges : 0u;
}
} // namespace mhx

namespace {

struct ContainCall { // everything on the device
    const uint64_t *q, *r;
    const uint32_t *q_len, *r_len;
    uint32_t nq, nr, stride, s_q, s_r, longest;
    uint32_t *shared, *n_qry, *n_ref;
    uint32_t *won = nullptr;              // winner-take-all: [nq][nr], and the passes behind the plain one run
    const uint64_t *ref_length = nullptr; // [nr] genome lengths or null (with `won` only)
};

// Launches the whole call on the engine's stream and waits for it, on the schedule of mhx_engine_sets.h: the finish pass and
// the pair kernel write straight into the outputs, so there is nothing to take out.
int contain_device(ContainCall &c)
{
    const uint64_t pairs = (uint64_t)c.nq * c.nr;
    SetSchedule sch(c.nq, c.nr, c.stride, SetGeometry{contain_ranges(c.longest), c.longest, "MHX_SEARCH_QBATCH", c.nq, "containment"});
    // the bounds and effective lengths of both sets
    const size_t o_bq = sch.extra((size_t)c.nq * 8), o_br = sch.extra((size_t)c.nr * 8), o_eq = sch.extra((size_t)c.nq * 4), o_er = sch.extra((size_t)c.nr * 4);
    // winner-take-all: a winner word per (query of a batch, position in its list), and the counter of the pairs walked
    const uint32_t width = std::min(c.stride, c.s_q);
    const size_t o_win = sch.extra(c.won ? (size_t)sch.qbatch * width * 4 : 0), o_count = sch.extra(c.won ? 256 : 0);
    int rc = sch.place("the containment workspace");
    if (rc) return rc;
    hipError_t &le = sch.le;
    ContainArgs all{};
    all.q = c.q; all.q_len = c.q_len; all.nq = c.nq; all.r = c.r; all.r_len = c.r_len; all.nr = c.nr; all.stride = c.stride; all.s_q = c.s_q; all.s_r = c.s_r;
    all.q_bound = (uint64_t *)sch.at(o_bq); all.r_bound = (uint64_t *)sch.at(o_br);
    all.q_eff = (uint32_t *)sch.at(o_eq); all.r_eff = (uint32_t *)sch.at(o_er);
    all.shift = sch.words;
    all.shared = c.shared; all.n_qry = c.n_qry; all.n_ref = c.n_ref; all.out_stride = c.nr;
    auto block_args = [&](const SearchBlock &b) {
        ContainArgs x = all;
        x.q0 = b.q0; x.bnq = b.nq; x.r0 = b.r0; x.bnr = b.nr;
        return x;
    };
    // the passes of mhx_dist.hip see the effective lengths: what lies behind them in a row is not part of a list.  They read
    // neither s nor k.
    DistArgs lists{};
    lists.q = c.q; lists.q_len = all.q_eff; lists.nq = c.nq; lists.r = c.r; lists.r_len = all.r_eff; lists.nr = c.nr; lists.stride = c.stride;
    sch.begin();
    if (le == hipSuccess) le = launch_contain_bounds(all, g.stream);
    sch.offsets(lists);
    rc = sch.run(
        0, c.nq, [&](const SearchBlock &b, const DistArgs &) { return launch_contain_pairs(block_args(b), g.stream); },
        [&](const SearchBlock &b, const DistArgs &, const DistWork &w) { return launch_contain_finish(block_args(b), w, g.stream); },
        [](const SearchBlock &, const uint32_t *) { return hipSuccess; });
    if (rc) return rc;
    // The plain pass of every block is queued.  Winner-take-all: per query batch, over ALL references, zero the batch's words,
    // let every pair that shares something propose, and count what every reference holds at the end.
    if (c.won && le == hipSuccess) {
        ContainWinnerArgs wa{(uint32_t *)sch.at(o_win), width, c.ref_length, c.won, (unsigned long long *)sch.at(o_count)};
        le = hipMemsetAsync(c.won, 0, (size_t)pairs * 4, g.stream);
        if (le == hipSuccess) le = hipMemsetAsync(wa.pairs, 0, 8, g.stream);
        for (uint32_t q0 = 0; q0 < c.nq && le == hipSuccess; q0 += sch.qbatch) {
            ContainArgs x = all;
            x.q0 = q0; x.bnq = std::min(sch.qbatch, c.nq - q0); x.r0 = 0; x.bnr = c.nr;
            le = hipMemsetAsync(wa.words, 0, (size_t)x.bnq * width * 4, g.stream);
            if (le == hipSuccess) le = launch_contain_claim(x, wa, g.stream);
            if (le == hipSuccess) le = launch_contain_tally(x, wa, g.stream);
        }
    }
    rc = sch.end();
    if (rc == MHX_OK) rc = sch.wait();
    if (rc) return rc;
    if (c.won) {
        unsigned long long walked = 0;
        if (hipMemcpy(&walked, sch.at(o_count), 8, hipMemcpyDeviceToHost) != hipSuccess) return fail(MHX_E_HIP, "D2H copy of the claim pass's counter failed");
        g.last_contain_winner_pairs = walked;
    }
    return MHX_OK;
}

int contain_check(uint32_t s_q, uint32_t s_r, uint32_t stride)
{
    if (s_q == 0 || s_r == 0 || stride == 0) return fail(MHX_E_ARG, "bad s_q / s_r / stride");
    return MHX_OK;
}

} // namespace

namespace mhx {
// Host rows, every one where it lies (q_rows / r_rows: q_len[i] / r_len[i] entries each), staged at `stride`; host outputs.
int contain_rows(const uint64_t *const *q_rows, const uint64_t *q, const uint32_t *q_len, uint32_t nq, uint32_t s_q, const uint64_t *const *r_rows,
                 const uint64_t *r, const uint32_t *r_len, uint32_t nr, uint32_t s_r, uint32_t stride, uint32_t *shared, uint32_t *n_qry, uint32_t *n_ref,
                 const uint64_t *ref_length, uint32_t *won)
{
    const size_t cells = (size_t)nq * nr;
    Carve outs; // the three [nq][nr] outputs, what was won, the genome lengths
    const size_t o_shared = outs.take(cells * 4), o_qry = outs.take(cells * 4), o_ref = outs.take(cells * 4), o_won = outs.take(won ? cells * 4 : 0);
    const size_t o_length = outs.take(won && ref_length ? (size_t)nr * 8 : 0);
    StagedSets in{};
    int rc = stage_sets("dist_contain", HostSet{q, q_rows, q_len, nq}, HostSet{r, r_rows, r_len, nr}, nullptr, stride, outs.bytes, in);
    if (rc) return rc;
    if (won && ref_length) {
        const hipError_t ce = hipMemcpyAsync(in.room + o_length, ref_length, (size_t)nr * 8, hipMemcpyHostToDevice, g.stream);
        if (ce != hipSuccess) return fail(MHX_E_HIP, "H2D copy failed in dist_contain: %s", hipGetErrorString(ce));
    }
    ContainCall c{};
    c.q = in.q; c.q_len = in.q_len; c.r = in.r; c.r_len = in.r_len;
    c.nq = nq; c.nr = nr; c.stride = stride; c.s_q = s_q; c.s_r = s_r;
    for (uint32_t i = 0; i < nq; ++i) c.longest = std::max(c.longest, contain_eff_len(q_len[i], stride, s_q));
    for (uint32_t i = 0; i < nr; ++i) c.longest = std::max(c.longest, contain_eff_len(r_len[i], stride, s_r));
    c.shared = (uint32_t *)(in.room + o_shared); c.n_qry = (uint32_t *)(in.room + o_qry); c.n_ref = (uint32_t *)(in.room + o_ref);
    if (won) { c.won = (uint32_t *)(in.room + o_won); c.ref_length = ref_length ? (const uint64_t *)(in.room + o_length) : nullptr; }
    rc = contain_device(c);
    if (rc) return rc;
    if (won) rc = read_back("dist_contain_winner", {{won, c.won, cells * 4}});
    return rc ? rc : read_back("dist_contain", {{shared, c.shared, cells * 4}, {n_qry, c.n_qry, cells * 4}, {n_ref, c.n_ref, cells * 4}});
}
} // namespace mhx

extern "C" int mhx_dist_contain(const uint64_t *q, const uint32_t *q_len, uint32_t nq, uint32_t s_q, const uint64_t *r, const uint32_t *r_len, uint32_t nr,
                                uint32_t s_r, uint32_t stride, uint32_t *shared, uint32_t *n_qry, uint32_t *n_ref, int device_ptrs)
{
    return entry("mhx_dist_contain", [&]() -> int {
        int rc = contain_check(s_q, s_r, stride);
        if (rc) return rc;
        if (nq == 0 || nr == 0) return MHX_OK;
        if (!q || !q_len || !r || !r_len || !shared || !n_qry || !n_ref) return fail(MHX_E_ARG, "null argument");
        if (!device_ptrs) return contain_rows(nullptr, q, q_len, nq, s_q, nullptr, r, r_len, nr, s_r, stride, shared, n_qry, n_ref);
        ContainCall c{}; // the lengths are on the device: the kernels clip them, the row stride and the sketch sizes bound them
        c.q = q; c.q_len = q_len; c.r = r; c.r_len = r_len; c.nq = nq; c.nr = nr; c.stride = stride; c.s_q = s_q; c.s_r = s_r;
        c.longest = std::min(stride, std::max(s_q, s_r));
        c.shared = shared; c.n_qry = n_qry; c.n_ref = n_ref;
        return contain_device(c);
    });
}

// The same call with the winner-take-all passes behind the plain one: `won` is a fourth output, ref_length ranks ties.
extern "C" int mhx_dist_contain_winner(const uint64_t *q, const uint32_t *q_len, uint32_t nq, uint32_t s_q, const uint64_t *r, const uint32_t *r_len, uint32_t nr,
                                       uint32_t s_r, uint32_t stride, const uint64_t *ref_length, uint32_t *won, uint32_t *shared, uint32_t *n_qry, uint32_t *n_ref,
                                       int device_ptrs)
{
    return entry("mhx_dist_contain_winner", [&]() -> int {
        int rc = contain_check(s_q, s_r, stride);
        if (rc) return rc;
        if (nq == 0 || nr == 0) return MHX_OK;
        if (!q || !q_len || !r || !r_len || !won || !shared || !n_qry || !n_ref) return fail(MHX_E_ARG, "null argument");
        g.last_contain_winner_pairs = 0;
        if (!device_ptrs) return contain_rows(nullptr, q, q_len, nq, s_q, nullptr, r, r_len, nr, s_r, stride, shared, n_qry, n_ref, ref_length, won);
        ContainCall c{}; // as mhx_dist_contain: the kernels clip the lengths
        c.q = q; c.q_len = q_len; c.r = r; c.r_len = r_len; c.nq = nq; c.nr = nr; c.stride = stride; c.s_q = s_q; c.s_r = s_r;
        c.longest = std::min(stride, std::max(s_q, s_r));
        c.shared = shared; c.n_qry = n_qry; c.n_ref = n_ref; c.won = won; c.ref_length = ref_length;
        return contain_device(c);
    });
}

extern "C" uint64_t mhx_last_contain_winner_pairs(void) { return g.last_contain_winner_pairs; }
