// mhx_engine_contain_search.cpp -- host side of the containment search (mhx_dist_contain_search): the need[] table of the
// identity bound, and what it gives the schedule and the staging of mhx_engine_sets.h -- the containment's geometry, bounds,
// finish pass and pair kernel (mhx_engine_contain.cpp), writing block-local, and a take-out pass behind every block as the
// search has one.  Rules: mhx_contain_search.h and mhx_contain.h; kernels: mhx_contain_search.hip, mhx_contain.hip and mhx_dist.hip.
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "mhx_device.h"
#include "mhx_contain_search.h"
#include "mhx_engine_sets.h"
#include "mhx_internal.h"

using namespace mhx;

namespace {

struct ContainSearchCall { // everything on the device but `need`
    const uint64_t *q, *r;
    const uint32_t *q_len, *r_len;
    uint32_t nq, nr, stride, s_q, s_r, longest;
    uint32_t top;
    const uint32_t *need; // HOST: [need_limit + 1] (contain_need_build)
    uint32_t need_limit;
    uint32_t *hit_ref, *hit_shared, *hit_n_ref, *hit_n_qry, *n_hits;
};

} // namespace

namespace mhx {
// The need table of the last call stays in the engine state, on the host, like the workspace it goes into: a bound between 0
// and 1 costs about three pow per entry (some milliseconds at 50 000 entries), and the batches of a file-level call, or a
// caller that searches set after set, ask for the same table again.  A call with another bound builds it anew.
const uint32_t *contain_need_table(uint32_t limit, int k, double min_identity, uint32_t min_shared)
{
    if (g.contain_need.size() != (size_t)limit + 1 || g.contain_need_k != k || g.contain_need_min_identity != min_identity ||
        g.contain_need_min_shared != min_shared) {
        std::vector<uint32_t> fresh((size_t)limit + 1);
        contain_need_build(limit, k, min_identity, min_shared, fresh.data());
        g.contain_need.swap(fresh);
        g.contain_need_k = k; g.contain_need_min_identity = min_identity; g.contain_need_min_shared = min_shared;
    }
    return g.contain_need.data();
}

int contain_hit_check(uint32_t s_q, uint32_t s_r, uint32_t stride, int k, double min_identity, uint32_t min_shared)
{
    if (min_shared == 0) return fail(MHX_E_ARG, "min_shared must be at least 1");
    if (!(min_identity == min_identity)) return fail(MHX_E_ARG, "min_identity is not a number");
    if (k < 1 || k > 32) return fail(MHX_E_ARG, "bad k");
    if (s_q == 0 || s_r == 0 || stride == 0) return fail(MHX_E_ARG, "bad s_q / s_r / stride");
    return MHX_OK;
}
} // namespace mhx

namespace {

// Launches the whole call on the engine's stream and waits for it, on the schedule of mhx_engine_sets.h with the containment's
// geometry.  The containment's finish pass and pair kernel write a block's [queries][32] counts block-local, and the take-out
// pass merges them into the best lists, which are the outputs themselves and stay in device memory between the blocks.  A
// flagged block is taken out when it is redone -- later than its neighbours, which the total order makes harmless.  Nothing of
// size nq x nr exists.
int contain_search_device(ContainSearchCall &c)
{
    SetSchedule sch(c.nq, c.nr, c.stride, SetGeometry{contain_ranges(c.longest), c.longest, "MHX_SEARCH_QBATCH", c.nq, "containment search"});
    // the bounds and effective lengths of both sets, the block-local shared, n_qry, n_ref, the need table
    const size_t o_bq = sch.extra((size_t)c.nq * 8), o_br = sch.extra((size_t)c.nr * 8), o_eq = sch.extra((size_t)c.nq * 4), o_er = sch.extra((size_t)c.nr * 4);
    const size_t b_loc = (size_t)sch.qbatch * kTriSlice * 4;
    const size_t o_ls = sch.extra(b_loc), o_lq = sch.extra(b_loc), o_lr = sch.extra(b_loc), o_need = sch.extra(((size_t)c.need_limit + 1) * 4);
    int rc = sch.place("the containment search workspace");
    if (rc) return rc;
    hipError_t &le = sch.le;
    uint32_t *need = (uint32_t *)sch.at(o_need);
    // the table goes over before anything is queued, with a blocking copy: like the host's build of it, this lies before the
    // first event, so mhx_last_dist_kernel_ms does not hold it (tools/contain_search_rate.py times the whole call as well)
    if (hipMemcpy(need, c.need, ((size_t)c.need_limit + 1) * 4, hipMemcpyHostToDevice) != hipSuccess) return fail(MHX_E_HIP, "H2D copy of the need table failed");
    ContainArgs all{};
    all.q = c.q; all.q_len = c.q_len; all.nq = c.nq; all.r = c.r; all.r_len = c.r_len; all.nr = c.nr; all.stride = c.stride; all.s_q = c.s_q; all.s_r = c.s_r;
    all.q_bound = (uint64_t *)sch.at(o_bq); all.r_bound = (uint64_t *)sch.at(o_br);
    all.q_eff = (uint32_t *)sch.at(o_eq); all.r_eff = (uint32_t *)sch.at(o_er);
    all.shift = sch.words;
    all.shared = (uint32_t *)sch.at(o_ls); all.n_qry = (uint32_t *)sch.at(o_lq); all.n_ref = (uint32_t *)sch.at(o_lr); all.out_stride = kTriSlice;
    auto block_args = [&](const SearchBlock &b) { // cell (q, r) of the block lies at (q - q0) * 32 + (r - r0)
        ContainArgs x = all;
        x.q0 = b.q0; x.bnq = b.nq; x.r0 = b.r0; x.bnr = b.nr;
        x.out_base = (uint64_t)b.q0 * kTriSlice + b.r0;
        return x;
    };
    ContainSearchOut out{};
    out.loc_shared = all.shared; out.loc_n_qry = all.n_qry; out.loc_n_ref = all.n_ref; out.top = c.top; out.need = need; out.need_limit = c.need_limit;
    out.hit_ref = c.hit_ref; out.hit_shared = c.hit_shared; out.hit_n_ref = c.hit_n_ref; out.hit_n_qry = c.hit_n_qry; out.n_hits = c.n_hits;
    // the passes of mhx_dist.hip see the effective lengths: what lies behind them in a row is not part of a list
    DistArgs lists{};
    lists.q = c.q; lists.q_len = all.q_eff; lists.nq = c.nq; lists.r = c.r; lists.r_len = all.r_eff; lists.nr = c.nr; lists.stride = c.stride;
    sch.begin();
    if (le == hipSuccess) le = hipMemsetAsync(c.n_hits, 0, (size_t)c.nq * 4, g.stream);
    if (le == hipSuccess) le = launch_contain_bounds(all, g.stream);
    sch.offsets(lists);
    rc = sch.run(
        0, c.nq, [&](const SearchBlock &b, const DistArgs &) { return launch_contain_pairs(block_args(b), g.stream); },
        [&](const SearchBlock &b, const DistArgs &, const DistWork &w) { return launch_contain_finish(block_args(b), w, g.stream); },
        [&](const SearchBlock &b, const uint32_t *flag) {
            ContainSearchOut t = out;
            t.flag = flag; t.r0 = b.r0; t.nr = b.nr; t.q0 = b.q0; t.nq = b.nq;
            return launch_contain_take(t, g.stream);
        });
    if (rc == MHX_OK) rc = sch.end();
    return rc ? rc : sch.wait();
}

int contain_search_check(uint32_t s_q, uint32_t s_r, uint32_t stride, int k, double min_identity, uint32_t min_shared, uint32_t top)
{
    if (top < 1 || top > kSearchMaxTop) return fail(MHX_E_ARG, "top must be 1 .. %u", kSearchMaxTop);
    return contain_hit_check(s_q, s_r, stride, k, min_identity, min_shared);
}

// Host queries against references that are on the device already (refs) or on the host (r / r_len, refs null).  The lists
// the device leaves are the result: the hit test is exact there.  Staging holds the rows, the lengths and the [nq][top] lists.
int contain_search_host(const uint64_t *q, const uint64_t *const *q_rows, const uint32_t *q_len, uint32_t nq, uint32_t s_q, const uint64_t *r,
                        const uint32_t *r_len, const SearchRefs *refs, uint32_t nr, uint32_t s_r, uint32_t stride, int k, double min_identity,
                        uint32_t min_shared, uint32_t top, uint32_t *hit_ref, uint32_t *hit_shared, uint32_t *hit_n_ref, uint32_t *hit_n_qry, uint32_t *n_hits)
{
    const size_t cells = (size_t)nq * top;
    Carve lists; // the four [nq][top] lists and their lengths
    const size_t o_ref = lists.take(cells * 4), o_shared = lists.take(cells * 4), o_nref = lists.take(cells * 4), o_nqry = lists.take(cells * 4);
    const size_t o_n = lists.take((size_t)nq * 4);
    StagedSets in{};
    int rc = stage_sets("dist_contain_search", HostSet{q, q_rows, q_len, nq}, HostSet{r, nullptr, r_len, nr}, refs, stride, lists.bytes, in);
    if (rc) return rc;
    ContainSearchCall c{};
    c.q = in.q; c.q_len = in.q_len; c.r = in.r; c.r_len = in.r_len;
    c.nq = nq; c.nr = nr; c.stride = stride; c.s_q = s_q; c.s_r = s_r; c.top = top;
    c.longest = refs ? contain_eff_len(refs->longest, stride, s_r) : 0;
    for (uint32_t i = 0; i < nq; ++i) c.longest = std::max(c.longest, contain_eff_len(q_len[i], stride, s_q));
    if (!refs) for (uint32_t i = 0; i < nr; ++i) c.longest = std::max(c.longest, contain_eff_len(r_len[i], stride, s_r));
    c.need_limit = std::min(stride, s_r);
    c.need = contain_need_table(c.need_limit, k, min_identity, min_shared);
    c.hit_ref = (uint32_t *)(in.room + o_ref); c.hit_shared = (uint32_t *)(in.room + o_shared); c.hit_n_ref = (uint32_t *)(in.room + o_nref);
    c.hit_n_qry = (uint32_t *)(in.room + o_nqry); c.n_hits = (uint32_t *)(in.room + o_n);
    rc = contain_search_device(c);
    if (rc) return rc;
    rc = read_back("dist_contain_search", {{hit_ref, c.hit_ref, cells * 4}, {hit_shared, c.hit_shared, cells * 4}, {hit_n_ref, c.hit_n_ref, cells * 4}, {hit_n_qry, c.hit_n_qry, cells * 4},
                                            {n_hits, c.n_hits, (size_t)nq * 4}});
    if (rc) return rc;
    for (uint32_t i = 0; i < nq; ++i) { // what the staging held behind a list's end is not part of the result
        if (n_hits[i] > top) return fail(MHX_E_INTERNAL, "containment search list of query %u longer than top", i);
        for (size_t t = (size_t)i * top + n_hits[i]; t < (size_t)(i + 1) * top; ++t) hit_ref[t] = hit_shared[t] = hit_n_ref[t] = hit_n_qry[t] = 0;
    }
    return MHX_OK;
}

} // namespace

namespace mhx {
int contain_search_rows(const uint64_t *const *q_rows, const uint32_t *q_len, uint32_t nq, uint32_t s_q, const SearchRefs &refs, uint32_t s_r, int k,
                        double min_identity, uint32_t min_shared, uint32_t top, uint32_t *hit_ref, uint32_t *hit_shared, uint32_t *hit_n_ref,
                        uint32_t *hit_n_qry, uint32_t *n_hits)
{
    int rc = contain_search_check(s_q, s_r, refs.stride, k, min_identity, min_shared, top);
    if (rc || nq == 0) return rc;
    if (refs.nr == 0) { memset(n_hits, 0, (size_t)nq * 4); return MHX_OK; }
    return contain_search_host(nullptr, q_rows, q_len, nq, s_q, nullptr, nullptr, &refs, refs.nr, s_r, refs.stride, k, min_identity, min_shared, top, hit_ref,
                               hit_shared, hit_n_ref, hit_n_qry, n_hits);
}
} // namespace mhx

extern "C" int mhx_dist_contain_search(const uint64_t *q, const uint32_t *q_len, uint32_t nq, uint32_t s_q, const uint64_t *r, const uint32_t *r_len, uint32_t nr,
                                       uint32_t s_r, uint32_t stride, int k, double min_identity, uint32_t min_shared, uint32_t top, uint32_t *hit_ref,
                                       uint32_t *hit_shared, uint32_t *hit_n_ref, uint32_t *hit_n_qry, uint32_t *n_hits, int device_ptrs)
{
    return entry("mhx_dist_contain_search", [&]() -> int {
        int rc = contain_search_check(s_q, s_r, stride, k, min_identity, min_shared, top);
        if (rc) return rc;
        if (nq == 0) return MHX_OK;
        if (!n_hits) return fail(MHX_E_ARG, "null argument");
        if (nr == 0) {
            if (device_ptrs) { if (hipMemset(n_hits, 0, (size_t)nq * 4) != hipSuccess) return fail(MHX_E_HIP, "hipMemset failed in dist_contain_search"); }
            else memset(n_hits, 0, (size_t)nq * 4);
            return MHX_OK;
        }
        if (!q || !q_len || !r || !r_len || !hit_ref || !hit_shared || !hit_n_ref || !hit_n_qry) return fail(MHX_E_ARG, "null argument");
        if (!device_ptrs)
            return contain_search_host(q, nullptr, q_len, nq, s_q, r, r_len, nullptr, nr, s_r, stride, k, min_identity, min_shared, top, hit_ref, hit_shared,
                                       hit_n_ref, hit_n_qry, n_hits);
        ContainSearchCall c{}; // the lengths are on the device: the kernels clip them, the row stride and the sketch sizes bound them
        c.q = q; c.q_len = q_len; c.r = r; c.r_len = r_len; c.nq = nq; c.nr = nr; c.stride = stride; c.s_q = s_q; c.s_r = s_r; c.top = top;
        c.longest = std::min(stride, std::max(s_q, s_r));
        c.need_limit = std::min(stride, s_r);
        c.need = contain_need_table(c.need_limit, k, min_identity, min_shared);
        c.hit_ref = hit_ref; c.hit_shared = hit_shared; c.hit_n_ref = hit_n_ref; c.hit_n_qry = hit_n_qry; c.n_hits = n_hits;
        return contain_search_device(c);
    });
}
