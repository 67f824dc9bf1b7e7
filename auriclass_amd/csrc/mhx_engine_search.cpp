// mhx_engine_search.cpp -- host side of the reference-set search (mhx_dist_search): what it gives the schedule and the
// staging of mhx_engine_sets.h -- its geometry, the block-local results, the finish pass, the generic pair kernel and the
// take-out pass that merges a block's candidates into every query's best list -- and the exact distance rule on the host.
// Rules: mhx_search.h; kernels: mhx_search.hip, mhx_triangle.hip and mhx_dist.hip.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <exception>
#include <new>
#include <vector>

#include "mhx_device.h"
#include "mhx_search.h"
#include "mhx_engine_sets.h"
#include "mhx_internal.h"

using namespace mhx;

namespace {

struct SearchCall { // everything on the device
    const uint64_t *q, *r;
    const uint32_t *q_len, *r_len;
    uint32_t nq, nr, stride, s, longest;
    int k;
    uint32_t top;
    double jmin;
    uint32_t *hit_ref, *hit_common, *hit_denom, *n_hits;
    double *hit_dist; // may be null
};

// Launches the whole call on the engine's stream and waits for it, on the schedule of mhx_engine_sets.h: every block's finish
// pass writes its block-local [queries][32] results, and the take-out pass merges them into the best lists, which stay in
// device memory between the blocks.  A flagged block is redone by the generic pair kernel into the same block-local arrays
// and taken out then -- later than its neighbours, which the total order makes harmless.
int search_device(SearchCall &c)
{
    const char *geo = getenv("MHX_SEARCH_GEOMETRY");
    const uint32_t ranges = geo && strcmp(geo, "dist") == 0 ? tri_ranges_dist(c.longest) : tri_ranges(c.longest);
    SetSchedule sch(c.nq, c.nr, c.stride, SetGeometry{ranges, c.s, "MHX_SEARCH_QBATCH", c.nq, "search"});
    const size_t o_lc = sch.extra((size_t)sch.qbatch * kTriSlice * 4), o_ld = sch.extra((size_t)sch.qbatch * kTriSlice * 4); // block-local common, denom
    int rc = sch.place("the search workspace");
    if (rc) return rc;
    hipError_t &le = sch.le;
    DistArgs all{};
    all.q = c.q; all.q_len = c.q_len; all.nq = c.nq; all.r = c.r; all.r_len = c.r_len; all.nr = c.nr; all.stride = c.stride; all.s = c.s; all.k = c.k;
    all.common = (uint32_t *)sch.at(o_lc); all.denom = (uint32_t *)sch.at(o_ld); all.dist = nullptr; all.out_stride = kTriSlice; all.out_off = 0;
    SearchOut out{};
    out.loc_common = all.common; out.loc_denom = all.denom; out.top = c.top; out.k = c.k; out.jmin = c.jmin;
    out.hit_ref = c.hit_ref; out.hit_common = c.hit_common; out.hit_denom = c.hit_denom; out.n_hits = c.n_hits; out.hit_dist = c.hit_dist;
    sch.begin();
    if (le == hipSuccess) le = hipMemsetAsync(c.n_hits, 0, (size_t)c.nq * 4, g.stream);
    sch.offsets(all);
    rc = sch.run(
        0, c.nq, [&](const SearchBlock &, const DistArgs &x) { return launch_dist_pairs(x, g.stream); },
        [&](const SearchBlock &, const DistArgs &x, const DistWork &w) {
            return ranges < (uint32_t)kDistRanges ? launch_tri_finish_small(x, w, g.stream) : launch_dist_finish(x, w, g.stream);
        },
        [&](const SearchBlock &b, const uint32_t *flag) {
            SearchOut t = out;
            t.flag = flag; t.r0 = b.r0; t.nr = b.nr; t.q0 = b.q0; t.nq = b.nq;
            return launch_search_take(t, g.stream);
        });
    if (rc) return rc;
    if (le == hipSuccess && c.hit_dist) {
        SearchOut t = out;
        t.q0 = 0; t.nq = c.nq;
        le = launch_search_dist(t, g.stream);
    }
    rc = sch.end();
    return rc ? rc : sch.wait();
}

int search_check(uint32_t nq, uint32_t nr, uint32_t stride, int k, uint32_t s, double max_dist, uint32_t top)
{
    if (top < 1 || top > kSearchMaxTop) return fail(MHX_E_ARG, "top must be 1 .. %u", kSearchMaxTop);
    if (!(max_dist == max_dist)) return fail(MHX_E_ARG, "max_dist is not a number");
    if (k < 1 || k > 32 || s == 0 || stride == 0) return fail(MHX_E_ARG, "bad k / s / stride");
    return MHX_OK;
}

// Host queries against references that are on the device already (refs) or on the host (r / r_len, refs null).  The
// device's lists hold what passes the prefilter, in rank order; the exact rule -- the libm distance, the double that is
// printed, <= max_dist -- drops what it does not keep.  A pair it drops ranks behind every pair it keeps (the distance
// falls as the index rises), so nothing that belongs into a list was pushed out of it by one that does not.
int search_host(const uint64_t *q, const uint64_t *const *q_rows, const uint32_t *q_len, uint32_t nq, const uint64_t *r, const uint32_t *r_len,
                const SearchRefs *refs, uint32_t nr, uint32_t stride, int k, uint32_t s, double max_dist, uint32_t top, uint32_t *hit_ref,
                uint32_t *hit_common, uint32_t *hit_denom, double *hit_dist, uint32_t *n_hits, SearchStaged *staged = nullptr)
{
    const size_t cells = (size_t)nq * top;
    Carve lists; // the [nq][top] lists and their lengths
    const size_t o_ref = lists.take(cells * 4), o_common = lists.take(cells * 4), o_denom = lists.take(cells * 4), o_n = lists.take((size_t)nq * 4);
    StagedSets in{};
    int rc = stage_sets("dist_search", HostSet{q, q_rows, q_len, nq}, HostSet{r, nullptr, r_len, nr}, refs, stride, lists.bytes, in);
    if (rc) return rc;
    SearchCall c{};
    c.q = in.q; c.q_len = in.q_len; c.r = in.r; c.r_len = in.r_len;
    c.nq = nq; c.nr = nr; c.stride = stride; c.s = s; c.k = k; c.top = top;
    c.longest = refs ? refs->longest : 0;
    for (uint32_t i = 0; i < nq; ++i) c.longest = std::max(c.longest, q_len[i]);
    if (!refs) for (uint32_t i = 0; i < nr; ++i) c.longest = std::max(c.longest, r_len[i]);
    c.jmin = tri_jmin(max_dist, k);
    c.hit_ref = (uint32_t *)(in.room + o_ref); c.hit_common = (uint32_t *)(in.room + o_common); c.hit_denom = (uint32_t *)(in.room + o_denom);
    c.n_hits = (uint32_t *)(in.room + o_n);
    c.hit_dist = nullptr; // distances in host libm below
    if (staged) *staged = SearchStaged{c.q, c.q_len};
    rc = search_device(c);
    if (rc) return rc;
    rc = read_back("dist_search", {{hit_ref, c.hit_ref, cells * 4}, {hit_common, c.hit_common, cells * 4}, {hit_denom, c.hit_denom, cells * 4}, {n_hits, c.n_hits, (size_t)nq * 4}});
    if (rc) return rc;
    for (uint32_t i = 0; i < nq; ++i) {
        uint32_t *hr = hit_ref + (size_t)i * top, *hc = hit_common + (size_t)i * top, *hd = hit_denom + (size_t)i * top;
        double *hx = hit_dist ? hit_dist + (size_t)i * top : nullptr;
        if (n_hits[i] > top) return fail(MHX_E_INTERNAL, "search list of query %u longer than top", i);
        uint32_t m = 0;
        for (uint32_t t = 0; t < n_hits[i]; ++t) {
            const double d = tri_distance(hc[t], hd[t], k);
            if (!(d <= max_dist)) continue;
            hr[m] = hr[t]; hc[m] = hc[t]; hd[m] = hd[t];
            if (hx) hx[m] = d;
            ++m;
        }
        for (uint32_t t = m; t < top; ++t) { hr[t] = hc[t] = hd[t] = 0; if (hx) hx[t] = 0.0; }
        n_hits[i] = m;
    }
    return MHX_OK;
}

} // namespace

namespace mhx {
int search_rows(const uint64_t *const *q_rows, const uint32_t *q_len, uint32_t nq, const SearchRefs &refs, int k, uint32_t s, double max_dist,
                uint32_t top, uint32_t *hit_ref, uint32_t *hit_common, uint32_t *hit_denom, double *hit_dist, uint32_t *n_hits, SearchStaged *staged)
{
    int rc = search_check(nq, refs.nr, refs.stride, k, s, max_dist, top);
    if (rc || nq == 0) return rc;
    if (refs.nr == 0) { memset(n_hits, 0, (size_t)nq * 4); return MHX_OK; }
    return search_host(nullptr, q_rows, q_len, nq, nullptr, nullptr, &refs, refs.nr, refs.stride, k, s, max_dist, top, hit_ref, hit_common, hit_denom,
                       hit_dist, n_hits, staged);
}
} // namespace mhx

extern "C" int mhx_dist_search(const uint64_t *q, const uint32_t *q_len, uint32_t nq, const uint64_t *r, const uint32_t *r_len, uint32_t nr, uint32_t stride, int k,
                               uint32_t s, double max_dist, uint32_t top, uint32_t *hit_ref, uint32_t *hit_common, uint32_t *hit_denom, double *hit_dist,
                               uint32_t *n_hits, int device_ptrs)
{
    return entry("mhx_dist_search", [&]() -> int {
        int rc = search_check(nq, nr, stride, k, s, max_dist, top);
        if (rc) return rc;
        if (nq == 0) return MHX_OK;
        if (!n_hits) return fail(MHX_E_ARG, "null argument");
        if (nr == 0) {
            if (device_ptrs) { if (hipMemset(n_hits, 0, (size_t)nq * 4) != hipSuccess) return fail(MHX_E_HIP, "hipMemset failed in dist_search"); }
            else memset(n_hits, 0, (size_t)nq * 4);
            return MHX_OK;
        }
        if (!q || !q_len || !r || !r_len || !hit_ref || !hit_common || !hit_denom) return fail(MHX_E_ARG, "null argument");
        if (!device_ptrs) return search_host(q, nullptr, q_len, nq, r, r_len, nullptr, nr, stride, k, s, max_dist, top, hit_ref, hit_common, hit_denom, hit_dist, n_hits);
        SearchCall c{}; // the lists stay where they are: prefiltered only, in rank order
        c.q = q; c.q_len = q_len; c.r = r; c.r_len = r_len; c.nq = nq; c.nr = nr; c.stride = stride; c.s = s; c.k = k; c.top = top;
        c.longest = stride; // the lengths are on the device: the row stride bounds them
        c.jmin = tri_jmin(max_dist, k);
        c.hit_ref = hit_ref; c.hit_common = hit_common; c.hit_denom = hit_denom; c.n_hits = n_hits; c.hit_dist = hit_dist;
        return search_device(c);
    });
}
