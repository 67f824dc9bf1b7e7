// mhx_engine_within.cpp -- host side of the bounded neighbourhood call (mhx_dist_within: all references within a distance of
// each query, as CSR): the cmin table of the bound, what it gives the schedule and the staging of mhx_engine_sets.h -- the
// search's geometry and passes with its own take-out -- the super-batches of queries that each are one run of that schedule,
// and behind the last block of each the scan and the gather.
// Rules: mhx_within.h; kernels: mhx_within.hip, mhx_triangle.hip and mhx_dist.hip.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <exception>
#include <new>
#include <vector>

#include "mhx_device.h"
#include "mhx_within.h"
#include "mhx_mst.h"
#include "mhx_engine_sets.h"
#include "mhx_internal.h"

using namespace mhx;

namespace {

struct WithinCall { // everything on the device but n_out
    const uint64_t *q, *r;
    const uint32_t *q_len, *r_len;
    uint32_t nq, nr, stride, s, longest;
    int k;
    double max_dist;
    uint64_t *row_off;                          // [nq + 1]
    uint32_t *hit_ref, *hit_common, *hit_denom; // [cap]; hit_ref null: the counting form
    double *hit_dist;                           // may be null
    uint64_t cap;
    uint64_t *n_out;                            // host
};

// The bound as integers on the device: cluster_cmin_build with the host's libm, kept until another (s, k, max_dist) comes.
int within_cmin(uint32_t s, int k, double max_dist, const uint32_t **out)
{
    if (g.within_cmin.cap() < (size_t)s + 1 || g.within_cmin_s != s || g.within_cmin_k != k || memcmp(&g.within_cmin_max_dist, &max_dist, sizeof max_dist) != 0) {
        std::vector<uint32_t> cmin((size_t)s + 1);
        cluster_cmin_build(s, k, max_dist, cmin.data());
        g.within_cmin_s = 0; // (nothing valid while the copy runs)
        if (g.within_cmin.grow((size_t)s + 1, g.stream) != hipSuccess) return fail(MHX_E_HIP, "hipMalloc failed for the bound table (%zu bytes)", ((size_t)s + 1) * 4);
        if (hipMemcpyAsync(g.within_cmin, cmin.data(), cmin.size() * 4, hipMemcpyHostToDevice, g.stream) != hipSuccess || hipStreamSynchronize(g.stream) != hipSuccess)
            return fail(MHX_E_HIP, "H2D copy of the bound table failed");
        g.within_cmin_s = s; g.within_cmin_k = k; g.within_cmin_max_dist = max_dist;
    }
    *out = g.within_cmin;
    return MHX_OK;
}

// Launches the whole call on the engine's stream and waits for it, on the schedule of mhx_engine_sets.h with the search's
// geometry.  The queries go through in super-batches (mhx_within.h) whose cells live in g.within_ws: one run of the schedule
// per super-batch, and behind its last block and its last fallback the cells are scanned into row_off and the arrival list is
// gathered into the call's outputs.  A block that is redone later fills the same cells, so neither the order of the blocks
// nor the batch sizes show in the result.
int within_device(WithinCall &c)
{
    const uint32_t *cmin = nullptr;
    int rc = within_cmin(c.s, c.k, c.max_dist, &cmin);
    if (rc) return rc;
    const char *geo = getenv("MHX_WITHIN_GEOMETRY");
    const uint32_t ranges = geo && strcmp(geo, "dist") == 0 ? tri_ranges_dist(c.longest) : tri_ranges(c.longest);
    uint64_t cells = kWithinCells;
    if (const char *e = getenv("MHX_WITHIN_CELLS")) { const long long v = atoll(e); if (v > 0 && (uint64_t)v < cells) cells = (uint64_t)v; }
    const uint32_t nslices = within_slices(c.nr), super = within_super_queries(c.nq, c.nr, cells);
    SetSchedule sch(c.nq, c.nr, c.stride, SetGeometry{ranges, c.s, "MHX_WITHIN_QBATCH", super, "dist_within"});
    sch.clear_first = sch.clear_later = sch.fast; // the flag words of the super-batch before are not this one's
    const size_t o_lc = sch.extra((size_t)sch.qbatch * kTriSlice * 4), o_ld = sch.extra((size_t)sch.qbatch * kTriSlice * 4); // block-local common, denom
    rc = sch.place("the workspace of dist_within");
    if (rc) return rc;
    const bool store = c.hit_ref != nullptr && c.cap != 0;
    // the arrival list of a super-batch: its hits are at most its pairs (below 2^32: kWithinCells x 32, or one row of the
    // references), and what lies beyond the room the caller gave is only counted
    const uint32_t room = store ? (uint32_t)std::min<uint64_t>(c.cap, (uint64_t)super * c.nr) : 0;
    // the cells of a super-batch: [mask][base][arrival counter][arrival common][arrival denom]
    Carve cw;
    const size_t o_mask = cw.take((size_t)super * nslices * 4), o_base = cw.take(store ? (size_t)super * nslices * 4 : 0), o_count = cw.take(256);
    const size_t o_arr_c = cw.take((size_t)room * 4), o_arr_d = cw.take((size_t)room * 4);
    if (g.within_ws.grow(cw.bytes, g.stream) != hipSuccess) return fail(MHX_E_HIP, "hipMalloc failed for the cells of dist_within (%zu bytes)", cw.bytes);
    uint32_t *mask = (uint32_t *)(g.within_ws + o_mask), *base = store ? (uint32_t *)(g.within_ws + o_base) : nullptr;
    uint32_t *count = (uint32_t *)(g.within_ws + o_count);
    uint32_t *arr_c = (uint32_t *)(g.within_ws + o_arr_c), *arr_d = (uint32_t *)(g.within_ws + o_arr_d);
    hipError_t &le = sch.le;
    DistArgs all{};
    all.q = c.q; all.q_len = c.q_len; all.nq = c.nq; all.r = c.r; all.r_len = c.r_len; all.nr = c.nr; all.stride = c.stride; all.s = c.s; all.k = c.k;
    all.common = (uint32_t *)sch.at(o_lc); all.denom = (uint32_t *)sch.at(o_ld); all.dist = nullptr; all.out_stride = kTriSlice; all.out_off = 0;
    WithinOut out{};
    out.loc_common = all.common; out.loc_denom = all.denom; out.cmin = cmin; out.s = c.s; out.nslices = nslices; out.mask = mask; out.base = base;
    out.arr_common = arr_c; out.arr_denom = arr_d; out.room = room; out.count = count;
    sch.begin();
    if (le == hipSuccess) le = hipMemsetAsync(c.row_off, 0, 8, g.stream);
    sch.offsets(all);
    for (uint32_t s0 = 0; s0 < c.nq && le == hipSuccess; s0 += super) {
        const uint32_t snq = std::min(super, c.nq - s0);
        le = hipMemsetAsync(mask, 0, (size_t)snq * nslices * 4, g.stream);
        if (le == hipSuccess) le = hipMemsetAsync(count, 0, 4, g.stream);
        rc = sch.run(
            s0, snq, [&](const SearchBlock &, const DistArgs &x) { return launch_dist_pairs(x, g.stream); },
            [&](const SearchBlock &, const DistArgs &x, const DistWork &w) {
                return ranges < (uint32_t)kDistRanges ? launch_tri_finish_small(x, w, g.stream) : launch_dist_finish(x, w, g.stream);
            },
            [&](const SearchBlock &b, const uint32_t *flag) {
                WithinOut t = out;
                t.flag = flag; t.r0 = b.r0; t.nr = b.nr; t.q0 = b.q0; t.nq = b.nq;
                return launch_within_take(t, g.stream);
            });
        if (rc) return rc;
        if (le != hipSuccess) break;
        WithinRows rows{};
        rows.mask = mask; rows.base = base; rows.nq = snq; rows.nslices = nslices; rows.row_off = c.row_off + s0;
        rows.arr_common = arr_c; rows.arr_denom = arr_d; rows.room = room;
        rows.hit_ref = c.hit_ref; rows.hit_common = c.hit_common; rows.hit_denom = c.hit_denom; rows.hit_dist = c.hit_dist; rows.cap = store ? c.cap : 0; rows.k = c.k;
        le = launch_within_scan(rows, g.stream);
        if (le == hipSuccess) le = launch_within_gather(rows, g.stream);
    }
    rc = sch.end();
    return rc ? rc : sch.wait(hipMemcpyAsync(c.n_out, c.row_off + c.nq, 8, hipMemcpyDeviceToHost, g.stream));
}

int within_check(uint32_t stride, int k, uint32_t s, double max_dist)
{
    if (!(max_dist == max_dist)) return fail(MHX_E_ARG, "max_dist is not a number");
    if (k < 1 || k > 32 || s == 0 || stride == 0) return fail(MHX_E_ARG, "bad k / s / stride");
    if (s >= kMstMaxS) return fail(MHX_E_ARG, "sketch size too large for dist_within (%u, below %u)", s, kMstMaxS);
    return MHX_OK;
}

int too_small(uint64_t found) { return fail(MHX_E_CAPACITY, "hit list too small (%llu needed)", (unsigned long long)found); }

// Host queries against references that are on the device already (refs) or on the host (r / r_len, refs null).  The device's
// CSR is the result: the bound went there as integers, so nothing is filtered here; only the distances are the host's libm.
int within_host(const uint64_t *q, const uint64_t *const *q_rows, const uint32_t *q_len, uint32_t nq, const uint64_t *r, const uint32_t *r_len,
                const SearchRefs *refs, uint32_t nr, uint32_t stride, int k, uint32_t s, double max_dist, uint64_t *row_off, uint32_t *hit_ref,
                uint32_t *hit_common, uint32_t *hit_denom, double *hit_dist, uint64_t cap, uint64_t *n_out)
{
    const uint64_t room = hit_ref ? std::min<uint64_t>(cap, (uint64_t)nq * nr) : 0;
    Carve csr; // row_off and the three hit arrays
    const size_t o_off = csr.take(((size_t)nq + 1) * 8), o_ref = csr.take((size_t)room * 4), o_common = csr.take((size_t)room * 4), o_denom = csr.take((size_t)room * 4);
    StagedSets in{};
    int rc = stage_sets("dist_within", HostSet{q, q_rows, q_len, nq}, HostSet{r, nullptr, r_len, nr}, refs, stride, csr.bytes, in);
    if (rc) return rc;
    WithinCall c{};
    c.q = in.q; c.q_len = in.q_len; c.r = in.r; c.r_len = in.r_len;
    c.nq = nq; c.nr = nr; c.stride = stride; c.s = s; c.k = k; c.max_dist = max_dist;
    c.longest = refs ? refs->longest : 0;
    for (uint32_t i = 0; i < nq; ++i) c.longest = std::max(c.longest, q_len[i]);
    if (!refs) for (uint32_t i = 0; i < nr; ++i) c.longest = std::max(c.longest, r_len[i]);
    c.row_off = (uint64_t *)(in.room + o_off);
    if (room) { c.hit_ref = (uint32_t *)(in.room + o_ref); c.hit_common = (uint32_t *)(in.room + o_common); c.hit_denom = (uint32_t *)(in.room + o_denom); }
    c.hit_dist = nullptr; // distances in host libm below
    c.cap = room;
    c.n_out = n_out;
    rc = within_device(c);
    if (rc) return rc;
    rc = read_back("dist_within", {{row_off, c.row_off, ((size_t)nq + 1) * 8}});
    if (rc) return rc;
    if (!hit_ref && cap == 0) return MHX_OK; // the counting form
    const uint64_t m = *n_out;
    if (m > cap) return too_small(m);
    rc = read_back("dist_within", {{hit_ref, c.hit_ref, m * 4, m != 0}, {hit_common, c.hit_common, m * 4, m != 0}, {hit_denom, c.hit_denom, m * 4, m != 0}});
    if (rc) return rc;
    if (hit_dist)
        for (uint64_t i = 0; i < m; ++i) hit_dist[i] = tri_distance(hit_common[i], hit_denom[i], k);
    return MHX_OK;
}

} // namespace

namespace mhx {
int within_rows(const uint64_t *const *q_rows, const uint32_t *q_len, uint32_t nq, const SearchRefs &refs, int k, uint32_t s, double max_dist,
                uint64_t *row_off, uint32_t *hit_ref, uint32_t *hit_common, uint32_t *hit_denom, double *hit_dist, uint64_t cap, uint64_t *n_out)
{
    *n_out = 0;
    int rc = within_check(refs.stride, k, s, max_dist);
    if (rc || nq == 0) return rc;
    if (refs.nr == 0) { memset(row_off, 0, ((size_t)nq + 1) * 8); return MHX_OK; }
    return within_host(nullptr, q_rows, q_len, nq, nullptr, nullptr, &refs, refs.nr, refs.stride, k, s, max_dist, row_off, hit_ref, hit_common, hit_denom,
                       hit_dist, cap, n_out);
}
} // namespace mhx

extern "C" int mhx_dist_within(const uint64_t *q, const uint32_t *q_len, uint32_t nq, const uint64_t *r, const uint32_t *r_len, uint32_t nr, uint32_t stride, int k,
                               uint32_t s, double max_dist, uint64_t *row_off, uint32_t *hit_ref, uint32_t *hit_common, uint32_t *hit_denom, double *hit_dist,
                               uint64_t cap, uint64_t *n_out, int device_ptrs)
{
    return entry("mhx_dist_within", [&]() -> int {
        int rc = within_check(stride, k, s, max_dist);
        if (rc) return rc;
        if (nq == 0) return MHX_OK;
        if (!row_off || !n_out) return fail(MHX_E_ARG, "null argument");
        const bool counting = !hit_ref && cap == 0;
        if (!counting && (!hit_ref || !hit_common || !hit_denom)) return fail(MHX_E_ARG, "null argument");
        *n_out = 0;
        if (nr == 0) {
            if (device_ptrs) { if (hipMemset(row_off, 0, ((size_t)nq + 1) * 8) != hipSuccess) return fail(MHX_E_HIP, "hipMemset failed in dist_within"); }
            else memset(row_off, 0, ((size_t)nq + 1) * 8);
            return MHX_OK;
        }
        if (!q || !q_len || !r || !r_len) return fail(MHX_E_ARG, "null argument");
        if (!device_ptrs) return within_host(q, nullptr, q_len, nq, r, r_len, nullptr, nr, stride, k, s, max_dist, row_off, hit_ref, hit_common, hit_denom, hit_dist, cap, n_out);
        WithinCall c{}; // the result stays where it is, exact and in its final order
        c.q = q; c.q_len = q_len; c.r = r; c.r_len = r_len; c.nq = nq; c.nr = nr; c.stride = stride; c.s = s; c.k = k; c.max_dist = max_dist;
        c.longest = stride; // the lengths are on the device: the row stride bounds them
        c.row_off = row_off; c.hit_ref = hit_ref; c.hit_common = hit_common; c.hit_denom = hit_denom; c.hit_dist = hit_dist; c.cap = cap; c.n_out = n_out;
        rc = within_device(c);
        if (rc) return rc;
        return !counting && *n_out > cap ? too_small(*n_out) : MHX_OK;
    });
}
