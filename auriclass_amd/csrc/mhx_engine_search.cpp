// mhx_engine_search.cpp -- host side of the reference-set search (mhx_dist_search): staging of a host-pointer call, ONE
// split of both sets into value ranges, the schedule of (query batch, reference slice) blocks, the fallback of a flagged
// block to the generic pair kernel, the take-out pass that merges a block's candidates into every query's best list, and
// the exact distance rule on the host.  Rules: mhx_search.h; kernels: mhx_search.hip, mhx_triangle.hip and mhx_dist.hip.
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
#include "mhx_engine_internal.h"
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

size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

// Launches the whole call on the engine's stream and waits for it.  Both sets are split into value ranges ONCE, with one
// shift (launch_dist_offsets_both); every block then runs the range pass and a finish pass into its block-local
// [queries][32] results, and the take-out pass merges them into the best lists, which stay in device memory between the
// blocks.  Block flags come back once per group of blocks; a flagged block is redone by the generic pair kernel into the
// same block-local arrays and taken out then -- later than its neighbours, which the total order makes harmless.
int search_device(SearchCall &c)
{
    const uint64_t pairs = (uint64_t)c.nq * c.nr;
    const char *geo = getenv("MHX_SEARCH_GEOMETRY");
    const uint32_t ranges = geo && strcmp(geo, "dist") == 0 ? tri_ranges_dist(c.longest) : tri_ranges(c.longest);
    const bool fast = (pairs >= 64 || (pairs >= 8 && pairs * (uint64_t)c.s >= 400000)) && ranges != 0 && getenv("MHX_DIST_GENERIC") == nullptr;
    uint32_t qbatch = tri_max_queries(fast ? ranges : kTriMinRanges);
    if (const char *e = getenv("MHX_SEARCH_QBATCH")) { const long v = atol(e); if (v > 0 && (uint64_t)v < qbatch) qbatch = (uint32_t)v; }
    qbatch = std::min(qbatch, c.nq);
    const uint64_t nblocks = search_blocks(c.nq, c.nr, qbatch);
    constexpr uint64_t kBlockGroup = 4096; // blocks whose flag words come back together
    const uint32_t group = (uint32_t)std::min(nblocks, kBlockGroup);
    // workspace: [offsets of the queries][offsets of the references][byte counters][window totals][block-local common,
    // denom][words: shift, 0, then two per block of a group]
    const uint64_t per = (uint64_t)ranges + 1;
    size_t o = 0;
    const size_t o_offq = o; if (fast) o += up256((size_t)c.nq * per * 4);
    const size_t o_offr = o; if (fast) o += up256((size_t)c.nr * per * 4);
    const size_t o_cpart = o; if (fast) o += up256((size_t)qbatch * ranges * kTriSlice);
    const size_t o_wtot = o; if (fast && ranges > (uint32_t)kDistRanges) o += up256((size_t)qbatch * (ranges / kDistWindowRanges) * kTriSlice * 4);
    const size_t o_lc = o; o += up256((size_t)qbatch * kTriSlice * 4);
    const size_t o_ld = o; o += up256((size_t)qbatch * kTriSlice * 4);
    const size_t o_words = o; o += up256((size_t)(2 + 2 * group) * 4);
    if (g.dist_ws.grow(o, g.stream) != hipSuccess) return fail(MHX_E_HIP, "hipMalloc failed for the search workspace (%zu bytes)", o);
    uint32_t *offq = (uint32_t *)(g.dist_ws + o_offq), *offr = (uint32_t *)(g.dist_ws + o_offr);
    uint32_t *loc_c = (uint32_t *)(g.dist_ws + o_lc), *loc_d = (uint32_t *)(g.dist_ws + o_ld);
    uint32_t *words = (uint32_t *)(g.dist_ws + o_words), *flags = words + 2;
    DistWork w{};
    w.cpart = g.dist_ws + o_cpart;
    w.wtot = (uint32_t *)(g.dist_ws + o_wtot);
    w.ranges = ranges;
    DistArgs all{};
    all.q = c.q; all.q_len = c.q_len; all.nq = c.nq; all.r = c.r; all.r_len = c.r_len; all.nr = c.nr; all.stride = c.stride; all.s = c.s; all.k = c.k;
    auto block_args = [&](const SearchBlock &b) {
        DistArgs x = all;
        x.q = c.q + (uint64_t)b.q0 * c.stride; x.q_len = c.q_len + b.q0; x.nq = b.nq;
        x.r = c.r + (uint64_t)b.r0 * c.stride; x.r_len = c.r_len + b.r0; x.nr = b.nr;
        x.common = loc_c; x.denom = loc_d; x.dist = nullptr; x.out_stride = kTriSlice; x.out_off = 0;
        return x;
    };
    SearchOut out{};
    out.loc_common = loc_c; out.loc_denom = loc_d; out.top = c.top; out.k = c.k; out.jmin = c.jmin;
    out.hit_ref = c.hit_ref; out.hit_common = c.hit_common; out.hit_denom = c.hit_denom; out.n_hits = c.n_hits; out.hit_dist = c.hit_dist;
    auto take_out = [&](const SearchBlock &b, const uint32_t *flag) {
        SearchOut t = out;
        t.flag = flag; t.r0 = b.r0; t.nr = b.nr; t.q0 = b.q0; t.nq = b.nq;
        return launch_search_take(t, g.stream);
    };
    hipEventRecord(g.ev0, g.stream);
    hipError_t le = hipMemsetAsync(words, 0, (size_t)(2 + 2 * group) * 4, g.stream);
    if (le == hipSuccess) le = hipMemsetAsync(c.n_hits, 0, (size_t)c.nq * 4, g.stream);
    g.last_dist_fallbacks = fast ? 0 : -1;
    g.last_dist_ranges = 0;
    if (fast && le == hipSuccess) {
        DistWork wa = w;
        wa.offs_q = offq; wa.offs_r = offr; wa.params = words; // words[0] the shift of the call, words[1] stays 0
        le = launch_dist_offsets_both(all, wa, g.stream);
    }
    std::vector<uint32_t> back;
    for (uint64_t b0 = 0; b0 < nblocks && le == hipSuccess; b0 += kBlockGroup) {
        const uint64_t b1 = std::min(nblocks, b0 + kBlockGroup);
        if (b0 != 0) le = hipMemsetAsync(flags, 0, (size_t)2 * group * 4, g.stream);
        for (uint64_t b = b0; b < b1 && le == hipSuccess; ++b) {
            const SearchBlock blk = search_block(c.nq, c.nr, qbatch, b);
            const DistArgs x = block_args(blk);
            if (!fast) {
                le = launch_dist_pairs(x, g.stream);
                if (le == hipSuccess) le = take_out(blk, words + 1);
                continue;
            }
            w.offs_q = offq + (uint64_t)blk.q0 * per;
            w.offs_r = offr + (uint64_t)blk.r0 * per;
            w.params = flags + 2 * (b - b0);
            le = launch_dist_range_pass(x, w, g.stream);
            if (le == hipSuccess) le = ranges < (uint32_t)kDistRanges ? launch_tri_finish_small(x, w, g.stream) : launch_dist_finish(x, w, g.stream);
            if (le == hipSuccess) le = take_out(blk, w.params + 1);
        }
        if (!fast || le != hipSuccess) continue;
        back.resize((size_t)(b1 - b0) * 2);
        if (hipMemcpyAsync(back.data(), flags, back.size() * 4, hipMemcpyDeviceToHost, g.stream) != hipSuccess ||
            hipStreamSynchronize(g.stream) != hipSuccess)
            return fail(MHX_E_HIP, "search kernel failed");
        for (uint64_t b = b0; b < b1 && le == hipSuccess; ++b)
            if (back[2 * (b - b0) + 1]) { // a value range overflowed the LDS table or the byte counters
                const SearchBlock blk = search_block(c.nq, c.nr, qbatch, b);
                le = launch_dist_pairs(block_args(blk), g.stream);
                if (le == hipSuccess) le = take_out(blk, words + 1);
                ++g.last_dist_fallbacks;
            }
    }
    if (le == hipSuccess && c.hit_dist) {
        SearchOut t = out;
        t.q0 = 0; t.nq = c.nq;
        le = launch_search_dist(t, g.stream);
    }
    hipEventRecord(g.ev1, g.stream);
    if (fast && (uint64_t)g.last_dist_fallbacks < nblocks) g.last_dist_ranges = (int)ranges;
    if (le != hipSuccess) return fail(MHX_E_HIP, "search kernel launch failed: %s", hipGetErrorString(le));
    const hipError_t se = hipStreamSynchronize(g.stream);
    float ms = 0.f;
    hipEventElapsedTime(&ms, g.ev0, g.ev1);
    g.last_dist_ms = ms;
    if (se != hipSuccess) return fail(MHX_E_HIP, "search kernel failed: %s", hipGetErrorString(se));
    return MHX_OK;
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
    for (uint32_t i = 0; i < nq; ++i) if (q_len[i] > stride) return fail(MHX_E_ARG, "q_len[%u] exceeds stride", i);
    if (!refs) for (uint32_t i = 0; i < nr; ++i) if (r_len[i] > stride) return fail(MHX_E_ARG, "r_len[%u] exceeds stride", i);
    const size_t bq = up256((size_t)nq * stride * 8), bql = up256((size_t)nq * 4), bh = up256((size_t)nq * top * 4);
    const size_t br = refs ? 0 : up256((size_t)nr * stride * 8), brl = refs ? 0 : up256((size_t)nr * 4);
    uint8_t *base = nullptr;
    int rc = dist_stage(bq + bql + br + brl + 3 * bh + bql, &base);
    if (rc) return rc;
    uint8_t *dq = base, *dql = dq + bq, *dr = dql + bql, *drl = dr + br, *dh = drl + brl;
    hipError_t ce = hipSuccess;
    if (q_rows) { // every row from its own place
        for (uint32_t i = 0; i < nq && ce == hipSuccess; ++i)
            if (q_len[i]) ce = hipMemcpyAsync(dq + (size_t)i * stride * 8, q_rows[i], (size_t)q_len[i] * 8, hipMemcpyHostToDevice, g.stream);
    } else
        ce = hipMemcpyAsync(dq, q, (size_t)nq * stride * 8, hipMemcpyHostToDevice, g.stream);
    if (ce == hipSuccess) ce = hipMemcpyAsync(dql, q_len, (size_t)nq * 4, hipMemcpyHostToDevice, g.stream);
    if (!refs && ce == hipSuccess) ce = hipMemcpyAsync(dr, r, (size_t)nr * stride * 8, hipMemcpyHostToDevice, g.stream);
    if (!refs && ce == hipSuccess) ce = hipMemcpyAsync(drl, r_len, (size_t)nr * 4, hipMemcpyHostToDevice, g.stream);
    if (ce != hipSuccess) return fail(MHX_E_HIP, "H2D copy failed in dist_search: %s", hipGetErrorString(ce));
    SearchCall c{};
    c.q = (const uint64_t *)dq; c.q_len = (const uint32_t *)dql;
    c.r = refs ? refs->rows : (const uint64_t *)dr; c.r_len = refs ? refs->len : (const uint32_t *)drl;
    c.nq = nq; c.nr = nr; c.stride = stride; c.s = s; c.k = k; c.top = top;
    c.longest = refs ? refs->longest : 0;
    for (uint32_t i = 0; i < nq; ++i) c.longest = std::max(c.longest, q_len[i]);
    if (!refs) for (uint32_t i = 0; i < nr; ++i) c.longest = std::max(c.longest, r_len[i]);
    c.jmin = tri_jmin(max_dist, k);
    c.hit_ref = (uint32_t *)dh; c.hit_common = (uint32_t *)(dh + bh); c.hit_denom = (uint32_t *)(dh + 2 * bh); c.n_hits = (uint32_t *)(dh + 3 * bh);
    c.hit_dist = nullptr; // distances in host libm below
    if (staged) *staged = SearchStaged{c.q, c.q_len};
    rc = search_device(c);
    if (rc) return rc;
    const size_t cells = (size_t)nq * top;
    if (hipMemcpy(hit_ref, c.hit_ref, cells * 4, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(hit_common, c.hit_common, cells * 4, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(hit_denom, c.hit_denom, cells * 4, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(n_hits, c.n_hits, (size_t)nq * 4, hipMemcpyDeviceToHost) != hipSuccess)
        return fail(MHX_E_HIP, "D2H copy failed in dist_search");
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
