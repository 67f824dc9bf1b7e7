// mhx_engine_within.cpp -- host side of the bounded neighbourhood call (mhx_dist_within: all references within a distance of
// each query, as CSR): the cmin table of the bound, staging of a host-pointer call, the search's schedule (ONE split of both
// sets into value ranges, blocks of (query batch, reference slice), the fallback of a flagged block to the generic pair
// kernel) inside super-batches of queries, and behind the last block of each the scan and the gather.
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
#include "mhx_engine_internal.h"
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

size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

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

// Launches the whole call on the engine's stream and waits for it.  Geometry, the one split of both sets and the blocks with
// their flag words and their fallback are search_device's; the queries go through in super-batches (mhx_within.h) whose cells
// live in g.within_ws, and behind the last block and the last fallback of a super-batch its cells are scanned into row_off
// and its arrival list is gathered into the call's outputs.  A block that is redone later fills the same cells, so neither
// the order of the blocks nor the batch sizes show in the result.
int within_device(WithinCall &c)
{
    const uint32_t *cmin = nullptr;
    int rc = within_cmin(c.s, c.k, c.max_dist, &cmin);
    if (rc) return rc;
    const uint64_t pairs = (uint64_t)c.nq * c.nr;
    const char *geo = getenv("MHX_WITHIN_GEOMETRY");
    const uint32_t ranges = geo && strcmp(geo, "dist") == 0 ? tri_ranges_dist(c.longest) : tri_ranges(c.longest);
    const bool fast = (pairs >= 64 || (pairs >= 8 && pairs * (uint64_t)c.s >= 400000)) && ranges != 0 && getenv("MHX_DIST_GENERIC") == nullptr;
    uint64_t cells = kWithinCells;
    if (const char *e = getenv("MHX_WITHIN_CELLS")) { const long long v = atoll(e); if (v > 0 && (uint64_t)v < cells) cells = (uint64_t)v; }
    const uint32_t nslices = within_slices(c.nr), super = within_super_queries(c.nq, c.nr, cells);
    uint32_t qbatch = tri_max_queries(fast ? ranges : kTriMinRanges);
    if (const char *e = getenv("MHX_WITHIN_QBATCH")) { const long v = atol(e); if (v > 0 && (uint64_t)v < qbatch) qbatch = (uint32_t)v; }
    qbatch = std::min(qbatch, super);
    const bool store = c.hit_ref != nullptr && c.cap != 0;
    // the arrival list of a super-batch: its hits are at most its pairs (below 2^32: kWithinCells x 32, or one row of the
    // references), and what lies beyond the room the caller gave is only counted
    const uint32_t room = store ? (uint32_t)std::min<uint64_t>(c.cap, (uint64_t)super * c.nr) : 0;
    constexpr uint64_t kBlockGroup = 4096; // blocks whose flag words come back together
    const uint64_t most_blocks = search_blocks(super, c.nr, qbatch);
    const uint32_t group = (uint32_t)std::min(most_blocks, kBlockGroup);
    // workspace of the passes, as the search's: [offsets of the queries][offsets of the references][byte counters][window
    // totals][block-local common, denom][words: shift, 0, then two per block of a group]
    const uint64_t per = (uint64_t)ranges + 1;
    size_t o = 0;
    const size_t o_offq = o; if (fast) o += up256((size_t)c.nq * per * 4);
    const size_t o_offr = o; if (fast) o += up256((size_t)c.nr * per * 4);
    const size_t o_cpart = o; if (fast) o += up256((size_t)qbatch * ranges * kTriSlice);
    const size_t o_wtot = o; if (fast && ranges > (uint32_t)kDistRanges) o += up256((size_t)qbatch * (ranges / kDistWindowRanges) * kTriSlice * 4);
    const size_t o_lc = o; o += up256((size_t)qbatch * kTriSlice * 4);
    const size_t o_ld = o; o += up256((size_t)qbatch * kTriSlice * 4);
    const size_t o_words = o; o += up256((size_t)(2 + 2 * group) * 4);
    if (g.dist_ws.grow(o, g.stream) != hipSuccess) return fail(MHX_E_HIP, "hipMalloc failed for the workspace of dist_within (%zu bytes)", o);
    // the cells of a super-batch: [mask][base][arrival counter][arrival common][arrival denom]
    const size_t b_cells = up256((size_t)super * nslices * 4), b_arr = up256((size_t)room * 4);
    const size_t need = b_cells + (store ? b_cells : 0) + 256 + 2 * b_arr;
    if (g.within_ws.grow(need, g.stream) != hipSuccess) return fail(MHX_E_HIP, "hipMalloc failed for the cells of dist_within (%zu bytes)", need);
    uint32_t *mask = (uint32_t *)(uint8_t *)g.within_ws, *base = store ? (uint32_t *)(g.within_ws + b_cells) : nullptr;
    uint32_t *count = (uint32_t *)(g.within_ws + b_cells + (store ? b_cells : 0));
    uint32_t *arr_c = (uint32_t *)((uint8_t *)count + 256), *arr_d = (uint32_t *)((uint8_t *)count + 256 + b_arr);
    uint32_t *offq = (uint32_t *)(g.dist_ws + o_offq), *offr = (uint32_t *)(g.dist_ws + o_offr);
    uint32_t *loc_c = (uint32_t *)(g.dist_ws + o_lc), *loc_d = (uint32_t *)(g.dist_ws + o_ld);
    uint32_t *words = (uint32_t *)(g.dist_ws + o_words), *flags = words + 2;
    DistWork w{};
    w.cpart = g.dist_ws + o_cpart;
    w.wtot = (uint32_t *)(g.dist_ws + o_wtot);
    w.ranges = ranges;
    DistArgs all{};
    all.q = c.q; all.q_len = c.q_len; all.nq = c.nq; all.r = c.r; all.r_len = c.r_len; all.nr = c.nr; all.stride = c.stride; all.s = c.s; all.k = c.k;
    WithinOut out{};
    out.loc_common = loc_c; out.loc_denom = loc_d; out.cmin = cmin; out.s = c.s; out.nslices = nslices; out.mask = mask; out.base = base;
    out.arr_common = arr_c; out.arr_denom = arr_d; out.room = room; out.count = count;
    hipEventRecord(g.ev0, g.stream);
    hipError_t le = hipMemsetAsync(words, 0, (size_t)(2 + 2 * group) * 4, g.stream);
    if (le == hipSuccess) le = hipMemsetAsync(c.row_off, 0, 8, g.stream);
    g.last_dist_fallbacks = fast ? 0 : -1;
    g.last_dist_ranges = 0;
    if (fast && le == hipSuccess) {
        DistWork wa = w;
        wa.offs_q = offq; wa.offs_r = offr; wa.params = words; // words[0] the shift of the call, words[1] stays 0
        le = launch_dist_offsets_both(all, wa, g.stream);
    }
    std::vector<uint32_t> back;
    uint64_t nblocks_all = 0;
    for (uint32_t s0 = 0; s0 < c.nq && le == hipSuccess; s0 += super) {
        const uint32_t snq = std::min(super, c.nq - s0);
        const uint64_t nblocks = search_blocks(snq, c.nr, qbatch);
        nblocks_all += nblocks;
        auto block_args = [&](const SearchBlock &b) {
            DistArgs x = all;
            x.q = c.q + (uint64_t)(s0 + b.q0) * c.stride; x.q_len = c.q_len + s0 + b.q0; x.nq = b.nq;
            x.r = c.r + (uint64_t)b.r0 * c.stride; x.r_len = c.r_len + b.r0; x.nr = b.nr;
            x.common = loc_c; x.denom = loc_d; x.dist = nullptr; x.out_stride = kTriSlice; x.out_off = 0;
            return x;
        };
        auto take_out = [&](const SearchBlock &b, const uint32_t *flag) {
            WithinOut t = out;
            t.flag = flag; t.r0 = b.r0; t.nr = b.nr; t.q0 = b.q0; t.nq = b.nq;
            return launch_within_take(t, g.stream);
        };
        le = hipMemsetAsync(mask, 0, (size_t)snq * nslices * 4, g.stream);
        if (le == hipSuccess) le = hipMemsetAsync(count, 0, 4, g.stream);
        for (uint64_t b0 = 0; b0 < nblocks && le == hipSuccess; b0 += kBlockGroup) {
            const uint64_t b1 = std::min(nblocks, b0 + kBlockGroup);
            if (fast) le = hipMemsetAsync(flags, 0, (size_t)2 * group * 4, g.stream);
            for (uint64_t b = b0; b < b1 && le == hipSuccess; ++b) {
                const SearchBlock blk = search_block(snq, c.nr, qbatch, b);
                const DistArgs x = block_args(blk);
                if (!fast) {
                    le = launch_dist_pairs(x, g.stream);
                    if (le == hipSuccess) le = take_out(blk, words + 1);
                    continue;
                }
                w.offs_q = offq + (uint64_t)(s0 + blk.q0) * per;
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
                return fail(MHX_E_HIP, "dist_within kernel failed");
            for (uint64_t b = b0; b < b1 && le == hipSuccess; ++b)
                if (back[2 * (b - b0) + 1]) { // a value range overflowed the LDS table or the byte counters
                    const SearchBlock blk = search_block(snq, c.nr, qbatch, b);
                    le = launch_dist_pairs(block_args(blk), g.stream);
                    if (le == hipSuccess) le = take_out(blk, words + 1);
                    ++g.last_dist_fallbacks;
                }
        }
        if (le != hipSuccess) break;
        WithinRows rows{};
        rows.mask = mask; rows.base = base; rows.nq = snq; rows.nslices = nslices; rows.row_off = c.row_off + s0;
        rows.arr_common = arr_c; rows.arr_denom = arr_d; rows.room = room;
        rows.hit_ref = c.hit_ref; rows.hit_common = c.hit_common; rows.hit_denom = c.hit_denom; rows.hit_dist = c.hit_dist; rows.cap = store ? c.cap : 0; rows.k = c.k;
        le = launch_within_scan(rows, g.stream);
        if (le == hipSuccess) le = launch_within_gather(rows, g.stream);
    }
    hipEventRecord(g.ev1, g.stream);
    if (fast && (uint64_t)g.last_dist_fallbacks < nblocks_all) g.last_dist_ranges = (int)ranges;
    if (le != hipSuccess) return fail(MHX_E_HIP, "dist_within kernel launch failed: %s", hipGetErrorString(le));
    hipError_t se = hipMemcpyAsync(c.n_out, c.row_off + c.nq, 8, hipMemcpyDeviceToHost, g.stream);
    if (se == hipSuccess) se = hipStreamSynchronize(g.stream);
    float ms = 0.f;
    hipEventElapsedTime(&ms, g.ev0, g.ev1);
    g.last_dist_ms = ms;
    if (se != hipSuccess) return fail(MHX_E_HIP, "dist_within kernel failed: %s", hipGetErrorString(se));
    return MHX_OK;
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
    for (uint32_t i = 0; i < nq; ++i) if (q_len[i] > stride) return fail(MHX_E_ARG, "q_len[%u] exceeds stride", i);
    if (!refs) for (uint32_t i = 0; i < nr; ++i) if (r_len[i] > stride) return fail(MHX_E_ARG, "r_len[%u] exceeds stride", i);
    const uint64_t room = hit_ref ? std::min<uint64_t>(cap, (uint64_t)nq * nr) : 0;
    const size_t bq = up256((size_t)nq * stride * 8), bql = up256((size_t)nq * 4), bo = up256(((size_t)nq + 1) * 8), bh = up256((size_t)room * 4);
    const size_t br = refs ? 0 : up256((size_t)nr * stride * 8), brl = refs ? 0 : up256((size_t)nr * 4);
    uint8_t *base = nullptr;
    int rc = dist_stage(bq + bql + br + brl + bo + 3 * bh, &base);
    if (rc) return rc;
    uint8_t *dq = base, *dql = dq + bq, *dr = dql + bql, *drl = dr + br, *doff = drl + brl, *dh = doff + bo;
    hipError_t ce = hipSuccess;
    if (q_rows) { // every row from its own place
        for (uint32_t i = 0; i < nq && ce == hipSuccess; ++i)
            if (q_len[i]) ce = hipMemcpyAsync(dq + (size_t)i * stride * 8, q_rows[i], (size_t)q_len[i] * 8, hipMemcpyHostToDevice, g.stream);
    } else
        ce = hipMemcpyAsync(dq, q, (size_t)nq * stride * 8, hipMemcpyHostToDevice, g.stream);
    if (ce == hipSuccess) ce = hipMemcpyAsync(dql, q_len, (size_t)nq * 4, hipMemcpyHostToDevice, g.stream);
    if (!refs && ce == hipSuccess) ce = hipMemcpyAsync(dr, r, (size_t)nr * stride * 8, hipMemcpyHostToDevice, g.stream);
    if (!refs && ce == hipSuccess) ce = hipMemcpyAsync(drl, r_len, (size_t)nr * 4, hipMemcpyHostToDevice, g.stream);
    if (ce != hipSuccess) return fail(MHX_E_HIP, "H2D copy failed in dist_within: %s", hipGetErrorString(ce));
    WithinCall c{};
    c.q = (const uint64_t *)dq; c.q_len = (const uint32_t *)dql;
    c.r = refs ? refs->rows : (const uint64_t *)dr; c.r_len = refs ? refs->len : (const uint32_t *)drl;
    c.nq = nq; c.nr = nr; c.stride = stride; c.s = s; c.k = k; c.max_dist = max_dist;
    c.longest = refs ? refs->longest : 0;
    for (uint32_t i = 0; i < nq; ++i) c.longest = std::max(c.longest, q_len[i]);
    if (!refs) for (uint32_t i = 0; i < nr; ++i) c.longest = std::max(c.longest, r_len[i]);
    c.row_off = (uint64_t *)doff;
    if (room) { c.hit_ref = (uint32_t *)dh; c.hit_common = (uint32_t *)(dh + bh); c.hit_denom = (uint32_t *)(dh + 2 * bh); }
    c.hit_dist = nullptr; // distances in host libm below
    c.cap = room;
    c.n_out = n_out;
    rc = within_device(c);
    if (rc) return rc;
    if (hipMemcpy(row_off, c.row_off, ((size_t)nq + 1) * 8, hipMemcpyDeviceToHost) != hipSuccess) return fail(MHX_E_HIP, "D2H copy failed in dist_within");
    if (!hit_ref && cap == 0) return MHX_OK; // the counting form
    const uint64_t m = *n_out;
    if (m > cap) return too_small(m);
    if (m && (hipMemcpy(hit_ref, c.hit_ref, m * 4, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(hit_common, c.hit_common, m * 4, hipMemcpyDeviceToHost) != hipSuccess ||
              hipMemcpy(hit_denom, c.hit_denom, m * 4, hipMemcpyDeviceToHost) != hipSuccess))
        return fail(MHX_E_HIP, "D2H copy failed in dist_within");
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
