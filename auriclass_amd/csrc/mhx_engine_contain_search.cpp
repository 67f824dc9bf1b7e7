// mhx_engine_contain_search.cpp -- host side of the containment search (mhx_dist_contain_search): staging of a host-pointer
// call, the need[] table of the identity bound, the schedule of contain_device (mhx_engine_contain.cpp: bounds, ONE split of
// both sets, (query batch, reference slice) blocks, the range pass, flags read back per group of blocks) with the finish pass
// and the pair kernel writing block-local and a take-out pass behind every block, as search_device (mhx_engine_search.cpp)
// has it.  Rules: mhx_contain_search.h and mhx_contain.h; kernels: mhx_contain_search.hip, mhx_contain.hip and mhx_dist.hip.
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "mhx_device.h"
#include "mhx_contain_search.h"
#include "mhx_engine_internal.h"
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

size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

// The need table of the last call stays in the engine state, on the host, like the workspace it goes into: a bound between 0
// and 1 costs about three pow per entry (some milliseconds at 50 000 entries), and the batches of a file-level call, or a
// caller that searches set after set, ask for the same table again.  A call with another bound builds it anew.
const uint32_t *need_table(uint32_t limit, int k, double min_identity, uint32_t min_shared)
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

// Launches the whole call on the engine's stream and waits for it.  Every block runs the range pass and the containment's
// finish pass into its block-local [queries][32] counts, and the take-out pass merges them into the best lists, which are
// the outputs themselves and stay in device memory between the blocks.  Block flags come back once per group of blocks; a
// flagged block is redone by the pair kernel into the same block-local arrays and taken out then -- later than its
// neighbours, which the total order makes harmless.  Nothing of size nq x nr exists.
int contain_search_device(ContainSearchCall &c)
{
    const uint64_t pairs = (uint64_t)c.nq * c.nr;
    const uint32_t ranges = contain_ranges(c.longest);
    const bool fast = (pairs >= 64 || (pairs >= 8 && pairs * (uint64_t)c.longest >= 400000)) && ranges != 0 && getenv("MHX_DIST_GENERIC") == nullptr;
    uint32_t qbatch = tri_max_queries(fast ? ranges : kTriMinRanges);
    if (const char *e = getenv("MHX_SEARCH_QBATCH")) { const long v = atol(e); if (v > 0 && (uint64_t)v < qbatch) qbatch = (uint32_t)v; }
    qbatch = std::min(qbatch, c.nq);
    const uint64_t nblocks = search_blocks(c.nq, c.nr, qbatch);
    constexpr uint64_t kBlockGroup = 4096; // blocks whose flag words come back together
    const uint32_t group = (uint32_t)std::min(nblocks, kBlockGroup);
    // workspace: [effective lengths and bounds of both sets][offsets of the queries][offsets of the references][byte
    // counters][block-local shared, n_qry, n_ref][need][words: shift, 0, then two per block of a group]
    const uint64_t per = (uint64_t)ranges + 1;
    size_t o = 0;
    const size_t o_bq = o; o += up256((size_t)c.nq * 8);
    const size_t o_br = o; o += up256((size_t)c.nr * 8);
    const size_t o_eq = o; o += up256((size_t)c.nq * 4);
    const size_t o_er = o; o += up256((size_t)c.nr * 4);
    const size_t o_offq = o; if (fast) o += up256((size_t)c.nq * per * 4);
    const size_t o_offr = o; if (fast) o += up256((size_t)c.nr * per * 4);
    const size_t o_cpart = o; if (fast) o += up256((size_t)qbatch * ranges * kTriSlice);
    const size_t b_loc = up256((size_t)qbatch * kTriSlice * 4);
    const size_t o_loc = o; o += 3 * b_loc;
    const size_t o_need = o; o += up256(((size_t)c.need_limit + 1) * 4);
    const size_t o_words = o; o += up256((size_t)(2 + 2 * group) * 4);
    if (g.dist_ws.grow(o, g.stream) != hipSuccess) return fail(MHX_E_HIP, "hipMalloc failed for the containment search workspace (%zu bytes)", o);
    uint32_t *offq = (uint32_t *)(g.dist_ws + o_offq), *offr = (uint32_t *)(g.dist_ws + o_offr);
    uint32_t *loc_s = (uint32_t *)(g.dist_ws + o_loc), *loc_q = (uint32_t *)(g.dist_ws + o_loc + b_loc), *loc_r = (uint32_t *)(g.dist_ws + o_loc + 2 * b_loc);
    uint32_t *need = (uint32_t *)(g.dist_ws + o_need);
    uint32_t *words = (uint32_t *)(g.dist_ws + o_words), *flags = words + 2;
    // the table goes over before anything is queued, with a blocking copy: like the host's build of it, this lies before the
    // first event, so mhx_last_dist_kernel_ms does not hold it (tools/contain_search_rate.py times the whole call as well)
    if (hipMemcpy(need, c.need, ((size_t)c.need_limit + 1) * 4, hipMemcpyHostToDevice) != hipSuccess) return fail(MHX_E_HIP, "H2D copy of the need table failed");
    ContainArgs all{};
    all.q = c.q; all.q_len = c.q_len; all.nq = c.nq; all.r = c.r; all.r_len = c.r_len; all.nr = c.nr; all.stride = c.stride; all.s_q = c.s_q; all.s_r = c.s_r;
    all.q_bound = (uint64_t *)(g.dist_ws + o_bq); all.r_bound = (uint64_t *)(g.dist_ws + o_br);
    all.q_eff = (uint32_t *)(g.dist_ws + o_eq); all.r_eff = (uint32_t *)(g.dist_ws + o_er);
    all.shift = words;
    all.shared = loc_s; all.n_qry = loc_q; all.n_ref = loc_r; all.out_stride = kTriSlice;
    auto block_args = [&](const SearchBlock &b) { // cell (q, r) of the block lies at (q - q0) * 32 + (r - r0)
        ContainArgs x = all;
        x.q0 = b.q0; x.bnq = b.nq; x.r0 = b.r0; x.bnr = b.nr;
        x.out_base = (uint64_t)b.q0 * kTriSlice + b.r0;
        return x;
    };
    ContainSearchOut out{};
    out.loc_shared = loc_s; out.loc_n_qry = loc_q; out.loc_n_ref = loc_r; out.top = c.top; out.need = need; out.need_limit = c.need_limit;
    out.hit_ref = c.hit_ref; out.hit_shared = c.hit_shared; out.hit_n_ref = c.hit_n_ref; out.hit_n_qry = c.hit_n_qry; out.n_hits = c.n_hits;
    auto take_out = [&](const SearchBlock &b, const uint32_t *flag) {
        ContainSearchOut t = out;
        t.flag = flag; t.r0 = b.r0; t.nr = b.nr; t.q0 = b.q0; t.nq = b.nq;
        return launch_contain_take(t, g.stream);
    };
    // the passes of mhx_dist.hip see the effective lengths: what lies behind them in a row is not part of a list
    DistArgs lists{};
    lists.q = c.q; lists.q_len = all.q_eff; lists.nq = c.nq; lists.r = c.r; lists.r_len = all.r_eff; lists.nr = c.nr; lists.stride = c.stride;
    DistWork w{};
    w.cpart = g.dist_ws + o_cpart;
    w.ranges = ranges;
    hipEventRecord(g.ev0, g.stream);
    hipError_t le = hipMemsetAsync(words, 0, (size_t)(2 + 2 * group) * 4, g.stream);
    if (le == hipSuccess) le = hipMemsetAsync(c.n_hits, 0, (size_t)c.nq * 4, g.stream);
    if (le == hipSuccess) le = launch_contain_bounds(all, g.stream);
    g.last_dist_fallbacks = fast ? 0 : -1;
    g.last_dist_ranges = 0;
    if (fast && le == hipSuccess) {
        DistWork wa = w;
        wa.offs_q = offq; wa.offs_r = offr; wa.params = words; // words[0] the shift of the call, words[1] stays 0
        le = launch_dist_offsets_both(lists, wa, g.stream);
    }
    std::vector<uint32_t> back;
    for (uint64_t b0 = 0; b0 < nblocks && le == hipSuccess; b0 += kBlockGroup) {
        const uint64_t b1 = std::min(nblocks, b0 + kBlockGroup);
        if (b0 != 0) le = hipMemsetAsync(flags, 0, (size_t)2 * group * 4, g.stream);
        for (uint64_t b = b0; b < b1 && le == hipSuccess; ++b) {
            const SearchBlock blk = search_block(c.nq, c.nr, qbatch, b);
            const ContainArgs a = block_args(blk);
            if (!fast) {
                le = launch_contain_pairs(a, g.stream);
                if (le == hipSuccess) le = take_out(blk, words + 1);
                continue;
            }
            DistArgs x = lists;
            x.q = c.q + (uint64_t)blk.q0 * c.stride; x.q_len = all.q_eff + blk.q0; x.nq = blk.nq;
            x.r = c.r + (uint64_t)blk.r0 * c.stride; x.r_len = all.r_eff + blk.r0; x.nr = blk.nr;
            w.offs_q = offq + (uint64_t)blk.q0 * per;
            w.offs_r = offr + (uint64_t)blk.r0 * per;
            w.params = flags + 2 * (b - b0);
            le = launch_dist_range_pass(x, w, g.stream);
            if (le == hipSuccess) le = launch_contain_finish(a, w, g.stream);
            if (le == hipSuccess) le = take_out(blk, w.params + 1);
        }
        if (!fast || le != hipSuccess) continue;
        back.resize((size_t)(b1 - b0) * 2);
        if (hipMemcpyAsync(back.data(), flags, back.size() * 4, hipMemcpyDeviceToHost, g.stream) != hipSuccess ||
            hipStreamSynchronize(g.stream) != hipSuccess)
            return fail(MHX_E_HIP, "containment search kernel failed");
        for (uint64_t b = b0; b < b1 && le == hipSuccess; ++b)
            if (back[2 * (b - b0) + 1]) { // a value range overflowed the LDS table or the byte counters: finish and take-out did nothing
                const SearchBlock blk = search_block(c.nq, c.nr, qbatch, b);
                le = launch_contain_pairs(block_args(blk), g.stream);
                if (le == hipSuccess) le = take_out(blk, words + 1);
                ++g.last_dist_fallbacks;
            }
    }
    hipEventRecord(g.ev1, g.stream);
    if (fast && (uint64_t)g.last_dist_fallbacks < nblocks) g.last_dist_ranges = (int)ranges;
    if (le != hipSuccess) return fail(MHX_E_HIP, "containment search kernel launch failed: %s", hipGetErrorString(le));
    const hipError_t se = hipStreamSynchronize(g.stream);
    float ms = 0.f;
    hipEventElapsedTime(&ms, g.ev0, g.ev1);
    g.last_dist_ms = ms;
    if (se != hipSuccess) return fail(MHX_E_HIP, "containment search kernel failed: %s", hipGetErrorString(se));
    return MHX_OK;
}

int contain_search_check(uint32_t s_q, uint32_t s_r, uint32_t stride, int k, double min_identity, uint32_t min_shared, uint32_t top)
{
    if (top < 1 || top > kSearchMaxTop) return fail(MHX_E_ARG, "top must be 1 .. %u", kSearchMaxTop);
    if (min_shared == 0) return fail(MHX_E_ARG, "min_shared must be at least 1");
    if (!(min_identity == min_identity)) return fail(MHX_E_ARG, "min_identity is not a number");
    if (k < 1 || k > 32) return fail(MHX_E_ARG, "bad k");
    if (s_q == 0 || s_r == 0 || stride == 0) return fail(MHX_E_ARG, "bad s_q / s_r / stride");
    return MHX_OK;
}

// Host queries against references that are on the device already (refs) or on the host (r / r_len, refs null).  The lists
// the device leaves are the result: the hit test is exact there.  Staging holds the rows, the lengths and the [nq][top] lists.
int contain_search_host(const uint64_t *q, const uint64_t *const *q_rows, const uint32_t *q_len, uint32_t nq, uint32_t s_q, const uint64_t *r,
                        const uint32_t *r_len, const SearchRefs *refs, uint32_t nr, uint32_t s_r, uint32_t stride, int k, double min_identity,
                        uint32_t min_shared, uint32_t top, uint32_t *hit_ref, uint32_t *hit_shared, uint32_t *hit_n_ref, uint32_t *hit_n_qry, uint32_t *n_hits)
{
    for (uint32_t i = 0; i < nq; ++i) if (q_len[i] > stride) return fail(MHX_E_ARG, "q_len[%u] exceeds stride", i);
    if (!refs) for (uint32_t i = 0; i < nr; ++i) if (r_len[i] > stride) return fail(MHX_E_ARG, "r_len[%u] exceeds stride", i);
    const size_t bq = up256((size_t)nq * stride * 8), bql = up256((size_t)nq * 4), bh = up256((size_t)nq * top * 4);
    const size_t br = refs ? 0 : up256((size_t)nr * stride * 8), brl = refs ? 0 : up256((size_t)nr * 4);
    uint8_t *base = nullptr;
    int rc = dist_stage(bq + bql + br + brl + 4 * bh + bql, &base);
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
    if (ce != hipSuccess) return fail(MHX_E_HIP, "H2D copy failed in dist_contain_search: %s", hipGetErrorString(ce));
    ContainSearchCall c{};
    c.q = (const uint64_t *)dq; c.q_len = (const uint32_t *)dql;
    c.r = refs ? refs->rows : (const uint64_t *)dr; c.r_len = refs ? refs->len : (const uint32_t *)drl;
    c.nq = nq; c.nr = nr; c.stride = stride; c.s_q = s_q; c.s_r = s_r; c.top = top;
    c.longest = refs ? contain_eff_len(refs->longest, stride, s_r) : 0;
    for (uint32_t i = 0; i < nq; ++i) c.longest = std::max(c.longest, contain_eff_len(q_len[i], stride, s_q));
    if (!refs) for (uint32_t i = 0; i < nr; ++i) c.longest = std::max(c.longest, contain_eff_len(r_len[i], stride, s_r));
    c.need_limit = std::min(stride, s_r);
    c.need = need_table(c.need_limit, k, min_identity, min_shared);
    c.hit_ref = (uint32_t *)dh; c.hit_shared = (uint32_t *)(dh + bh); c.hit_n_ref = (uint32_t *)(dh + 2 * bh); c.hit_n_qry = (uint32_t *)(dh + 3 * bh);
    c.n_hits = (uint32_t *)(dh + 4 * bh);
    rc = contain_search_device(c);
    if (rc) return rc;
    const size_t cells = (size_t)nq * top;
    if (hipMemcpy(hit_ref, c.hit_ref, cells * 4, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(hit_shared, c.hit_shared, cells * 4, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(hit_n_ref, c.hit_n_ref, cells * 4, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(hit_n_qry, c.hit_n_qry, cells * 4, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(n_hits, c.n_hits, (size_t)nq * 4, hipMemcpyDeviceToHost) != hipSuccess)
        return fail(MHX_E_HIP, "D2H copy failed in dist_contain_search");
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
        c.need = need_table(c.need_limit, k, min_identity, min_shared);
        c.hit_ref = hit_ref; c.hit_shared = hit_shared; c.hit_n_ref = hit_n_ref; c.hit_n_qry = hit_n_qry; c.n_hits = n_hits;
        return contain_search_device(c);
    });
}
