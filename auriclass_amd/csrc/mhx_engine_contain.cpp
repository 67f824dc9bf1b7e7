// mhx_engine_contain.cpp -- host side of the containment of reference sketches in query sketches (mhx_dist_contain): staging
// of a host-pointer call, the bounds of every list, ONE split of both sets into value ranges, the search's schedule of (query
// batch, reference slice) blocks with a finish pass that writes straight into the outputs, and the fallback of a flagged
// block to the generic pair kernel.  Rules: mhx_contain.h; kernels: mhx_contain.hip and the passes of mhx_dist.hip.
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
#include "mhx_engine_internal.h"
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

size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

// Launches the whole call on the engine's stream and waits for it: the schedule of search_device (mhx_engine_search.cpp)
// without its block-local arrays and its take-out pass.
int contain_device(ContainCall &c)
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
    // counters][words: shift, 0, then two per block of a group]
    const uint64_t per = (uint64_t)ranges + 1;
    size_t o = 0;
    const size_t o_bq = o; o += up256((size_t)c.nq * 8);
    const size_t o_br = o; o += up256((size_t)c.nr * 8);
    const size_t o_eq = o; o += up256((size_t)c.nq * 4);
    const size_t o_er = o; o += up256((size_t)c.nr * 4);
    const size_t o_offq = o; if (fast) o += up256((size_t)c.nq * per * 4);
    const size_t o_offr = o; if (fast) o += up256((size_t)c.nr * per * 4);
    const size_t o_cpart = o; if (fast) o += up256((size_t)qbatch * ranges * kTriSlice);
    const size_t o_words = o; o += up256((size_t)(2 + 2 * group) * 4);
    // winner-take-all: a winner word per (query of a batch, position in its list), and the counter of the pairs walked
    const uint32_t width = std::min(c.stride, c.s_q);
    const size_t o_win = o; if (c.won) o += up256((size_t)qbatch * width * 4);
    const size_t o_count = o; if (c.won) o += 256;
    if (g.dist_ws.grow(o, g.stream) != hipSuccess) return fail(MHX_E_HIP, "hipMalloc failed for the containment workspace (%zu bytes)", o);
    uint32_t *offq = (uint32_t *)(g.dist_ws + o_offq), *offr = (uint32_t *)(g.dist_ws + o_offr);
    uint32_t *words = (uint32_t *)(g.dist_ws + o_words), *flags = words + 2;
    ContainArgs all{};
    all.q = c.q; all.q_len = c.q_len; all.nq = c.nq; all.r = c.r; all.r_len = c.r_len; all.nr = c.nr; all.stride = c.stride; all.s_q = c.s_q; all.s_r = c.s_r;
    all.q_bound = (uint64_t *)(g.dist_ws + o_bq); all.r_bound = (uint64_t *)(g.dist_ws + o_br);
    all.q_eff = (uint32_t *)(g.dist_ws + o_eq); all.r_eff = (uint32_t *)(g.dist_ws + o_er);
    all.shift = words;
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
    DistWork w{};
    w.cpart = g.dist_ws + o_cpart;
    w.ranges = ranges;
    hipEventRecord(g.ev0, g.stream);
    hipError_t le = hipMemsetAsync(words, 0, (size_t)(2 + 2 * group) * 4, g.stream);
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
            if (!fast) { le = launch_contain_pairs(block_args(blk), g.stream); continue; }
            DistArgs x = lists;
            x.q = c.q + (uint64_t)blk.q0 * c.stride; x.q_len = all.q_eff + blk.q0; x.nq = blk.nq;
            x.r = c.r + (uint64_t)blk.r0 * c.stride; x.r_len = all.r_eff + blk.r0; x.nr = blk.nr;
            w.offs_q = offq + (uint64_t)blk.q0 * per;
            w.offs_r = offr + (uint64_t)blk.r0 * per;
            w.params = flags + 2 * (b - b0);
            le = launch_dist_range_pass(x, w, g.stream);
            if (le == hipSuccess) le = launch_contain_finish(block_args(blk), w, g.stream);
        }
        if (!fast || le != hipSuccess) continue;
        back.resize((size_t)(b1 - b0) * 2);
        if (hipMemcpyAsync(back.data(), flags, back.size() * 4, hipMemcpyDeviceToHost, g.stream) != hipSuccess ||
            hipStreamSynchronize(g.stream) != hipSuccess)
            return fail(MHX_E_HIP, "containment kernel failed");
        for (uint64_t b = b0; b < b1 && le == hipSuccess; ++b)
            if (back[2 * (b - b0) + 1]) { // a value range overflowed the LDS table or the byte counters: the finish pass did nothing
                le = launch_contain_pairs(block_args(search_block(c.nq, c.nr, qbatch, b)), g.stream);
                ++g.last_dist_fallbacks;
            }
    }
    // The plain pass of every block is queued.  Winner-take-all: per query batch, over ALL references, zero the batch's words,
    // let every pair that shares something propose, and count what every reference holds at the end.
    if (c.won && le == hipSuccess) {
        ContainWinnerArgs wa{(uint32_t *)(g.dist_ws + o_win), width, c.ref_length, c.won, (unsigned long long *)(g.dist_ws + o_count)};
        le = hipMemsetAsync(c.won, 0, (size_t)pairs * 4, g.stream);
        if (le == hipSuccess) le = hipMemsetAsync(wa.pairs, 0, 8, g.stream);
        for (uint32_t q0 = 0; q0 < c.nq && le == hipSuccess; q0 += qbatch) {
            ContainArgs x = all;
            x.q0 = q0; x.bnq = std::min(qbatch, c.nq - q0); x.r0 = 0; x.bnr = c.nr;
            le = hipMemsetAsync(wa.words, 0, (size_t)x.bnq * width * 4, g.stream);
            if (le == hipSuccess) le = launch_contain_claim(x, wa, g.stream);
            if (le == hipSuccess) le = launch_contain_tally(x, wa, g.stream);
        }
    }
    hipEventRecord(g.ev1, g.stream);
    if (fast && (uint64_t)g.last_dist_fallbacks < nblocks) g.last_dist_ranges = (int)ranges;
    if (le != hipSuccess) return fail(MHX_E_HIP, "containment kernel launch failed: %s", hipGetErrorString(le));
    const hipError_t se = hipStreamSynchronize(g.stream);
    float ms = 0.f;
    hipEventElapsedTime(&ms, g.ev0, g.ev1);
    g.last_dist_ms = ms;
    if (se != hipSuccess) return fail(MHX_E_HIP, "containment kernel failed: %s", hipGetErrorString(se));
    if (c.won) {
        unsigned long long walked = 0;
        if (hipMemcpy(&walked, g.dist_ws + o_count, 8, hipMemcpyDeviceToHost) != hipSuccess) return fail(MHX_E_HIP, "D2H copy of the claim pass's counter failed");
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
    for (uint32_t i = 0; i < nq; ++i) if (q_len[i] > stride) return fail(MHX_E_ARG, "q_len[%u] exceeds stride", i);
    for (uint32_t i = 0; i < nr; ++i) if (r_len[i] > stride) return fail(MHX_E_ARG, "r_len[%u] exceeds stride", i);
    const size_t bq = up256((size_t)nq * stride * 8), bql = up256((size_t)nq * 4), br = up256((size_t)nr * stride * 8), brl = up256((size_t)nr * 4);
    const size_t cells = (size_t)nq * nr, bo = up256(cells * 4), bw = won ? bo : 0, bg = won && ref_length ? up256((size_t)nr * 8) : 0;
    uint8_t *base = nullptr;
    int rc = dist_stage(bq + bql + br + brl + 3 * bo + bw + bg, &base);
    if (rc) return rc;
    uint8_t *dq = base, *dql = dq + bq, *dr = dql + bql, *drl = dr + br, *dout = drl + brl, *dwon = dout + 3 * bo, *dlen = dwon + bw;
    hipError_t ce = hipSuccess;
    auto rows_in = [&](uint8_t *dst, const uint64_t *const *rows, const uint64_t *flat, const uint32_t *len, uint32_t n) {
        if (!rows) { ce = hipMemcpyAsync(dst, flat, (size_t)n * stride * 8, hipMemcpyHostToDevice, g.stream); return; }
        for (uint32_t i = 0; i < n && ce == hipSuccess; ++i)
            if (len[i]) ce = hipMemcpyAsync(dst + (size_t)i * stride * 8, rows[i], (size_t)len[i] * 8, hipMemcpyHostToDevice, g.stream);
    };
    rows_in(dq, q_rows, q, q_len, nq);
    if (ce == hipSuccess) rows_in(dr, r_rows, r, r_len, nr);
    if (ce == hipSuccess) ce = hipMemcpyAsync(dql, q_len, (size_t)nq * 4, hipMemcpyHostToDevice, g.stream);
    if (ce == hipSuccess) ce = hipMemcpyAsync(drl, r_len, (size_t)nr * 4, hipMemcpyHostToDevice, g.stream);
    if (ce == hipSuccess && bg) ce = hipMemcpyAsync(dlen, ref_length, (size_t)nr * 8, hipMemcpyHostToDevice, g.stream);
    if (ce != hipSuccess) return fail(MHX_E_HIP, "H2D copy failed in dist_contain: %s", hipGetErrorString(ce));
    ContainCall c{};
    c.q = (const uint64_t *)dq; c.q_len = (const uint32_t *)dql; c.r = (const uint64_t *)dr; c.r_len = (const uint32_t *)drl;
    c.nq = nq; c.nr = nr; c.stride = stride; c.s_q = s_q; c.s_r = s_r;
    for (uint32_t i = 0; i < nq; ++i) c.longest = std::max(c.longest, contain_eff_len(q_len[i], stride, s_q));
    for (uint32_t i = 0; i < nr; ++i) c.longest = std::max(c.longest, contain_eff_len(r_len[i], stride, s_r));
    c.shared = (uint32_t *)dout; c.n_qry = (uint32_t *)(dout + bo); c.n_ref = (uint32_t *)(dout + 2 * bo);
    if (won) { c.won = (uint32_t *)dwon; c.ref_length = bg ? (const uint64_t *)dlen : nullptr; }
    rc = contain_device(c);
    if (rc) return rc;
    if (won && hipMemcpy(won, c.won, cells * 4, hipMemcpyDeviceToHost) != hipSuccess) return fail(MHX_E_HIP, "D2H copy failed in dist_contain_winner");
    if (hipMemcpy(shared, c.shared, cells * 4, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(n_qry, c.n_qry, cells * 4, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(n_ref, c.n_ref, cells * 4, hipMemcpyDeviceToHost) != hipSuccess)
        return fail(MHX_E_HIP, "D2H copy failed in dist_contain");
    return MHX_OK;
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
