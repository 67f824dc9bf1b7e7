// mhx_engine_sets.h -- what the host sides of the set calls share: the rounding and the carving of a workspace or a staging
// area, the readback of a host form, the loop over groups of blocks whose flag words come back together, the block schedule
// (BlockSchedule: route, query batch, workspace, clock and the passes of a block) with what the query-by-reference calls put on
// it (SetSchedule: mhx_engine_search.cpp, mhx_engine_within.cpp, mhx_engine_contain.cpp, mhx_engine_contain_search.cpp; the
// all-pairs calls' TriSchedule is in mhx_engine_triangle.cpp) and the staging of their host forms.  Internal, host only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdlib.h>

#include <algorithm>
#include <initializer_list>
#include <vector>

#include "mhx_device.h"
#include "mhx_search.h"
#include "mhx_engine_internal.h"
#include "mhx_internal.h"

namespace mhx {

inline size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

// Regions of one allocation: take(n) declares a region of n bytes and gives its offset; `bytes` is what to allocate.
struct Carve {
    size_t bytes = 0;
    size_t take(size_t n) { const size_t o = bytes; bytes += up256(n); return o; }
};

constexpr uint32_t kBlockGroup = 4096; // blocks whose flag words come back together

// What the loop over the groups of a schedule's blocks is told: flags holds two words per block of a group (`group` blocks).
// fast: the flag words of a group are read back behind its last launch, and the flagged blocks are redone.
struct BlockGroups {
    uint64_t nblocks;
    bool fast;
    uint32_t *flags;
    uint32_t group;
    bool clear_first; // the flag words are cleared in front of the first group
    bool clear_later; // ... and in front of every later one
    bool count;       // a redone block adds to g.last_dist_fallbacks
    const char *what; // of "<what> kernel failed"
};

// Every block once, on the engine's stream: launch(b, params) queues block b, params its two words (what the range pass
// writes; params[1] is its flag); redo(b) queues a flagged block again.  One copy and one synchronisation per group.  le: the
// first launch error -- nothing is launched after it, the caller reports it.
template <class Launch, class Redo> int run_block_groups(const BlockGroups &p, hipError_t &le, Launch launch, Redo redo)
{
    std::vector<uint32_t> back;
    for (uint64_t b0 = 0; b0 < p.nblocks && le == hipSuccess; b0 += kBlockGroup) {
        const uint64_t b1 = std::min<uint64_t>(p.nblocks, b0 + kBlockGroup);
        if (b0 != 0 ? p.clear_later : p.clear_first) le = hipMemsetAsync(p.flags, 0, (size_t)2 * p.group * 4, g.stream);
        for (uint64_t b = b0; b < b1 && le == hipSuccess; ++b) le = launch(b, p.flags + 2 * (b - b0));
        if (!p.fast || le != hipSuccess) continue;
        back.resize((size_t)(b1 - b0) * 2);
        if (hipMemcpyAsync(back.data(), p.flags, back.size() * 4, hipMemcpyDeviceToHost, g.stream) != hipSuccess ||
            hipStreamSynchronize(g.stream) != hipSuccess)
            return fail(MHX_E_HIP, "%s kernel failed", p.what);
        for (uint64_t b = b0; b < b1 && le == hipSuccess; ++b)
            if (back[2 * (b - b0) + 1]) { // a value range overflowed the LDS table or the byte counters
                le = redo(b);
                if (p.count) ++g.last_dist_fallbacks;
            }
    }
    return MHX_OK;
}

// A short list of device arrays to the host, one after the other with hipMemcpy (each waits for the device); an entry that is
// not wanted is left out.  name: the call's, for the message ("dist_mst").
struct Readback {
    void *to;
    const void *from;
    size_t bytes;
    bool wanted = true;
};
inline int read_back(const char *name, std::initializer_list<Readback> list)
{
    for (const Readback &r : list)
        if (r.wanted && hipMemcpy(r.to, r.from, r.bytes, hipMemcpyDeviceToHost) != hipSuccess) return fail(MHX_E_HIP, "D2H copy failed in %s", name);
    return MHX_OK;
}

// What a set call is scheduled by, from its inputs alone.
struct SetGeometry {
    uint32_t ranges;        // value ranges per block (0: none, the pair kernel takes the call)
    uint64_t weight;        // of a pair in the test for the range route
    const char *qbatch_env; // the variable that lowers the query batch
    uint32_t most_queries;  // the most queries a block covers
    const char *what;       // the call in the messages: "<what> kernel failed"
};

// The schedule of (query batch, slice of 32 references) blocks over the engine's stream, what the query-by-reference calls
// (SetSchedule below) and the all-pairs calls (TriSchedule, mhx_engine_triangle.cpp) share: the choice of the route and of the
// query batch, the common workspace, the clock, and the passes of a block -- the range pass, the call's finish pass and the
// call's take-out pass; a flagged block is redone by the call's pair kernel and taken out then.
// A call goes: construct (geometry, from the inputs alone), extra() for room of its own, place(), begin(), its own setup,
// offsets(), its blocks once or several times, its own last launches, end(), its own readback in wait().
struct BlockSchedule {
    uint32_t ranges, qbatch, group = 0, lead = 0;
    const char *what;
    bool fast;
    // workspace in g.dist_ws: [offsets of the queries][offsets of the references][byte counters][window totals][words: shift, 0,
    // the schedule's own up to `lead`, then two per block of a group][what the call asked for through extra()]
    Carve ws;
    size_t o_offq = 0, o_offr = 0, o_cpart = 0, o_wtot = 0, o_words = 0;
    uint32_t *offq = nullptr, *offr = nullptr, *words = nullptr, *flags = nullptr;
    DistWork w{};
    uint64_t counted = 0;       // the blocks of the runs whose fallbacks are counted
    hipError_t le = hipSuccess; // the first launch error: nothing is launched after it, end() reports it

    BlockSchedule(uint64_t pairs, const SetGeometry &geo) : ranges(geo.ranges), what(geo.what)
    {
        fast = (pairs >= 64 || (pairs >= 8 && pairs * geo.weight >= 400000)) && ranges != 0 && getenv("MHX_DIST_GENERIC") == nullptr;
        qbatch = tri_max_queries(fast ? ranges : kTriMinRanges);
        if (const char *e = getenv(geo.qbatch_env)) { const long v = atol(e); if (v > 0 && (uint64_t)v < qbatch) qbatch = (uint32_t)v; }
        qbatch = std::min(qbatch, geo.most_queries);
    }
    uint64_t per() const { return (uint64_t)ranges + 1; } // offsets per list
    // the common workspace: offsets tables of n_q and of n_r lists (0: no such table), at most `blocks` blocks in a run, `lead_`
    // words in front of the flag words
    void carve(uint64_t n_q, uint64_t n_r, uint64_t blocks, uint32_t lead_)
    {
        group = (uint32_t)std::min<uint64_t>(blocks, kBlockGroup);
        lead = lead_;
        o_offq = ws.take(fast ? (size_t)n_q * per() * 4 : 0);
        o_offr = ws.take(fast ? (size_t)n_r * per() * 4 : 0);
        o_cpart = ws.take(fast ? (size_t)qbatch * ranges * kTriSlice : 0);
        o_wtot = ws.take(fast && ranges > (uint32_t)kDistRanges ? (size_t)qbatch * (ranges / kDistWindowRanges) * kTriSlice * 4 : 0);
        o_words = ws.take((size_t)(lead + 2 * group) * 4);
    }
    // room of the call's own behind the common part (before place()): where it lies, for at()
    size_t extra(size_t n) { return ws.take(n); }
    uint8_t *at(size_t o) const { return g.dist_ws + o; }
    int place(const char *room) // room: "the search workspace"
    {
        if (g.dist_ws.grow(ws.bytes, g.stream) != hipSuccess) return fail(MHX_E_HIP, "hipMalloc failed for %s (%zu bytes)", room, ws.bytes);
        offq = (uint32_t *)at(o_offq); offr = (uint32_t *)at(o_offr);
        words = (uint32_t *)at(o_words); flags = words + lead;
        w.cpart = at(o_cpart);
        w.wtot = (uint32_t *)at(o_wtot);
        w.ranges = ranges;
        return MHX_OK;
    }
    // the clock starts, the words are zero, nothing has fallen back yet
    void begin()
    {
        hipEventRecord(g.ev0, g.stream);
        le = hipMemsetAsync(words, 0, (size_t)(lead + 2 * group) * 4, g.stream);
        g.last_dist_fallbacks = fast ? 0 : -1;
        g.last_dist_ranges = 0;
    }
    // what the one split of the lists into value ranges works on: words[0] the shift of the call, words[1] stays 0
    DistWork offsets_work(uint32_t *offs_q, uint32_t *offs_r) const
    {
        DistWork wa = w;
        wa.offs_q = offs_q; wa.offs_r = offs_r; wa.params = words;
        return wa;
    }
    // n blocks once; clear_first, clear_later, count: see BlockGroups.  where(b, x) makes x the lists of block b and points
    // w.offs_q / w.offs_r at the offsets of its first query and first reference.  The passes of block b, each returning its
    // launch's hipError_t: pairs(b, x) the pair kernel, finish(b, x, w) the finish pass behind the range pass, take(b, flag,
    // generic) the take-out pass, which does nothing where *flag is set; generic: behind the pair kernel, whose blocks have
    // words + 1, which stays 0, for a flag.
    template <class Where, class Pairs, class Finish, class Take>
    int run_blocks(uint64_t n, bool clear_first, bool clear_later, bool count, Where where, Pairs pairs, Finish finish, Take take)
    {
        if (count) counted += n;
        auto generic = [&](uint64_t b) {
            DistArgs x;
            where(b, x);
            hipError_t e = pairs(b, x);
            if (e == hipSuccess) e = take(b, words + 1, true);
            return e;
        };
        return run_block_groups(
            BlockGroups{n, fast, flags, group, clear_first, clear_later, count, what}, le,
            [&](uint64_t b, uint32_t *params) {
                if (!fast) return generic(b);
                DistArgs x;
                where(b, x);
                w.params = params;
                hipError_t e = launch_dist_range_pass(x, w, g.stream);
                if (e == hipSuccess) e = finish(b, x, w);
                if (e == hipSuccess) e = take(b, params + 1, false);
                return e;
            },
            generic);
    }
    // the clock stops behind the call's last launch; a launch that failed anywhere is reported here
    int end()
    {
        hipEventRecord(g.ev1, g.stream);
        if (fast && (uint64_t)g.last_dist_fallbacks < counted) g.last_dist_ranges = (int)ranges;
        if (le != hipSuccess) return fail(MHX_E_HIP, "%s kernel launch failed: %s", what, hipGetErrorString(le));
        return MHX_OK;
    }
    // waits for the call, its readback (se: how queueing it went) included, and notes the time
    int wait(hipError_t se = hipSuccess)
    {
        if (se == hipSuccess) se = hipStreamSynchronize(g.stream);
        float ms = 0.f;
        hipEventElapsedTime(&ms, g.ev0, g.ev1);
        g.last_dist_ms = ms;
        if (se != hipSuccess) return fail(MHX_E_HIP, "%s kernel failed: %s", what, hipGetErrorString(se));
        return MHX_OK;
    }
};

// The schedule of a query-by-reference call.  Both sets are split into value ranges ONCE, with one shift (offsets()); run()
// goes once or once per range of queries.
struct SetSchedule : BlockSchedule {
    uint32_t nr, stride;
    bool clear_first = false, clear_later = true; // see BlockGroups
    DistArgs lists{};                             // both sets as offsets() saw them; a block's lists are cut from here

    SetSchedule(uint32_t nq, uint32_t nr_, uint32_t stride_, const SetGeometry &geo) : BlockSchedule((uint64_t)nq * nr_, geo), nr(nr_), stride(stride_)
    {
        carve(nq, nr, search_blocks(geo.most_queries, nr, qbatch), 2);
    }
    // both sets as the passes of mhx_dist.hip see them, and their one split
    void offsets(const DistArgs &both)
    {
        lists = both;
        if (fast && le == hipSuccess) le = launch_dist_offsets_both(lists, offsets_work(offq, offr), g.stream);
    }
    // The blocks of queries [q_first, q_first + q_count), whose block coordinates count from q_first.  The call's passes as
    // BlockSchedule::run_blocks has them, with the block itself for its index: pairs(blk, x), finish(blk, x, w), take(blk, flag).
    template <class Pairs, class Finish, class Take> int run(uint32_t q_first, uint32_t q_count, Pairs pairs, Finish finish, Take take)
    {
        auto block = [&](uint64_t b) { return search_block(q_count, nr, qbatch, b); };
        return run_blocks(
            search_blocks(q_count, nr, qbatch), clear_first, clear_later, true,
            [&](uint64_t b, DistArgs &x) {
                const SearchBlock blk = block(b);
                x = lists;
                x.q = lists.q + (uint64_t)(q_first + blk.q0) * stride; x.q_len = lists.q_len + q_first + blk.q0; x.nq = blk.nq;
                x.r = lists.r + (uint64_t)blk.r0 * stride; x.r_len = lists.r_len + blk.r0; x.nr = blk.nr;
                w.offs_q = offq + (uint64_t)(q_first + blk.q0) * per();
                w.offs_r = offr + (uint64_t)blk.r0 * per();
            },
            [&](uint64_t b, const DistArgs &x) { return pairs(block(b), x); },
            [&](uint64_t b, const DistArgs &x, DistWork &wk) { return finish(block(b), x, wk); },
            [&](uint64_t b, uint32_t *flag, bool) { return take(block(b), flag); });
    }
};

// The staging of a host form in g.dist_in: both sets at `stride`, and `room` bytes behind them for the caller's outputs.
// A set comes as a matrix [n][stride] (flat, copied as one block), as row pointers (rows: len[i] entries from each), or, the
// references only, resident on the device already (refs).  name: the call's, for the messages ("dist_search").
struct HostSet {
    const uint64_t *flat;
    const uint64_t *const *rows;
    const uint32_t *len;
    uint32_t n;
};
struct StagedSets {
    const uint64_t *q, *r;
    const uint32_t *q_len, *r_len;
    uint8_t *room;
};
inline int stage_sets(const char *name, const HostSet &Q, const HostSet &R, const SearchRefs *refs, uint32_t stride, size_t room, StagedSets &out)
{
    for (uint32_t i = 0; i < Q.n; ++i) if (Q.len[i] > stride) return fail(MHX_E_ARG, "q_len[%u] exceeds stride", i);
    if (!refs) for (uint32_t i = 0; i < R.n; ++i) if (R.len[i] > stride) return fail(MHX_E_ARG, "r_len[%u] exceeds stride", i);
    Carve in;
    const size_t o_q = in.take((size_t)Q.n * stride * 8), o_ql = in.take((size_t)Q.n * 4);
    const size_t o_r = in.take(refs ? 0 : (size_t)R.n * stride * 8), o_rl = in.take(refs ? 0 : (size_t)R.n * 4);
    const size_t o_room = in.take(room);
    uint8_t *base = nullptr;
    const int rc = dist_stage(in.bytes, &base);
    if (rc) return rc;
    hipError_t ce = hipSuccess;
    auto set_in = [&](const HostSet &S, size_t o_rows, size_t o_len) {
        if (S.rows) { // every row from its own place
            for (uint32_t i = 0; i < S.n && ce == hipSuccess; ++i)
                if (S.len[i]) ce = hipMemcpyAsync(base + o_rows + (size_t)i * stride * 8, S.rows[i], (size_t)S.len[i] * 8, hipMemcpyHostToDevice, g.stream);
        } else if (ce == hipSuccess)
            ce = hipMemcpyAsync(base + o_rows, S.flat, (size_t)S.n * stride * 8, hipMemcpyHostToDevice, g.stream);
        if (ce == hipSuccess) ce = hipMemcpyAsync(base + o_len, S.len, (size_t)S.n * 4, hipMemcpyHostToDevice, g.stream);
    };
    set_in(Q, o_q, o_ql);
    if (!refs) set_in(R, o_r, o_rl);
    if (ce != hipSuccess) return fail(MHX_E_HIP, "H2D copy failed in %s: %s", name, hipGetErrorString(ce));
    out.q = (const uint64_t *)(base + o_q); out.q_len = (const uint32_t *)(base + o_ql);
    out.r = refs ? refs->rows : (const uint64_t *)(base + o_r); out.r_len = refs ? refs->len : (const uint32_t *)(base + o_rl);
    out.room = base + o_room;
    return MHX_OK;
}

} // namespace mhx
