// tests/emul/line_rel_items_emul.cpp -- CPU run of the line-relative items of sketch_tile_kernel (test tool): the item writer
// (phase_line_rel_items) next to the map path on the same staged tile, and the whole path -- writer, item reader
// (process_line_rel_item, line_rel_source), the hot body on the trips that begin among the full
// items and the TAIL body on the trips that begin among the tails, 64 entries to a trip as a wave takes them -- next to the
// aligned items (phase_line_items + process_group), with T admitting every hash.  The very functions of
// auriclass_amd/csrc/mhx_tile.h the HIP kernel runs, in the order it separates them with __syncthreads().
// Not part of the product; built by tests/test_line_rel_items.py with g++.
#include <cstdint>
#include <cstring>
#include <vector>
#include "../../auriclass_amd/csrc/mhx_tile.h"

using namespace mhx;

enum : int {
    kOutTiles = 0,       // tiles run
    kOutRel = 1,         // tiles that take the line-relative items
    kOutTooLong = 2,     // tiles that try the line path and fall back to the maps (a line above the bound)
    kOutWindowDiff = 3,  // tiles whose items' windows are not the map path's valid starts, each once
    kOutKmerDiff = 4,    // tiles whose k-mer counts differ
    kOutOrderDiff = 5,   // tiles with a tail in front of a full item, a full item without its flag, a tail that is not
                         //   (1 << (kmers & 7)) - 1 at a + 8 (kmers >> 3), or a listed tail of no window
    kOutBoundsDiff = 6,  // tiles with an entry whose 4 ND source bytes are not all staged
    kOutFull = 7,        // full items
    kOutTails = 8,       // tail items
    kOutAligned = 9,     // items of the aligned list on the same tiles
    kOutMoreItems = 10,  // tiles with more entries than the aligned list has
    kOutHotTrips = 11,   // trips of 64 entries run on the hot body (hashes call)
    kOutTailTrips = 12,  // ... on the TAIL body
    kOutChosen = 13,     // tiles of kOutRel on which the kernel's choice (line_rel_choose) takes the new items
    kOutOffsetDiff = 14, // tiles on which the packed prefix does not give a lane its offset in the aligned list
    kOutCount = 15
};
enum : uint8_t { kFormMaps = 0, kFormRel = 1, kFormTooLong = 2 };

static TileSmem sm;
static ThreadState st[kBlock];

struct VecInserter {
    std::vector<uint64_t> *out;
    void operator()(uint64_t h) { out->push_back(h); }
};
// the queue forms' candidate: finished at once from its byte position, as finish_candidate does behind the loop
template <int K> struct AtOnce {
    const TileSmem &sm; uint64_t T; VecInserter &ins; bool aligned;
    void operator()(uint32_t at, int window) const { process_deferred<K>(sm, aligned ? (at << 3) | (uint32_t)window : at + (uint32_t)window, T, ins); }
};

static uint32_t parse_head(const uint8_t *base, uint64_t tile_off, uint64_t begin, uint64_t end, bool interior, uint32_t (&excl)[kBlock])
{
    for (int t = 0; t < kBlock; ++t) phase_stage(sm, t, base, tile_off, end);
    for (int t = 0; t < kBlock; ++t) phase_classify(sm, t, st[t], tile_off, begin, end, interior);
    uint32_t tile_total = 0;
    for (int t = 0; t < kBlock; ++t) { excl[t] = tile_total; tile_total += st[t].nlcount; }
    return tile_total;
}

// the map path's list and masks of the tile staged in sm; returns the k-mers
template <int K> static uint32_t by_maps(bool fast_parse, uint32_t line_base, const uint32_t (&excl)[kBlock], uint32_t tile_total, uint32_t check_limit,
                                         uint64_t tile_off, uint64_t end, uint32_t &nitems)
{
    bool bad = false;
    if (fast_parse) {
        for (int t = 0; t < kBlock; ++t) phase_events(sm, t, st[t], excl[t]);
        for (int t = 0; t < kBlock; ++t) phase_good_events(sm, t, st[t], line_base, excl[t], tile_total, check_limit, bad, tile_off, end, (uint32_t)K);
    } else {
        for (int t = 0; t < kBlock; ++t) phase_good<true>(sm, t, st[t], line_base, excl[t], tile_total, check_limit, bad, tile_off, end, (uint32_t)K);
    }
    uint32_t items[kBlock], kmers = 0;
    nitems = 0;
    for (int t = 0; t < kBlock; ++t) kmers += phase_runs<K>(sm, t, items[t]);
    for (int t = 0; t < kBlock; ++t) { phase_compact(sm, t, nitems); nitems += items[t]; }
    return kmers;
}

// the line path up to its barrier: the spans, the aligned offsets and the packed ones; false: a line above the bound
template <int K> static bool line_spans(uint32_t line_base, uint32_t tile_total, LineSpan (&span)[kLineItemLines], uint32_t (&at)[kLineItemLines],
                                        uint32_t (&at_rel)[kLineItemLines], uint32_t &naligned, uint32_t &packed, bool &offset_diff)
{
    bool too_long = false;
    naligned = packed = 0;
    offset_diff = false;
    for (uint32_t t = 0; t < kLineItemLines; ++t) {
        span[t] = phase_line_span<K>(sm, t, line_base, tile_total);
        if (line_span_too_long(span[t])) too_long = true;
        at[t] = naligned;               // the kernel's atomicAdd on sm.misc[1], either form
        naligned += span[t].ngroups;
        at_rel[t] = packed;
        packed += line_rel_counts(span[t]);
        if (line_rel_aligned(at_rel[t]) != at[t]) offset_diff = true; // the lane's offset in the aligned list, from the packed prefix
    }
    return !too_long;
}

template <int K, bool QUEUE>
static int run(const uint8_t *base, uint64_t begin, uint64_t end, uint32_t first_line, uint64_t *out, uint8_t *form,
               std::vector<uint64_t> *h_new, std::vector<uint64_t> *h_ref)
{
    constexpr int ND = GroupGeom<K>::ND;
    constexpr bool kPairs = pair_words_form<K>(2, QUEUE);
    memset(out, 0, kOutCount * sizeof(uint64_t));
    const uint32_t first_tile = (uint32_t)(begin / kTileBytes);
    const uint32_t ntiles = (uint32_t)((end + kTileBytes - 1) / kTileBytes);
    const uint64_t T = ~0ull;
    const uint32_t limit = admission_limit(T);
    uint32_t line_prefix = first_line;
    static uint8_t ref_valid[kTileBytes], seen[kTileBytes];
    for (uint32_t tile = first_tile; tile < ntiles; ++tile) {
        const uint64_t tile_off = (uint64_t)tile * kTileBytes;
        const bool interior = tile_off >= begin && tile_off + kTileBytes + kHaloBytes <= end;
        const uint64_t span_left = end > tile_off ? end - tile_off : 0;
        const uint32_t check_limit = span_left < (uint64_t)(kTileBytes + kHaloBytes) ? (uint32_t)span_left : (uint32_t)(kTileBytes + kHaloBytes);
        uint32_t excl[kBlock];
        uint32_t tile_total = parse_head(base, tile_off, begin, end, interior, excl);
        const uint32_t line_base = line_prefix & 3u;
        line_prefix += tile_total;
        const bool fast_parse = parse_events_fit(tile_total);
        ++out[kOutTiles];

        // ---- the map path: the reference of the windows, and the list both hash runs take on a tile that keeps the maps
        uint32_t nitems_ref = 0;
        const uint32_t kmers_ref = by_maps<K>(fast_parse, line_base, excl, tile_total, check_limit, tile_off, end, nitems_ref);
        memset(ref_valid, 0, sizeof(ref_valid));
        for (uint32_t i = 0; i < nitems_ref; ++i) {
            const uint32_t g = sm.list[i], m = reinterpret_cast<const uint8_t *>(sm.valid)[g];
            for (uint32_t j = 0; j < 8; ++j) if ((m >> j) & 1u) ref_valid[8 * g + j] = 1;
        }
        uint8_t &f = form[tile - first_tile];
        f = kFormMaps;
        bool rel = line_items_apply<K>() && line_items_try(fast_parse, interior, line_base, tile_total); // (every K of the line path: which kernel forms take the items is line_rel_form's)
        LineSpan span[kLineItemLines];
        uint32_t at[kLineItemLines], at_rel[kLineItemLines], naligned = 0, packed = 0;
        bool offset_diff = false;
        if (rel) {
            tile_total = parse_head(base, tile_off, begin, end, interior, excl);
            for (int t = 0; t < kBlock; ++t) phase_events(sm, t, st[t], excl[t]);
            if (!line_spans<K>(line_base, tile_total, span, at, at_rel, naligned, packed, offset_diff)) {
                rel = false;
                f = kFormTooLong;
                ++out[kOutTooLong];
                if (h_new) by_maps<K>(fast_parse, line_base, excl, tile_total, check_limit, tile_off, end, nitems_ref); // (the events are listed: the maps again)
            }
        }
        if (!rel) { // the aligned format, on both sides
            if (h_new) {
                VecInserter in_new{h_new}, in_ref{h_ref};
                AtOnce<K> q_new{sm, T, in_new, true}, q_ref{sm, T, in_ref, true};
                for (uint32_t it = 0; it < nitems_ref; ++it) {
                    process_group<K, QUEUE, kPairs>(sm, sm.list[it], T, limit, in_new, q_new, hot_tail_table<K>());
                    process_group<K, QUEUE, kPairs>(sm, sm.list[it], T, limit, in_ref, q_ref, hot_tail_table<K>());
                }
            }
            continue;
        }
        f = kFormRel;
        ++out[kOutRel];
        // ---- behind the barrier: nothing of the events, the newline map or the other path's result may stand in
        memset(sm.valid, 0xA5, sizeof(sm.valid));
        memset(sm.maps, 0xA5, sizeof(sm.maps));
        uint32_t kmers_new = 0;
        for (uint32_t t = 0; t < kLineItemLines; ++t) {
            kmers_new += span[t].kmers;
            phase_line_rel_items(sm, span[t], at_rel[t], packed);
        }
        if (offset_diff || line_rel_aligned(packed) != naligned) ++out[kOutOffsetDiff];
        if (line_rel_choose(packed)) ++out[kOutChosen];
        const uint32_t nfull = line_rel_full(packed), nitems = line_rel_items(packed);
        out[kOutFull] += nfull;
        out[kOutTails] += nitems - nfull;
        out[kOutAligned] += naligned;
        if (nitems > naligned || nitems > (uint32_t)kGroupsPerTile) ++out[kOutMoreItems];
        bool window_diff = false, order_diff = false, bounds_diff = false;
        memset(seen, 0, sizeof(seen));
        for (uint32_t i = 0; i < nitems && i < (uint32_t)kGroupsPerTile; ++i) {
            const uint32_t e = sm.list[i], vm = line_rel_vm(sm, e), pos = vm >> 8, mask = vm & 0xFFu;
            if (((e & kLineRelFull) != 0u) != (i < nfull) || (e & ~(kLineRelFull | kLineRelPos))) order_diff = true;
            if (i < nfull ? mask != 0xFFu : (mask == 0u || mask == 0xFFu || (mask & (mask + 1u)))) order_diff = true;
            if (pos + 4u * ND > (uint32_t)(kTileBytes + kHaloBytes)) bounds_diff = true;
            for (uint32_t j = 0; j < 8; ++j) {
                if (!((mask >> j) & 1u)) continue;
                if (pos + j >= (uint32_t)kTileBytes || seen[pos + j] || !ref_valid[pos + j]) { window_diff = true; continue; }
                seen[pos + j] = 1;
            }
        }
        if (memcmp(seen, ref_valid, sizeof(seen))) window_diff = true;
        for (uint32_t t = 0; t < kLineItemLines; ++t) { // every line's tail where the writer's rule puts it
            const uint32_t c = span[t].kmers & 7u;
            if (!c) continue;
            const uint32_t e = sm.list[nfull + line_rel_tails(at_rel[t])], want = span[t].a + 8u * (span[t].kmers >> 3);
            if (e != want || reinterpret_cast<const uint8_t *>(sm.valid)[want >> 3] != (1u << c) - 1u) order_diff = true;
        }
        if (window_diff) ++out[kOutWindowDiff];
        if (order_diff) ++out[kOutOrderDiff];
        if (bounds_diff) ++out[kOutBoundsDiff];
        if (kmers_new != kmers_ref) ++out[kOutKmerDiff];
        if (!h_new) continue;

        // ---- the hash loop over the new list, trip by trip
        {
            VecInserter in_new{h_new};
            AtOnce<K> q_new{sm, T, in_new, false};
            for (uint32_t t0 = 0; t0 < nitems; t0 += 64u) {
                const bool tail_trip = t0 >= nfull; // the kernel's scalar test on the trip's first entry
                ++out[tail_trip ? kOutTailTrips : kOutHotTrips];
                for (uint32_t it = t0; it < nitems && it < t0 + 64u; ++it) {
                    if (tail_trip) process_line_rel_item<K, QUEUE, kPairs, true>(sm, sm.list[it], T, limit, in_new, q_new, hot_tail_table<K>());
                    else process_line_rel_item<K, QUEUE, kPairs, false>(sm, sm.list[it], T, limit, in_new, q_new, hot_tail_table<K>());
                }
            }
        }
        // ---- ... and over the aligned list of the same lines (sm.bytes stands; list and masks are written anew)
        {
            for (uint32_t t = 0; t < kLineItemLines; ++t) phase_line_items(sm, span[t], at[t]);
            VecInserter in_ref{h_ref};
            AtOnce<K> q_ref{sm, T, in_ref, true};
            for (uint32_t it = 0; it < naligned; ++it) process_group<K, QUEUE, kPairs>(sm, sm.list[it], T, limit, in_ref, q_ref, hot_tail_table<K>());
        }
    }
    return 0;
}

#define K_LIST(X) X(8) X(16) X(21) X(27) X(32)

// the span [begin, end) of base, which begins in line number first_line (mod 4) of its file; form: one byte per tile.
// With hash buffers (cap entries each): the hashes either list inserts, in the order found; queue: the queue forms' loop.
extern "C" int emul_line_rel_run(const uint8_t *base, uint64_t begin, uint64_t end, uint32_t first_line, int k, int queue, uint64_t *out15,
                                 uint8_t *form, uint64_t *hashes_new, uint64_t *hashes_ref, uint64_t cap, uint64_t *n2)
{
    std::vector<uint64_t> h_new, h_ref;
    const bool hash = hashes_new != nullptr;
    int rc = -1;
    switch (k) {
#define X(KK) case KK: rc = queue ? run<KK, true>(base, begin, end, first_line, out15, form, hash ? &h_new : nullptr, hash ? &h_ref : nullptr) \
                                  : run<KK, false>(base, begin, end, first_line, out15, form, hash ? &h_new : nullptr, hash ? &h_ref : nullptr); break;
        K_LIST(X)
#undef X
    default: return -1;
    }
    if (hash) {
        n2[0] = h_new.size();
        n2[1] = h_ref.size();
        if (h_new.size() > cap || h_ref.size() > cap) return -2;
        if (!h_new.empty()) memcpy(hashes_new, h_new.data(), h_new.size() * 8);
        if (!h_ref.empty()) memcpy(hashes_ref, h_ref.data(), h_ref.size() * 8);
    }
    return rc;
}

// line_rel_form<K>(fmt, queue): does that kernel form take the line-relative items? (-1: no such K)
extern "C" int emul_line_rel_form(int k, int fmt, int queue)
{
    switch (k) {
#define X(KK) case KK: return line_rel_form<KK>(fmt, queue != 0) ? 1 : 0;
        X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10) X(11) X(12) X(13) X(14) X(15) X(16)
        X(17) X(18) X(19) X(20) X(21) X(22) X(23) X(24) X(25) X(26) X(27) X(28) X(29) X(30) X(31) X(32)
#undef X
    default: return -1;
    }
}

// line_rel_choose on the packed totals of a tile with these counts (extra: aligned groups beyond the new entries)
extern "C" int emul_line_rel_choose(uint32_t full, uint32_t tails, uint32_t extra)
{
    const uint32_t packed = full | (tails << 13) | (extra << 20);
    if (line_rel_full(packed) != full || line_rel_tails(packed) != tails || line_rel_aligned(packed) != full + tails + extra) return -1;
    return line_rel_choose(packed) ? 1 : 0;
}
