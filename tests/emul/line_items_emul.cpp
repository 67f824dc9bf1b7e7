// tests/emul/line_items_emul.cpp -- CPU comparison of the two ways sketch_tile_kernel makes a FASTQ tile's work list (test
// tool).  Runs, tile by tile and thread by thread, the map path (phase_events + phase_good_events or phase_good, phase_runs,
// the scan, phase_compact) and the line-item form (phase_events, phase_event_checks, phase_line_span, phase_line_items) of
// auriclass_amd/csrc/mhx_tile.h -- the very functions the HIP kernel runs, in the order it separates them with
// __syncthreads() -- on the same staged tile, and compares what they leave behind: the set of listed groups, the start mask
// of every listed group, the k-mer count, the long-record count and the bad-format flag.  It also reports which form the
// kernel's conditions choose for each tile.
// Not part of the product; built by tests/test_line_items.py with g++.
#include <cstdint>
#include <cstring>
#include "../../auriclass_amd/csrc/mhx_tile.h"

using namespace mhx;

enum : int {
    kOutTiles = 0,      // tiles run
    kOutByLines = 1,    // tiles that take the line-item form
    kOutTooLong = 2,    // tiles that try it and find a sequence line above the bound: the maps after all
    kOutListDiff = 3,   // tiles whose sets of listed groups differ (or whose list names a group twice)
    kOutMaskDiff = 4,   // tiles in which a listed group's start mask differs
    kOutKmerDiff = 5,   // tiles whose k-mer counts differ
    kOutCheckDiff = 6,  // tiles whose long-record counts or bad-format flags differ
    kOutKmers = 7,      // k-mers, map path
    kOutItems = 8,      // listed groups, map path
    kOutRecords = 9,    // long records, map path
    kOutCount = 10
};
enum : uint8_t { kFormMaps = 0, kFormLines = 1, kFormTooLong = 2 };

static TileSmem sm;
static ThreadState st[kBlock];

// stage, classify, scan: the kernel up to the barrier behind which the line phase is known
static uint32_t parse_head(const uint8_t *base, uint64_t tile_off, uint64_t begin, uint64_t end, bool interior, uint32_t (&excl)[kBlock])
{
    for (int t = 0; t < kBlock; ++t) phase_stage(sm, t, base, tile_off, end);
    for (int t = 0; t < kBlock; ++t) phase_classify(sm, t, st[t], tile_off, begin, end, interior);
    uint32_t tile_total = 0;
    for (int t = 0; t < kBlock; ++t) { excl[t] = tile_total; tile_total += st[t].nlcount; }
    return tile_total;
}

template <int K>
static int compare(const uint8_t *base, uint64_t begin, uint64_t end, uint32_t first_line, uint64_t *out, uint8_t *form)
{
    memset(out, 0, kOutCount * sizeof(uint64_t));
    const uint32_t first_tile = (uint32_t)(begin / kTileBytes);
    const uint32_t ntiles = (uint32_t)((end + kTileBytes - 1) / kTileBytes);
    uint32_t line_prefix = first_line; // index of the line the span begins in
    static uint8_t mask_ref[kGroupsPerTile];
    static bool listed_ref[kGroupsPerTile], listed_new[kGroupsPerTile];
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

        // ---- the map path
        bool bad_ref = false;
        uint32_t long_ref = 0, kmers_ref = 0, nitems_ref = 0;
        if (fast_parse) {
            for (int t = 0; t < kBlock; ++t) phase_events(sm, t, st[t], excl[t]);
            for (int t = 0; t < kBlock; ++t) long_ref += phase_good_events(sm, t, st[t], line_base, excl[t], tile_total, check_limit, bad_ref, tile_off, end, (uint32_t)K);
        } else {
            for (int t = 0; t < kBlock; ++t) long_ref += phase_good<true>(sm, t, st[t], line_base, excl[t], tile_total, check_limit, bad_ref, tile_off, end, (uint32_t)K);
        }
        uint32_t items[kBlock];
        for (int t = 0; t < kBlock; ++t) kmers_ref += phase_runs<K>(sm, t, items[t]);
        for (int t = 0; t < kBlock; ++t) { phase_compact(sm, t, nitems_ref); nitems_ref += items[t]; }
        memset(listed_ref, 0, sizeof(listed_ref));
        for (uint32_t i = 0; i < nitems_ref; ++i) {
            const uint32_t g = sm.list[i];
            listed_ref[g] = true;
            mask_ref[g] = reinterpret_cast<const uint8_t *>(sm.valid)[g];
        }
        out[kOutKmers] += kmers_ref;
        out[kOutItems] += nitems_ref;
        out[kOutRecords] += long_ref;

        // ---- the kernel's choice
        uint8_t &f = form[tile - first_tile];
        f = kFormMaps;
        if (!(line_items_apply<K>() && line_items_try(fast_parse, interior, line_base, tile_total))) continue;

        // ---- the line-item form, on the tile staged anew (the map path has written over the newline map and the events)
        tile_total = parse_head(base, tile_off, begin, end, interior, excl);
        for (int t = 0; t < kBlock; ++t) phase_events(sm, t, st[t], excl[t]);
        bool bad_new = false;
        uint32_t long_new = 0, kmers_new = 0, nitems_new = 0;
        LineSpan span[kLineItemLines];
        uint32_t at[kLineItemLines];
        bool too_long = false;
        for (int t = 0; t < kBlock; ++t) {
            long_new += phase_event_checks(sm, t, line_base, tile_total, check_limit, bad_new, tile_off, end, (uint32_t)K);
            if (t < (int)kLineItemLines) {
                span[t] = phase_line_span<K>(sm, (uint32_t)t, line_base, tile_total);
                if (line_span_too_long(span[t])) too_long = true;
                at[t] = nitems_new;            // the kernel's atomicAdd on sm.misc[1]
                nitems_new += span[t].ngroups;
            }
        }
        if (bad_ref != bad_new || long_ref != long_new) ++out[kOutCheckDiff];
        if (too_long) { f = kFormTooLong; ++out[kOutTooLong]; continue; }
        f = kFormLines;
        ++out[kOutByLines];
        // behind the barrier: nothing of the events, the newline map or the other path's result may stand in
        memset(sm.valid, 0xA5, sizeof(sm.valid));
        memset(sm.maps, 0xA5, sizeof(sm.maps));
        for (int t = 0; t < (int)kLineItemLines; ++t) {
            kmers_new += span[t].kmers;
            phase_line_items(sm, span[t], at[t]);
        }
        memset(listed_new, 0, sizeof(listed_new));
        bool list_diff = nitems_new != nitems_ref || nitems_new > (uint32_t)kGroupsPerTile, mask_diff = false;
        for (uint32_t i = 0; i < nitems_new && i < (uint32_t)kGroupsPerTile; ++i) {
            const uint32_t g = sm.list[i];
            if (g >= (uint32_t)kGroupsPerTile || listed_new[g] || !listed_ref[g]) { list_diff = true; continue; }
            listed_new[g] = true;
            if (reinterpret_cast<const uint8_t *>(sm.valid)[g] != mask_ref[g]) mask_diff = true;
        }
        if (list_diff) ++out[kOutListDiff];
        if (mask_diff) ++out[kOutMaskDiff];
        if (kmers_new != kmers_ref) ++out[kOutKmerDiff];
    }
    return 0;
}

// the span [begin, end) of base, which begins in line number first_line (mod 4) of its file; form: one byte per tile
extern "C" int emul_line_items_compare(const uint8_t *base, uint64_t begin, uint64_t end, uint32_t first_line, int k, uint64_t *out10, uint8_t *form)
{
    switch (k) {
#define X(KK) case KK: return compare<KK>(base, begin, end, first_line, out10, form);
        X(8) X(16) X(21) X(27) X(32)
        X(7) // below the form's smallest K: every tile keeps the maps
#undef X
    default: return -1;
    }
}

// line_items_form<K>(fmt, queue): does that kernel form have the path? (-1: no such K)
extern "C" int emul_line_items_form(int k, int fmt, int queue)
{
    switch (k) {
#define X(KK) case KK: return line_items_form<KK>(fmt, queue != 0) ? 1 : 0;
        X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10) X(11) X(12) X(13) X(14) X(15) X(16)
        X(17) X(18) X(19) X(20) X(21) X(22) X(23) X(24) X(25) X(26) X(27) X(28) X(29) X(30) X(31) X(32)
#undef X
    default: return -1;
    }
}

extern "C" void emul_line_items_bounds(uint32_t *out3)
{
    out3[0] = kLineItemLines;
    out3[1] = kLineItemGroups;
    out3[2] = kLineItemMinNewlines;
}
