// tests/emul/parse_front_emul.cpp -- CPU check of the long-record count of the line path of sketch_tile_kernel (test tool):
// what the path takes from the ends of its sequence lines (phase_line_span, line_span_long_record) against the sum of
// seqline_is_long over the same tile -- the very functions of auriclass_amd/csrc/mhx_tile.h the HIP kernel runs, in the order
// it separates them with __syncthreads().
// Not part of the product; built by tests/test_parse_front.py with g++.
#include <cstdint>
#include <cstring>
#include "../../auriclass_amd/csrc/mhx_tile.h"

using namespace mhx;

enum : int {
    kOutTiles = 0,     // tiles run
    kOutByLines = 1,   // tiles that take the line path (line_items_try)
    kOutTooLong = 2,   // ... of which a sequence line is above the bound of phase_line_items: back to the maps through sm.misc[6]
    kOutCountDiff = 3, // line-path tiles whose span count differs from the sum of seqline_is_long
    kOutCheckDiff = 4, // line-path tiles where phase_event_checks<false> counts something, or flags another format verdict than <true>
    kOutRecords = 5,   // long records over all tiles, by seqline_is_long
    kOutSpanRecords = 6, // long records of the line-path tiles, from the spans
    kOutLine0 = 7,     // line-path tiles whose line 0 is a sequence line (it continues from the tile in front)
    kOutCount = 8
};

static TileSmem sm;
static ThreadState st[kBlock];

template <int K> static int records(const uint8_t *base, uint64_t begin, uint64_t end, uint32_t first_line, uint64_t *out)
{
    memset(out, 0, kOutCount * sizeof(uint64_t));
    const uint32_t first_tile = (uint32_t)(begin / kTileBytes);
    const uint32_t ntiles = (uint32_t)((end + kTileBytes - 1) / kTileBytes);
    uint32_t line_prefix = first_line;
    for (uint32_t tile = first_tile; tile < ntiles; ++tile) {
        const uint64_t tile_off = (uint64_t)tile * kTileBytes;
        const bool interior = tile_off >= begin && tile_off + kTileBytes + kHaloBytes <= end;
        const uint64_t span_left = end > tile_off ? end - tile_off : 0;
        const uint32_t check_limit = span_left < (uint64_t)(kTileBytes + kHaloBytes) ? (uint32_t)span_left : (uint32_t)(kTileBytes + kHaloBytes);
        for (int t = 0; t < kBlock; ++t) phase_stage(sm, t, base, tile_off, end);
        for (int t = 0; t < kBlock; ++t) phase_classify(sm, t, st[t], tile_off, begin, end, interior);
        uint32_t excl[kBlock], tile_total = 0;
        for (int t = 0; t < kBlock; ++t) { excl[t] = tile_total; tile_total += st[t].nlcount; }
        const uint32_t line_base = line_prefix & 3u;
        line_prefix += tile_total;
        ++out[kOutTiles];
        // the reference: seqline_is_long for the line behind every newline of the tile that starts a sequence line
        uint32_t ref = 0, e = 0;
        const uint8_t *tb = reinterpret_cast<const uint8_t *>(sm.bytes);
        for (uint32_t w = 0; w < (uint32_t)kTileBytes / 32; ++w)
            for (uint32_t m = tile_nlmap(sm)[w]; m; m &= m - 1u, ++e)
                if (((line_base + e + 1u) & 3u) == 1u && seqline_is_long(tile_nlmap(sm), tb, 32u * w + (uint32_t)__builtin_ctz(m) + 1u, tile_off, end, (uint32_t)K)) ++ref;
        out[kOutRecords] += ref;
        const bool fast_parse = parse_events_fit(tile_total);
        if (!(line_items_apply<K>() && line_items_try(fast_parse, interior, line_base, tile_total))) continue;
        // the line path as the kernel runs it up to the line-phase barrier
        ++out[kOutByLines];
        if (seqline_first(line_base) == 0u) ++out[kOutLine0];
        for (int t = 0; t < kBlock; ++t) phase_events(sm, t, st[t], excl[t]);
        bool bad_len = false, bad_nolen = false, too_long = false;
        uint32_t with_len = 0, without_len = 0, from_spans = 0;
        for (int t = 0; t < kBlock; ++t) {
            with_len += phase_event_checks<true>(sm, t, line_base, tile_total, check_limit, bad_len, tile_off, end, (uint32_t)K);
            without_len += phase_event_checks<false>(sm, t, line_base, tile_total, check_limit, bad_nolen, tile_off, end, (uint32_t)K);
            if (t < (int)kLineItemLines) {
                const LineSpan s = phase_line_span<K>(sm, (uint32_t)t, line_base, tile_total);
                from_spans += s.long_record;
                if (line_span_too_long(s)) too_long = true;
            }
        }
        if (too_long) ++out[kOutTooLong]; // the count stands as it is: the fall-back behind the barrier makes maps, it counts nothing
        out[kOutSpanRecords] += from_spans;
        if (from_spans != ref || with_len != ref) ++out[kOutCountDiff];
        if (without_len != 0 || bad_len != bad_nolen) ++out[kOutCheckDiff];
    }
    return 0;
}

// the span [begin, end) of base, which begins in line number first_line (mod 4) of its file
extern "C" int emul_parse_front_records(const uint8_t *base, uint64_t begin, uint64_t end, uint32_t first_line, int k, uint64_t *out8)
{
    switch (k) {
#define X(KK) case KK: return records<KK>(base, begin, end, first_line, out8);
        X(8) X(21) X(32)
#undef X
    default: return -1;
    }
}
