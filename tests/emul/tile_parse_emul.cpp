// tests/emul/tile_parse_emul.cpp -- CPU comparison of the two FASTQ good-map forms of sketch_tile_kernel (test tool).
// Runs, tile by tile and thread by thread, phase_good (the per-newline loops) and phase_events + phase_good_events
// (auriclass_amd/csrc/mhx_tile.h, the very functions the HIP kernel runs) on the same staged tile, in the order the
// kernel separates them with __syncthreads(), and compares what they leave behind: every word of the good map (tile
// and halo), the bad-format flag and the number of long records.  Also exports murmur3_h1<K> for one window.
// Not part of the product; built by tests/test_tile_parse_emulation.py with g++.
#include <cstdint>
#include <cstring>
#include "../../auriclass_amd/csrc/mhx_tile.h"

using namespace mhx;

enum : int {
    kOutTiles = 0,        // tiles run
    kOutFallback = 1,     // tiles the event list does not hold (parse_events_fit false): phase_good is what runs
    kOutGoodDiff = 2,     // tiles whose good maps differ
    kOutBadDiff = 3,      // tiles whose bad-format flags differ
    kOutCountDiff = 4,    // tiles whose long-record counts differ
    kOutBadTiles = 5,     // tiles phase_good flags
    kOutRecords = 6,      // long records, phase_good
    kOutLines = 7,        // newlines
    kOutCount = 8
};

extern "C" int emul_parse_compare(const uint8_t *base, uint64_t begin, uint64_t end, uint32_t k, uint64_t *out8)
{
    static TileSmem sm;
    static ThreadState st[kBlock];
    constexpr int kGoodWords = kTileBytes / 32 + 4;
    memset(out8, 0, kOutCount * sizeof(uint64_t));
    const uint32_t first_tile = (uint32_t)(begin / kTileBytes);
    const uint32_t ntiles = (uint32_t)((end + kTileBytes - 1) / kTileBytes);
    uint32_t line_prefix = 0;
    for (uint32_t tile = first_tile; tile < ntiles; ++tile) {
        const uint64_t tile_off = (uint64_t)tile * kTileBytes;
        for (int t = 0; t < kBlock; ++t) phase_stage(sm, t, base, tile_off, end);
        const bool interior = tile_off >= begin && tile_off + kTileBytes + kHaloBytes <= end;
        for (int t = 0; t < kBlock; ++t) phase_classify(sm, t, st[t], tile_off, begin, end, interior);
        uint32_t excl[kBlock], tile_total = 0;
        for (int t = 0; t < kBlock; ++t) { excl[t] = tile_total; tile_total += st[t].nlcount; } // the kernel's block_scan_excl
        const uint32_t line_base = line_prefix; // the running line count: what self-synchronisation or the look-back gives
        line_prefix += tile_total;
        const uint64_t span_left = end > tile_off ? end - tile_off : 0;
        const uint32_t check_limit = span_left < (uint64_t)(kTileBytes + kHaloBytes) ? (uint32_t)span_left : (uint32_t)(kTileBytes + kHaloBytes);
        ++out8[kOutTiles];
        out8[kOutLines] += tile_total;

        bool bad_ref = false;
        uint32_t count_ref = 0, good_ref[kGoodWords];
        for (int t = 0; t < kBlock; ++t) count_ref += phase_good<true>(sm, t, st[t], line_base, excl[t], tile_total, check_limit, bad_ref, tile_off, end, k);
        memcpy(good_ref, tile_good(sm), sizeof(good_ref));
        out8[kOutRecords] += count_ref;
        if (bad_ref) ++out8[kOutBadTiles];

        if (!parse_events_fit(tile_total)) { ++out8[kOutFallback]; continue; }
        memset(tile_good(sm), 0xA5, sizeof(good_ref)); // nothing of the first form's result may stand in for the second's
        memset(sm.valid, 0xFF, sizeof(sm.valid));
        for (int t = 0; t < kBlock; ++t) phase_events(sm, t, st[t], excl[t]);
        bool bad_new = false;
        uint32_t count_new = 0;
        for (int t = 0; t < kBlock; ++t) count_new += phase_good_events(sm, t, st[t], line_base, excl[t], tile_total, check_limit, bad_new, tile_off, end, k);
        if (memcmp(good_ref, tile_good(sm), sizeof(good_ref)) != 0) ++out8[kOutGoodDiff];
        if (bad_ref != bad_new) ++out8[kOutBadDiff];
        if (count_ref != count_new) ++out8[kOutCountDiff];
    }
    return 0;
}

// seqline_mask (the loop) against seqline_mask_bits on single words; returns the number of words that differ
extern "C" uint64_t emul_mask_compare(const uint32_t *words, uint64_t n)
{
    uint64_t diff = 0;
    for (uint64_t i = 0; i < n; ++i)
        for (uint32_t line = 0; line < 4; ++line) {
            bool ignore = false;
            if (seqline_mask(words[i], line, nullptr, 0, 0, ignore) != seqline_mask_bits(words[i], line)) ++diff;
        }
    return diff;
}

extern "C" int emul_murmur3_h1(int k, const uint32_t *w8, uint64_t *h)
{
    uint32_t w[8];
    memcpy(w, w8, sizeof(w));
    switch (k) {
#define X(KK) case KK: *h = murmur3_h1<KK>(w); return 0;
        X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10) X(11) X(12) X(13) X(14) X(15) X(16)
        X(17) X(18) X(19) X(20) X(21) X(22) X(23) X(24) X(25) X(26) X(27) X(28) X(29) X(30) X(31) X(32)
#undef X
    default: return -1;
    }
}
