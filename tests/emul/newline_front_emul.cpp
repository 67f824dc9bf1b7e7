// tests/emul/newline_front_emul.cpp -- CPU check of the two front pieces of sketch_tile_kernel that work on fewer instructions
// (test tool): newline_mask, pair by pair, and the phase search from the newline list (selfsync_triple, selfsync_phase)
// against phase_selfsync -- the very functions of auriclass_amd/csrc/mhx_tile.h the HIP kernel runs, in its order.
// Not part of the product; built by tests/test_newline_front.py with g++.
#include <cstdint>
#include <cstring>
#include "../../auriclass_amd/csrc/mhx_tile.h"

using namespace mhx;

// newline mask of the 32 bytes at p (4-byte aligned): out[0] the kernel's form, out[1] the form for wave-uniform bytes,
// out[2] the form of before (one 32-bit multiply per pair).  On the host <true> and <false> are the same code, the 64-bit
// arithmetic: what is checked here is that arithmetic (no carry between bytes, the gather constants).  The device-only
// spelling of <true> -- the asm v_lshl_add_u64, the v_bitop3_b32 truth tables, the v_perm_b32 selectors -- is checked on
// the device only, by tests/test_gpu_newline_front.py.
extern "C" void emul_newline_mask(const uint32_t *p, uint32_t *out3)
{
    out3[0] = newline_mask<true>(p);
    out3[1] = newline_mask<false>(p);
    uint32_t n = 0;
    for (int d = 0; d < 8; d += 2) n |= flags_to_byte(byte_eq_flags(p[d], 0x0A0A0A0Au), byte_eq_flags(p[d + 1], 0x0A0A0A0Au)) << (4 * d);
    out3[2] = n;
}
// the flag words of a dword pair, and what the gather makes of them (its low byte is the mask, the rest strays)
extern "C" uint64_t emul_pair_flags(uint32_t v_lo, uint32_t v_hi) { return nl_pair_flags<true>(v_lo, v_hi); }
extern "C" uint32_t emul_pair_gather(uint32_t f_lo, uint32_t f_hi) { return nl_pair_gather(make64(f_lo, f_hi)); }

enum : int {
    kOutMap = 0,        // phase_selfsync of the tile (0 for the span's first tile, as the kernel has it)
    kOutTaken = 1,      // the list route is taken (selfsync_from_list)
    kOutList = 2,       // its answer (9: not taken)
    kOutWave0 = 3,      // newlines of the first wave's bytes
    kOutTotal = 4,      // newlines of the tile
    kOutAnyList = 5,    // the list's answer wherever the first wave lists six newlines, taken or not (9: fewer)
    kOutWholeList = 6,  // phase_selfsync_list wherever the tile has a list (9: it has none)
    kOutCount = 7
};

static TileSmem sm;
static ThreadState st[kBlock];

// One tile of the span [begin, end) of base, up to the barrier behind the phase search.  check_limit: 0xFFFFFFFF for the
// kernel's own (what of the staged bytes lies in the span), anything else to cut the search where the caller likes.
extern "C" int emul_selfsync(const uint8_t *base, uint64_t begin, uint64_t end, uint32_t tile, uint32_t limit_override, uint32_t *out)
{
    const uint32_t first_tile = (uint32_t)(begin / kTileBytes);
    const uint64_t tile_off = (uint64_t)tile * kTileBytes;
    if (tile < first_tile || tile_off >= end) return -1;
    const bool interior = tile_off >= begin && tile_off + kTileBytes + kHaloBytes <= end;
    const uint64_t span_left = end - tile_off;
    uint32_t check_limit = span_left < (uint64_t)(kTileBytes + kHaloBytes) ? (uint32_t)span_left : (uint32_t)(kTileBytes + kHaloBytes);
    if (limit_override != 0xFFFFFFFFu) check_limit = limit_override;
    for (int t = 0; t < kBlock; ++t) phase_stage(sm, t, base, tile_off, end);
    for (int t = 0; t < kBlock; ++t) phase_classify(sm, t, st[t], tile_off, begin, end, interior);
    uint32_t excl[kBlock], tile_total = 0, wave0 = 0;
    for (int t = 0; t < kBlock; ++t) { excl[t] = tile_total; tile_total += st[t].nlcount; if (t < 64) wave0 += st[t].nlcount; }
    // the search of the map first: the list lives in sm.valid, the map in sm.maps, neither touches the other
    out[kOutMap] = tile == first_tile ? 0u : phase_selfsync(sm, check_limit);
    out[kOutWave0] = wave0;
    out[kOutTotal] = tile_total;
    const bool fast_parse = parse_events_fit(tile_total);
    // the first wave reads the list behind its OWN phase_events, with no barrier: the other waves' entries are not there yet
    memset(sm.valid, 0xFF, sizeof(sm.valid));
    out[kOutTaken] = 0; out[kOutList] = 9; out[kOutAnyList] = 9; out[kOutWholeList] = 9;
    if (fast_parse) {
        for (int t = 0; t < 64; ++t) phase_events(sm, t, st[t], excl[t]);
        if (wave0 >= kSelfsyncNewlines) {
            uint32_t passing = 0;
            for (uint32_t lane = 0; lane < kSelfsyncTriples; ++lane) passing |= (selfsync_triple(sm, lane, check_limit) ? 1u : 0u) << lane;
            // the kernel's ballot carries the other 60 lanes' bits as zeros; give the formula stray bits above the four instead
            const uint32_t phase = selfsync_phase(passing | 0xFFFFFFF0u);
            out[kOutAnyList] = phase;
            if (selfsync_from_list(fast_parse, tile == first_tile, wave0)) { out[kOutTaken] = 1; out[kOutList] = phase; }
        }
        // the tiles the lanes do not take: thread 0, behind the barrier that completes the list
        for (int t = 64; t < kBlock; ++t) phase_events(sm, t, st[t], excl[t]);
        out[kOutWholeList] = phase_selfsync_list(sm, st[0], tile_total, check_limit);
    }
    return 0;
}
