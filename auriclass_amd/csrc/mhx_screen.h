// mhx_screen.h -- the rules of the containment screen (`mash screen`) that are more than a line: geometry of the screen
// table, the walk of a probe sequence, the build step that claims a slot, the counter that must not wrap and the selection
// of a reference's median multiplicity.  Host+device functions: the kernels (mhx_kernels.hip) and the CPU emulator
// (tests/emul/screen_emul.cpp) run these very functions.
//
// The screen table is the candidate table's sibling: keys u64[2^n], vacant = 2^64-1 (kEmptyKey), cnts u32[2^n], slot =
// hash & mask, linear probing.  It is built once from the reference rows (duplicates across references collapse into one
// key), then only read: a window of the read set whose hash is a key adds one to that key's counter, any other window
// changes nothing.  The hash value 2^64-1 cannot be a key; its occurrences are counted in a word of their own.
#pragma once
#include <stdint.h>

#include "mhx_device_consts.h"
#include "mhx_hd.h"

namespace mhx {

constexpr uint64_t kScreenMinSlots = 1024;
constexpr uint64_t kScreenAbsent = ~0ull;           // screen_find: the hash is not a key
// A counter stops here: an increment that finds it at or beyond this value is taken back and raises kFlagCountWrap.  The
// margin to 2^32 (2^28 increments that would all have to be in flight at once) is what makes "taken back" race-free.
constexpr uint32_t kScreenCountLimit = 0xF0000000u;

// slots for `entries` reference hashes (duplicates counted: an upper bound of the distinct keys): a power of two, at least
// twice the entries, so that a probe sequence always meets a vacant slot
MHX_HD uint64_t screen_table_slots(uint64_t entries)
{
    uint64_t n = kScreenMinSlots;
    while (n < 2 * entries) n <<= 1;
    return n;
}

// Build: the slot of key h, claimed if nobody holds it yet.  claim(slot, h) stores h into a vacant slot and returns what
// the slot held before (kEmptyKey: claimed now) -- a 64-bit compare-and-swap on the device.  kScreenAbsent: no room
// (cannot happen in a table sized by screen_table_slots).
template <class Claim> MHX_HD uint64_t screen_insert(uint64_t mask, uint64_t h, Claim &claim)
{
    uint64_t slot = h & mask;
    for (uint64_t i = 0; i <= mask; ++i) {
        const uint64_t prev = claim(slot, h);
        if (prev == kEmptyKey || prev == h) return slot;
        slot = (slot + 1) & mask;
    }
    return kScreenAbsent;
}

// Probe: the slot that holds h, or kScreenAbsent when a vacant slot comes first.  Plain loads: nobody writes keys after
// the build.
MHX_HD uint64_t screen_find(const uint64_t *keys, uint64_t mask, uint64_t h)
{
    uint64_t slot = h & mask;
    for (uint64_t i = 0; i <= mask; ++i) {
        const uint64_t key = keys[slot];
        if (key == h) return slot;
        if (key == kEmptyKey) return kScreenAbsent;
        slot = (slot + 1) & mask;
    }
    return kScreenAbsent;
}

// the counter after an increment that found it at `before`: true = the increment stands
MHX_HD bool screen_count_stands(uint32_t before) { return before < kScreenCountLimit; }

// count of hash h as the tally reads it (maxkey: occurrences of the hash value 2^64-1, clipped like a counter)
MHX_HD uint32_t screen_count_of(const uint64_t *keys, const uint32_t *cnts, uint64_t mask, uint64_t h, uint64_t maxkey)
{
    if (h == kEmptyKey) return maxkey < kScreenCountLimit ? (uint32_t)maxkey : kScreenCountLimit;
    const uint64_t slot = screen_find(keys, mask, h);
    return slot == kScreenAbsent ? 0u : cnts[slot];
}

// Median of a reference: element [len / 2] of the ascending list of its non-zero counts, found without sorting by four
// passes over the counts, eight bits each from the top (radix select).  A pass histograms digit `screen_select_digit(c,
// shift)` of the counts that `screen_select_match` lets through (non-zero, and equal to the digits chosen so far above the
// current one); screen_select_step then picks the digit that holds the wanted rank and makes the rank relative to it.
constexpr int kScreenSelectBins = 256;
MHX_HD bool screen_select_match(uint32_t c, uint32_t prefix, int shift)
{
    return c != 0u && (shift == 24 || (c >> (shift + 8)) == prefix);
}
MHX_HD uint32_t screen_select_digit(uint32_t c, int shift) { return (c >> shift) & 255u; }
MHX_HD uint32_t screen_select_step(const uint32_t *hist, uint32_t &rank)
{
    uint32_t d = 0;
    while (d + 1 < (uint32_t)kScreenSelectBins && rank >= hist[d]) { rank -= hist[d]; ++d; }
    return d;
}

} // namespace mhx
