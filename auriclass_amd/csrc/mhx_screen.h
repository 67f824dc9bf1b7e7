// mhx_screen.h -- the rules of the containment screen (`mash screen`) that are more than a line: geometry of the screen
// table, the walk of a probe sequence, the build step that claims a slot, the counter that must not wrap and the selection
// of a reference's median multiplicity, and the winner-take-all form of the tally (`-w`: priority order, claim, "won").
// Host+device functions: the kernels (mhx_screen.hip, mhx_sketch.hip) and the CPU emulators (tests/emul/screen_emul.cpp,
// tests/emul/screen_winner_emul.cpp) run these very functions.
//
// The screen table is the candidate table's sibling: keys u64[2^n], vacant = 2^64-1 (kEmptyKey), cnts u32[2^n], slot =
// hash & mask, linear probing.  It is built once from the reference rows (duplicates across references collapse into one
// key), then only read: a window of the read set whose hash is a key adds one to that key's counter, any other window
// changes nothing.  The hash value 2^64-1 cannot be a key; its occurrences are counted in a word of their own.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

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

// Winner-take-all (`mash screen -w`): every hash found in the reads is credited to ONE of the references that hold it, the
// best by (score, genome length, lowest index), score = the plain screen's shared / n.  The order of the scores is the
// order of the exact ratios (pow(x, 1 / k) is monotone), so it is decided in integers: shared_a * n_b against shared_b *
// n_a, both below 2^63 for lists of up to 2^31 entries.  A reference without entries holds no hash and is ranked last.
// The order becomes one word per reference, the priority: unique, greater is better, kScreenNobody (0) is nobody's.
// A winner word per table slot (win[nslots], and win[nslots] itself for the hash value 2^64-1, which is not a key) starts
// at kScreenNobody; every entry whose key was seen raises the key's word to its reference's priority (claim); the tally
// then keeps a count only where the word equals the reference's priority (won).
constexpr uint32_t kScreenNobody = 0;

// a ranks before b (strictly).  length: genome lengths, nullptr = all equal.
inline bool screen_ranks_before(const uint32_t *shared0, const uint32_t *len, const uint64_t *length, uint32_t a, uint32_t b)
{
    if ((len[a] == 0) != (len[b] == 0)) return len[a] != 0;
    const uint64_t sa = (uint64_t)shared0[a] * len[b], sb = (uint64_t)shared0[b] * len[a];
    if (sa != sb) return sa > sb;
    if (length && length[a] != length[b]) return length[a] > length[b];
    return a < b;
}

// prio[nr]: nr for the best reference down to 1 for the last.  Host only (the plain tally's shared0 is on the host anyway).
inline void screen_priorities(const uint32_t *shared0, const uint32_t *len, const uint64_t *length, uint32_t nr, uint32_t *prio)
{
    std::vector<uint32_t> order(nr);
    for (uint32_t i = 0; i < nr; ++i) order[i] = i;
    std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return screen_ranks_before(shared0, len, length, a, b); });
    for (uint32_t at = 0; at < nr; ++at) prio[order[at]] = nr - at;
}

// the winner word of hash h: a slot, mask + 1 for the hash value 2^64-1, kScreenAbsent when h is not a key
MHX_HD uint64_t screen_winner_word(const uint64_t *keys, uint64_t mask, uint64_t h)
{
    return h == kEmptyKey ? mask + 1 : screen_find(keys, mask, h);
}

// Claim: the entry h of a reference with priority prio.  raise(word, prio) lifts win[word] to at least prio -- an
// atomicMax on the device.
template <class Raise>
MHX_HD void screen_claim(const uint64_t *keys, const uint32_t *cnts, uint64_t mask, uint64_t h, uint64_t maxkey, uint32_t prio, Raise &raise)
{
    const uint64_t w = screen_winner_word(keys, mask, h);
    if (w == kScreenAbsent) return;
    if (w > mask ? maxkey != 0 : cnts[w] != 0u) raise(w, prio);
}

MHX_HD bool screen_won(uint32_t winner_word, uint32_t prio) { return winner_word == prio; }

// count of hash h as the winner tally reads it for the reference with priority prio: screen_count_of where that
// reference won h, 0 elsewhere
MHX_HD uint32_t screen_count_won(const uint64_t *keys, const uint32_t *cnts, const uint32_t *win, uint64_t mask, uint64_t h,
                                 uint64_t maxkey, uint32_t prio)
{
    const uint64_t w = screen_winner_word(keys, mask, h);
    if (w == kScreenAbsent || !screen_won(win[w], prio)) return 0u;
    if (w > mask) return maxkey < kScreenCountLimit ? (uint32_t)maxkey : kScreenCountLimit;
    return cnts[w];
}

} // namespace mhx
