// mhx_dist.h -- the logic of the all-vs-refs distance path that does not depend on how a GPU runs it, as host+device
// functions: the geometry rule (how many value ranges a call gets), the range index of a value, the offset rule of the
// split pass, the range table's probe and the spread of a reference mask into byte counters, the window totals and the
// finish walk (window totals -> cut window -> cut range -> two-pointer rule).  The kernels in mhx_dist.hip call these
// functions; tests/emul/dist_emul.cpp runs the same functions sequentially over whole batches on the CPU.
#pragma once
#include "mhx_hd.h"
#include "mhx_device_consts.h"

namespace mhx {

#ifndef MHX_DIST_RANGES
#define MHX_DIST_RANGES 1024
#endif
#ifndef MHX_DIST_SLOTS
#define MHX_DIST_SLOTS 2048
#endif
constexpr int kDistRanges = MHX_DIST_RANGES;     // value ranges the hash space is cut into (x W in the windowed form)
constexpr int kDistTableSlots = MHX_DIST_SLOTS; // LDS table of one range (refs' hashes of that range)
constexpr uint32_t kDistTableLimit = (kDistTableSlots * 3) / 4; // distinct keys a range's table may hold
constexpr uint32_t kDistSliceLimit = 255;          // entries of a (list, range) slice: its shared hashes are counted in bytes
constexpr int kDistSegs = 16;                    // finish kernel: the base form's ranges are summed in 16 segments first

// ---- geometry ---------------------------------------------------------------------------------------------------------
// A call gets R = kDistRanges * W value ranges, W a power of two chosen from the LENGTH of its longest list alone (never
// from the values): the smallest W that leaves at most kDistSliceTarget entries per (list, range) slice on average, so
// that slices stay as short as they are at s = 50 000 (49) whatever the sketch size -- the byte counters (255 entries per
// slice) and the range table (kDistTableLimit distinct keys over all references) are sized for slices of that length.
// W = 1 up to 65 536 entries, 16 at 2^20; longer lists have no geometry (0) and go to the generic pair kernel.
constexpr uint32_t kDistSliceTarget = 64;
constexpr uint32_t kDistMaxWindows = 16;
constexpr uint32_t kDistWindowRanges = 64; // ranges per window: the level between a pair and a range in the finish pass
static_assert(kDistRanges % (kDistSegs * kDistWindowRanges) == 0 && (kDistRanges & (kDistRanges - 1)) == 0, "range geometry");

MHX_HD uint32_t dist_windows(uint64_t longest)
{
    for (uint32_t W = 1; W <= kDistMaxWindows; W <<= 1)
        if (longest <= (uint64_t)kDistRanges * W * kDistSliceTarget) return W;
    return 0;
}

// Workspace of the windowed form per (query batch, reference slice) block: offsets 4 (R + 1) bytes per list, byte counters
// R * 4 ceil(nr / 4) per query (about 5 % of a query row of 64-entry slices), window totals a sixteenth of that again.  The
// host cuts the queries into batches of at most this many, so that a block's workspace stays below kDistWideWorkLimit
// (256 MiB: 450 queries against 32 references at R = 16 384) -- which also keeps every q * (R + 1) index below 2^32.
constexpr uint64_t kDistWideWorkLimit = 256ull << 20;
MHX_HD uint32_t dist_wide_max_queries(uint32_t nr, uint32_t ranges)
{
    const uint64_t cell = 4ull * ((nr + 3) / 4);
    const uint64_t per_query = 4ull * (ranges + 1) + ranges * cell + (ranges / kDistWindowRanges) * cell * 4;
    const uint64_t fixed = 4ull * nr * (ranges + 1) + 4 * 256; // the references' offsets, the rounding of the four arrays
    const uint64_t n = (kDistWideWorkLimit - fixed) / per_query;
    return n < 1 ? 1u : (uint32_t)n;
}

// value >> shift is a range index < ranges (a power of two) for every value <= maxval
MHX_HD uint32_t dist_shift_for(uint64_t maxval, uint32_t ranges)
{
    const int bits = maxval ? 64 - __builtin_clzll(maxval) : 1;
    const int lg = 31 - __builtin_clz(ranges);
    return bits > lg ? (uint32_t)(bits - lg) : 0u;
}
MHX_HD uint32_t dist_range_of(uint64_t v, uint32_t shift) { return (uint32_t)(v >> shift); }

// the range a workgroup of the range pass takes: consecutive workgroups go round the eight XCDs, so this order puts
// ranges p, p + 1, ... of one eighth of the value space on ONE XCD (its L2), close in time
MHX_HD uint32_t dist_range_of_block(uint32_t block, uint32_t ranges) { return (block & 7u) * (ranges / 8) + (block >> 3); }

// ---- split pass -------------------------------------------------------------------------------------------------------
// offs[p] = first element of the list whose range index is >= p, for p = 0 .. per - 1 (per = ranges + 1).  The work item of
// elements i and i + 1 (`two`: i + 1 < n) of a list of n writes the offsets that point at them: p in (range of the left
// neighbour, range of this element]; `from` is the left neighbour's range index + 1, or 0 for the list's first element,
// which also serves p = 0 .. its own range; the last work item leaves everything above its range at n.
MHX_HD void dist_split_offsets(uint32_t *offs, uint32_t per, uint32_t i, uint32_t n, bool two, uint32_t from, uint32_t r0, uint32_t r1)
{
    for (uint32_t p = from; p <= r0 && p < per; ++p) offs[p] = i;
    if (two) for (uint32_t p = r0 + 1; p <= r1 && p < per; ++p) offs[p] = i + 1;
    if (i + 2 >= n)
        for (uint32_t p = r1 + 1; p < per; ++p) offs[p] = n;
}

// ---- range pass -------------------------------------------------------------------------------------------------------
MHX_HD uint32_t dist_slot_of(uint64_t v) { return (uint32_t)((v * 0x9E3779B97F4A7C15ull) >> 40) & (kDistTableSlots - 1); }

// The table of one range: kDistTableSlots keys and kDistMaskWords masks.  A hash may be any 64-bit value, kEmptyKey (2^64 - 1)
// included -- the segmented sketch appends it behind a row's sorted values -- but a slot cannot hold the vacant-slot marker as
// a key: a compare-and-swap of kEmptyKey against kEmptyKey claims nothing, the slot stays vacant with the reference's bit on
// it, the next key to probe it inherits the bit, and a query that holds 2^64 - 1 reads the mask of whatever vacant slot ends
// its probe.  So that one value stays OUT of the slots: its references are kept in the mask word behind the last slot
// (kDistEmptyMask), insert and probe go there directly, and it does not count as a key of the table.
constexpr int kDistEmptyMask = kDistTableSlots;    // masks[kDistEmptyMask]: the references that hold kEmptyKey
constexpr int kDistMaskWords = kDistTableSlots + 1;

// bit mask of the references that hold v (0: none); the table always has vacant slots (kDistTableLimit).  v == kEmptyKey
// "matches" the first vacant slot of its probe and takes the word kept for it instead of that slot's.
MHX_HD uint32_t dist_table_probe(const unsigned long long *keys, const uint32_t *masks, uint64_t v)
{
    uint32_t sl = dist_slot_of(v), m = 0;
    for (;;) {
        const unsigned long long kx = keys[sl];
        if (kx == v) { m = masks[kx == kEmptyKey ? (uint32_t)kDistEmptyMask : sl]; break; }
        if (kx == kEmptyKey) break;
        sl = (sl + 1) & (kDistTableSlots - 1);
    }
    return m;
}

// One reference hash into the table, by ONE thread of control (the emulator's form; the kernels' dist_table_insert is this
// with atomicCAS / atomicOr in place of the plain accesses).  Returns the number of keys added: 0, 1, or kDistTableSlots
// when the table had no room at all.  kEmptyKey goes into its own mask word and adds no key.
MHX_HD uint32_t dist_table_insert_plain(unsigned long long *keys, uint32_t *masks, uint64_t v, uint32_t r)
{
    if (v == kEmptyKey) { masks[kDistEmptyMask] |= 1u << r; return 0u; }
    uint32_t sl = dist_slot_of(v);
    for (int probe = 0; probe < kDistTableSlots; ++probe) {
        const unsigned long long prev = keys[sl];
        if (prev == kEmptyKey || prev == v) { keys[sl] = v; masks[sl] |= 1u << r; return prev == kEmptyKey ? 1u : 0u; }
        sl = (sl + 1) & (kDistTableSlots - 1);
    }
    return (uint32_t)kDistTableSlots;
}

// a vacant table: every slot, and the word of kEmptyKey (work item `i` of `step` clears its share)
MHX_HD void dist_table_clear(unsigned long long *keys, uint32_t *masks, int i, int step)
{
    for (; i < kDistMaskWords; i += step) {
        if (i < kDistTableSlots) keys[i] = kEmptyKey;
        masks[i] = 0;
    }
}

// bits 4j .. 4j+3 of a reference mask -> the low bit of the four byte counters of word j
MHX_HD uint32_t dist_spread4(uint32_t m, int j) { return (((m >> (4 * j)) & 0xFu) * 0x00204081u) & 0x01010101u; }

// ---- window totals (windowed form) --------------------------------------------------------------------------------------
// Sum of word j of `n` (<= 257) consecutive cells of byte counters, `wstride` words apart: four totals, one per reference.
MHX_HD void dist_window_sum(const uint32_t *cell, uint32_t wstride, uint32_t n, uint32_t out[4])
{
    uint32_t lo = 0, hi = 0; // 16-bit lanes: bytes 0 and 2, bytes 1 and 3
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t x = cell[(uint64_t)i * wstride];
        lo += x & 0x00FF00FFu;
        hi += (x >> 8) & 0x00FF00FFu;
    }
    out[0] = lo & 0xFFFFu; out[1] = hi & 0xFFFFu; out[2] = lo >> 16; out[3] = hi >> 16;
}

// ---- finish pass ------------------------------------------------------------------------------------------------------
// One (query, reference) pair as the finish pass sees it.
struct DistPair {
    const uint8_t *cp;       // shared hashes of the pair in range p: cp[p * cstride]
    uint32_t cstride;
    const uint32_t *oq, *orr; // offsets of the query and of the reference, [ranges + 1]
    const uint64_t *A, *B;    // the reference's and the query's hashes
    uint32_t S;
};

MHX_HD uint32_t dist_range_union(const DistPair &x, uint32_t p0, uint32_t p1, uint32_t com)
{ // union elements of ranges p0 .. p1 - 1, `com` of them shared
    return (x.orr[p1] - x.orr[p0]) + (x.oq[p1] - x.oq[p0]) - com;
}

// Walk totals t = first .. end - 1 (union tu[t * stride], shared tc[t * stride]) while the union stays below S; returns the
// first t whose total carries it to S (the cut is inside t), `end` when there is none.
MHX_HD uint32_t dist_scan_totals(const uint32_t *tu, const uint32_t *tc, uint32_t stride, uint32_t first, uint32_t end, uint32_t S,
                                 uint32_t &uni, uint32_t &common)
{
    uint32_t t = first;
    for (; t < end; ++t) {
        if (uni + tu[t * stride] >= S) break;
        uni += tu[t * stride];
        common += tc[t * stride];
    }
    return t;
}

// The same over the ranges p0 .. p1 - 1 of a window that holds the cut: its last range is the cut at the latest.
MHX_HD uint32_t dist_scan_ranges(const DistPair &x, uint32_t p0, uint32_t p1, uint32_t &uni, uint32_t &common)
{
    uint32_t p = p0;
    for (; p + 1 < p1; ++p) {
        const uint32_t c = x.cp[(uint64_t)p * x.cstride];
        const uint32_t u = dist_range_union(x, p, p + 1, c);
        if (uni + u >= x.S) break;
        uni += u;
        common += c;
    }
    return p;
}

// The same over the windows w0 .. w1 - 1 (kDistWindowRanges ranges each, shared totals wt[win * wstride]) of a group of
// windows that holds the cut: its last window holds it at the latest.
MHX_HD uint32_t dist_scan_windows(const DistPair &x, const uint32_t *wt, uint32_t wstride, uint32_t w0, uint32_t w1, uint32_t &uni, uint32_t &common)
{
    uint32_t win = w0;
    for (; win + 1 < w1; ++win) {
        const uint32_t c = wt[(uint64_t)win * wstride];
        const uint32_t u = dist_range_union(x, win * kDistWindowRanges, (win + 1) * kDistWindowRanges, c);
        if (uni + u >= x.S) break;
        uni += u;
        common += c;
    }
    return win;
}

// The cut range, element by element with the sequential two-pointer rule (mash's compareSketches): it stops at the s-th
// union element.
MHX_HD void dist_two_pointer(const DistPair &x, uint32_t p, uint32_t &uni, uint32_t &common)
{
    uint32_t i = x.orr[p], j = x.oq[p];
    const uint32_t ie = x.orr[p + 1], je = x.oq[p + 1];
    while (uni < x.S && i < ie && j < je) {
        const uint64_t a = x.A[i], b = x.B[j];
        if (a < b) ++i;
        else if (b < a) ++j;
        else { ++i; ++j; ++common; }
        ++uni;
    }
}

} // namespace mhx
