// mhx_segsketch.h -- rules of the segmented sketch (`mash sketch -i` at buffer level: one bottom-s list per segment of an
// MHX_FMT_SEQ stream), written as host+device inline functions: mhx_segsketch.hip strings the phases together with
// __syncthreads(), the CPU emulator (tests/emul/segsketch_emul.cpp) runs the very same functions thread by thread.
//
// A segment is [seg_off[i], seg_off[i + 1]) of the stream.  A window is K bytes inside ONE segment, all A/C/G/T (either
// case); its value is the hash an MHX_FMT_SEQ push gives it (canonical strand, MurmurHash3_x64_128 seed 42, 32 bits for
// K <= 16).  Segments may touch: the cut is seg_off, not a separator byte.
//
// Segments of at most kSegCut windows ("small") take ONE workgroup each, and everything stays in LDS:
//   stage   the segment's bytes (whole aligned dwords around them) into LDS
//   hash    one window per lane and turn: base check, reverse complement, strand choice, hash -> keys[w]
//           (a window that holds anything but A/C/G/T leaves the vacant key)
//   sort    bitonic network over the next power of two >= the window count, vacant keys last
//   select  first occurrence of every value, numbered by a workgroup scan, the first s written to the segment's row
// No admission threshold, no table, no retry: every window of the segment is in the sort, so the row is exact by
// construction.  Larger segments go through the sketcher on their slice of the stream (mhx_engine_segments.cpp).
#pragma once
#include <stdint.h>

#include "mhx_tile.h"

namespace mhx {

// L: the most windows one workgroup takes.  4096 keys of 8 bytes are 32 KiB of LDS; with the staged bytes and the scan words
// a workgroup holds 37.1 KiB, four of them fit the 160 KiB of a CU (16 waves), and a 2 kb or 4 kb record -- plasmid genes,
// marker loci -- stays on this side of the cut.  8192 would leave two workgroups per CU to hide ~80 barriers each.
constexpr uint32_t kSegCut = 4096;
constexpr uint32_t kSegBlock = 256;
// staged image: up to 3 bytes of misalignment + kSegCut + 31 bytes of a small segment, and the dword a window's last
// funnel shift reads past its end: (3 + 4095) / 4 + 8 = 1032 is the last index read
constexpr uint32_t kSegStageDwords = 1040;
static_assert((3 + kSegCut - 1) / 4 + 8 < kSegStageDwords && (3 + kSegCut + 31 + 3) / 4 <= kSegStageDwords, "staged image of a small segment");

struct SegSmem {
    uint64_t keys[kSegCut];             // one hash per window, kEmptyKey for none; sorted in place
    uint32_t bytes[kSegStageDwords];    // the segment's bytes from the aligned dword in front of it on, zero behind
    uint32_t scan[kSegBlock];           // distinct values in each thread's share of the sorted keys
    uint32_t misc[4];                   // 0: a window hashed to kEmptyKey itself (2^64 - 1: cannot stand in keys[])
};

// windows of k bytes inside [b, e)
MHX_HD uint64_t seg_windows(uint64_t b, uint64_t e, int k) { return e >= b + (uint64_t)k ? e - b - (uint64_t)k + 1 : 0; }
MHX_HD bool seg_is_small(uint64_t windows) { return windows <= kSegCut; }
// keys the sort network runs over: the power of two >= windows (>= 2; windows in 1..kSegCut)
MHX_HD uint32_t seg_sort_size(uint32_t windows)
{
    uint32_t n = 2;
    while (n < windows) n <<= 1;
    return n;
}
// byte offset of the segment's first byte inside the staged image
MHX_HD uint32_t seg_misalign(const uint8_t *first) { return (uint32_t)((uintptr_t)first & 3u); }

// P1: stage.  Dword d of the image is the aligned dword at (first & ~3) + 4 d; dwords that hold no byte of the segment
// are zero.  The bytes of the first and last dword that lie outside the segment belong to its neighbours (or to the
// allocation's padding): no window of this segment covers them.
MHX_HD void seg_phase_stage(SegSmem &sm, uint32_t tid, const uint8_t *first, uint32_t nbytes)
{
    const uint32_t mis = seg_misalign(first);
    const uint32_t *src = reinterpret_cast<const uint32_t *>(first - mis);
    const uint32_t nd = (mis + nbytes + 3) / 4;
    for (uint32_t d = tid; d < kSegStageDwords; d += kSegBlock) sm.bytes[d] = d < nd ? src[d] : 0u;
    if (tid == 0) sm.misc[0] = 0;
}

// The window at byte `pos` of the staged image: false when it holds anything but A/C/G/T (mash skips it), else its hash.
// The steps are those of process_deferred (mhx_tile.h), which finishes a queued candidate of the sketch kernel the same way.
template <int K> MHX_HD bool seg_window_hash(const uint32_t *image, uint32_t pos, uint64_t &h)
{
    constexpr int NW = (K + 3) / 4;
    constexpr uint32_t tail_mask = (K % 4) ? (1u << (8 * (K % 4))) - 1u : 0xFFFFFFFFu;
    const uint32_t *b = image + (pos >> 2);
    const uint32_t sh = 8u * (pos & 3u);
    uint32_t wf[8], wr[8], rev[NW + 1];
    uint32_t ok_bits = 0;
#pragma unroll
    for (int d = 0; d < NW; ++d) {
        const uint32_t raw = funnel_bits(b[d + 1], b[d], sh);
        ok_bits |= flags_to_nibble(acgt_flags(raw)) << (4 * d);
        wf[d] = raw & 0xDFDFDFDFu; // fold case
    }
    constexpr uint32_t want = (uint32_t)((1ull << K) - 1ull);
    if ((ok_bits & want) != want) return false;
    wf[NW - 1] &= tail_mask;
#pragma unroll
    for (int d = NW; d < 8; ++d) wf[d] = 0u;
    // reverse complement: the 4 * NW bytes reversed and complemented put the window's K bytes behind 4 * NW - K bytes of padding
#pragma unroll
    for (int d = 0; d < NW; ++d) rev[d] = __builtin_bswap32(complement4(wf[NW - 1 - d]));
    rev[NW] = 0u;
    constexpr uint32_t pad_bits = 8u * (4 * NW - K);
#pragma unroll
    for (int d = 0; d < 8; ++d) wr[d] = d < NW ? (pad_bits ? funnel_bits(rev[d + 1], rev[d], pad_bits) : rev[d]) : 0u;
    const bool rc = rc_is_smaller_full<NW>(wf, wr);
    uint32_t w[8];
#pragma unroll
    for (int d = 0; d < 8; ++d) w[d] = rc ? wr[d] : wf[d];
    const Murmur3Tail tail = murmur3_core<K>(w);
    h = K <= 16 ? (uint64_t)tail.low32() : tail.finish();
    return true;
}

// P2: hash.  keys[w] for every w below the sort size: the window's hash, kEmptyKey for an invalid window and for padding.
template <int K> MHX_HD void seg_phase_hash(SegSmem &sm, uint32_t tid, uint32_t mis, uint32_t windows, uint32_t nsort)
{
    for (uint32_t w = tid; w < nsort; w += kSegBlock) {
        uint64_t key = kEmptyKey, h;
        if (w < windows && seg_window_hash<K>(sm.bytes, mis + w, h)) {
            if (h == kEmptyKey) sm.misc[0] = 1; // appended behind the sorted values by the select phase
            else key = h;
        }
        sm.keys[w] = key;
    }
}

// P3: one step of the bitonic network (size = 2, 4, .. nsort; stride = size / 2, .. 1), a barrier between steps
MHX_HD void seg_sort_step(SegSmem &sm, uint32_t tid, uint32_t nsort, uint32_t size, uint32_t stride)
{
    for (uint32_t t = tid; t < nsort / 2; t += kSegBlock) {
        const uint32_t i = 2 * t - (t & (stride - 1)), j = i + stride;
        const uint64_t a = sm.keys[i], b = sm.keys[j];
        const bool up = (i & size) == 0;
        if ((a > b) == up) { sm.keys[i] = b; sm.keys[j] = a; }
    }
}

// P4: select.  Thread tid owns keys [tid * per, (tid + 1) * per) of the sorted list, per = max(1, nsort / kSegBlock).
MHX_HD uint32_t seg_share(uint32_t nsort) { return nsort > kSegBlock ? nsort / kSegBlock : 1u; }
MHX_HD bool seg_is_first(const SegSmem &sm, uint32_t i) { return sm.keys[i] != kEmptyKey && (i == 0 || sm.keys[i] != sm.keys[i - 1]); }
MHX_HD void seg_phase_count(SegSmem &sm, uint32_t tid, uint32_t nsort)
{
    const uint32_t per = seg_share(nsort);
    uint32_t c = 0;
    for (uint32_t i = tid * per; i < (tid + 1) * per && i < nsort; ++i) c += seg_is_first(sm, i) ? 1u : 0u;
    sm.scan[tid] = c;
}
// the first `cap` = min(s, stride) distinct values go to `row`, ascending; the thread that owns the end of the list
// appends the value 2^64 - 1 if a window had it and writes the row's length
MHX_HD void seg_phase_write(const SegSmem &sm, uint32_t tid, uint32_t nsort, uint32_t cap, uint64_t *row, uint32_t *len)
{
    const uint32_t per = seg_share(nsort);
    if (tid * per >= nsort) return;
    uint32_t pos = 0;
    for (uint32_t t = 0; t < tid; ++t) pos += sm.scan[t];
    for (uint32_t i = tid * per; i < (tid + 1) * per; ++i)
        if (seg_is_first(sm, i)) {
            if (pos < cap) row[pos] = sm.keys[i];
            ++pos;
        }
    if ((tid + 1) * per >= nsort) {
        if (sm.misc[0]) {
            if (pos < cap) row[pos] = kEmptyKey;
            ++pos;
        }
        *len = pos < cap ? pos : cap;
    }
}

} // namespace mhx
