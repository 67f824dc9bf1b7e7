// mhx_tile.h -- per-tile logic of the sketch kernel, written as host+device inline
// functions: mhx_sketch.hip strings the phases together with __syncthreads(); the CPU
// phase emulator (tests/emul/tile_emul.cpp) runs the very same functions thread by
// thread so that indexing and bit logic are checked without a GPU.
//
// What one tile does (replaces mash's kseq_read + addMinHashes + getHash hot loop,
// Mash 2.x Sketch.cpp; reached from /root/reference/auriclass/classes.py:576-596,696-713):
//   stage     16 KiB (+64 B halo) of the byte stream into LDS, 16 B per lane, coalesced
//   classify  per byte: newline?                                 -> bit mask (SIMD-in-register)
//   phase     FASTQ: newline prefix -> line number mod 4 == 1 marks sequence lines
//   runs      candidate k-mer starts = K bytes inside one line   -> 1 bit per position
//   compact   groups of 8 start positions with any candidate     -> LDS work list
//   work      each lane takes a group: 8 windows share one 28..39 byte register chunk;
//             canonical strand by big-endian compare, MurmurHash3_x64_128(seed 42) up to the last
//             multiplication, a 32-bit necessary test against the global threshold; the few
//             windows that pass finish the hash, are checked base by base (A/C/G/T, either
//             case -- mash skips every window holding anything else) and go into the table.
// The base check is deferred on purpose: one window in 10^4..10^6 is ever a candidate, so
// testing every byte of the stream for A/C/G/T up front cost more than hashing the rare
// window that holds an N (its hash is garbage, it passes the threshold as rarely as any
// other, and the exact check then drops it).
#pragma once
#include <stdint.h>
#include <type_traits>

#include "mhx_hd.h"
#include "mhx_device_consts.h"
#include "mhx_tail_lut.h"

// rare branches are laid out of line: the hot path falls through instead of jumping over the cold block
#define MHX_UNLIKELY(x) __builtin_expect(!!(x), 0)

namespace mhx {

constexpr int kMapWords = (kTileBytes + kHaloBytes) / 32 + 2; // words of a 1-bit-per-byte map of tile + halo (+2 look-ahead)
// The queue form of the kernel (large sketches, early launches; process_group_regs<K, true>): windows whose partial
// hash passes the admission test are not finished where they are found -- one candidate lane would take the other 63
// through the cold code (hash tail, exact compare, base check, two atomics: ~100 instructions), and with s = 50 000 (one
// window in 230 below T) that happens in every fourth wave-iteration -- but queued as (group << 3) | window in the part of
// the work list the tile's items leave free (list[nitems ..)) and finished together after the hash loop, one per lane
// (process_deferred).  A window that finds the queue full is finished at once.
struct TileSmem {
    uint4 bytes[(kTileBytes + kHaloBytes) / 16];      // staged stream bytes
    uint32_t valid[kGroupsPerTile / 4];                // byte g = candidate-start mask of group g
    // One area, three tenants with disjoint lifetimes: the newline map (classify -> good-map phase) and the
    // good map (good-map phase -> candidate starts) side by side, then the work list (compaction -> hash loop).
    // 22.7 KB of LDS per workgroup in all: seven workgroups per CU.
    union {
        uint16_t list[kGroupsPerTile];                 // compacted work list (group ids)
        uint32_t maps[2 * kMapWords];
    };
    uint32_t cnt[16];                                  // wave partials of the two workgroup scans
    uint32_t misc[8];                                  // 0: line base, 1: #items, 2: tile id, 3: k-mers, 4: inserts, 5: long records, 6: a sequence line too long for phase_line_items, 7: #queued candidates
};

MHX_HD uint32_t *tile_nlmap(TileSmem &sm) { return sm.maps; }             // 1 bit per byte: newline
MHX_HD uint32_t *tile_good(TileSmem &sm) { return sm.maps + kMapWords; } // 1 bit per byte: may be covered by a k-mer

// per-thread state carried between phases (registers on the GPU)
struct ThreadState {
    uint32_t nl[kWordsPerThread];  // newline mask of this thread's 32-byte words (bytes outside the span cleared)
    uint32_t in[kWordsPerThread];  // bytes of those words that lie inside the span
    uint32_t hnl[2], hin[2];       // thread 0 only: the two halo words
    uint32_t nlcount;
};

// ---- byte-parallel helpers ----------------------------------------------------------
MHX_HD uint32_t zero_byte_flags(uint32_t y)
{ // 0x80 in every byte of y that is zero (exact, no cross-byte carries)
    uint32_t t = (y & 0x7F7F7F7Fu) + 0x7F7F7F7Fu;
    return ~(t | y | 0x7F7F7F7Fu);
}
MHX_HD uint32_t flags_to_nibble(uint32_t f)
{ // bits 7,15,23,31 -> bits 0..3
    return (f * 0x00204081u) >> 28;
}
MHX_HD uint32_t perm_lut(uint32_t lut, uint32_t sel)
{ // out.byte[i] = lut.byte[sel.byte[i]]  (selectors 0..3)
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_perm(lut, lut, sel);
#else
    uint32_t o = 0;
    for (int i = 0; i < 4; ++i) o |= ((lut >> (8 * ((sel >> (8 * i)) & 3))) & 0xFFu) << (8 * i);
    return o;
#endif
}
// 2-bit index of a (case-folded) byte: bits 1..2, which tell A, C, G, T apart (0, 1, 3, 2); any other
// byte lands on one of the four as well and is exposed by the comparison with the table entry
MHX_HD uint32_t base_index(uint32_t u) { return (u >> 1) & 0x03030303u; }
constexpr uint32_t kLutBase = 0x47544341u; // index -> 'A','C','T','G'
constexpr uint32_t kLutComp = 0x43414754u; // index -> complement: 'T','G','A','C'

// low 32 bits of {hi:lo} >> (8 * byte_shift), byte_shift in 0..3.  On the device this must be
// the v_alignbyte/v_alignbit instruction itself: written as a C shift-or, LLVM turns the
// pattern into an unaligned load from a stack copy of the register array (scratch traffic).
MHX_HD uint32_t funnel(uint32_t hi, uint32_t lo, int byte_shift)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_alignbyte(hi, lo, (uint32_t)byte_shift);
#else
    return (uint32_t)(((((uint64_t)hi) << 32) | lo) >> (8 * byte_shift));
#endif
}
// value the optimiser must treat as unknown at this point (pins cold-path work behind its branch)
MHX_HD uint32_t opaque(uint32_t v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("" : "+v"(v));
#endif
    return v;
}
// a value that is the same in every active lane (or held by the only active one), as a scalar: v_readfirstlane_b32
MHX_HD uint32_t wave_uniform(uint32_t v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_readfirstlane(v);
#else
    return v;
#endif
}
// is v true in any active lane?  (the host runs one lane at a time)
MHX_HD bool wave_any(bool v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_ballot_w64(v) != 0ull;
#else
    return v;
#endif
}
MHX_HD uint32_t funnel_bits(uint32_t hi, uint32_t lo, uint32_t bit_shift)
{ // bit_shift in 0..31
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_alignbit(hi, lo, bit_shift);
#else
    return (uint32_t)(((((uint64_t)hi) << 32) | lo) >> bit_shift);
#endif
}
// WIDTH bits of v from bit `shift` on (shift + WIDTH <= 32, WIDTH < 32): one v_bfe_u32 with a run-time offset
template <uint32_t WIDTH> MHX_HD uint32_t bit_field(uint32_t v, uint32_t shift)
{
    static_assert(WIDTH > 0 && WIDTH < 32, "field width");
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_ubfe(v, shift, WIDTH);
#else
    return (v >> shift) & ((1u << WIDTH) - 1u);
#endif
}
// a ^ b ^ c as one v_bitop3_b32 (truth table 0x96); hipcc's own choice for two chained xors is two v_xor_b32
MHX_HD uint32_t xor3(uint32_t a, uint32_t b, uint32_t c)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_bitop3_b32(a, b, c, 0x96);
#else
    return a ^ b ^ c;
#endif
}

// 0x80 in every byte of v that equals the byte replicated in `pattern` (exact).  One instruction less than
// zero_byte_flags(v ^ pattern): the xor-ed word itself is never needed, only its low seven bits per byte (one v_bitop3:
// (v ^ pattern) & 0x7F7F7F7F) and its top bits, which for patterns below 0x80 are v's own top bits.
MHX_HD uint32_t byte_eq_flags(uint32_t v, uint32_t pattern)
{
    const uint32_t t = ((v ^ pattern) & 0x7F7F7F7Fu) + 0x7F7F7F7Fu;
    return ~(t | v) & 0x80808080u;
}
// flags (0x80 per byte) of two consecutive dwords -> 8 mask bits, low dword first, with ONE multiplication: the first
// dword's flags move to bit 3 of each byte, the second's stay at bit 7; times 0x00204081 the eight flags land in bits
// 24..31 in byte order (the stray partial products fall on distinct bits below 24 or beyond 31, so nothing carries).
MHX_HD uint32_t flags_to_byte(uint32_t f_lo, uint32_t f_hi) { return (((f_lo >> 4) | f_hi) * 0x00204081u) >> 24; }

// ---- newline mask of one 32-byte word (8 dwords at p) ---------------------------------
// Two dwords at a time ("The newline map on fewer instructions"):
//   flags   byte_eq_flags on the pair.  ((v ^ 0x0A..) & 0x7F..) + 0x7F.. is at most 0xFE per byte, so nothing carries from
//           a byte into the next, nor from the low dword into the high one: the add of a pair is ONE 64-bit add
//           (v_lshl_add_u64 with shift 0, the constant in an SGPR pair); the xor-and in front of it and the
//           ~(t | v) & 0x80.. behind it stay one v_bitop3_b32 per dword.  Five instructions per pair.
//   gather  with f_lo, f_hi the flag words (bits 7, 15, 23, 31), f_lo * 0x02040810 + f_hi * 0x20408100 as a 64-bit value
//           holds the eight flags in byte order in bits 32..39: f_lo's land there from 7 + 25, 15 + 18, 23 + 11, 31 + 4,
//           f_hi's from 7 + 29, 15 + 22, 23 + 15, 31 + 8.  The twelve stray partial products below bit 32 fall on twelve
//           distinct bits (11, 18, 19, 25, 26, 27 and 15, 22, 23, 29, 30, 31), so no carry reaches bit 32; the strays at
//           bit 40 and above are cut off with the byte.  Two v_mad_u64_u32, the second with the first's result as its
//           64-bit addend.
//   merge   byte 0 of the four high dwords side by side: two v_perm_b32 and an or (which the compiler fuses with the
//           span mask behind it into one v_bitop3_b32).
// nl_pair_gather returns the high dword of that value: the mask byte in bits 0..7, strays above.
// What hipcc had to be told: only the 64-bit add is asm -- the compiler proves by itself that no carry crosses bit 32
// and splits a C++ add into two v_add_u32.  The chained v_mad_u64_u32 and the v_bitop3_b32 it emits from plain C++.
// LANES = false is the same arithmetic in plain C++ (the host form): for thread 0's halo words, whose bytes are the
// same for the whole wave -- the compiler does them on the scalar unit, which asm with vector operands would forbid.
// -DMHX_NL_MUL32 keeps the form of before, one v_mul_lo_u32 per pair (flags_to_byte), for A/B builds (tools/build_variants.sh).
constexpr uint64_t kNlPattern64 = 0x0A0A0A0A0A0A0A0Aull, kLow7x8 = 0x7F7F7F7F7F7F7F7Full, kTop1x8 = 0x8080808080808080ull;
constexpr uint32_t kNlGatherLo = 0x02040810u, kNlGatherHi = 0x20408100u;
template <bool LANES = true> MHX_HD uint64_t nl_pair_flags(uint32_t v_lo, uint32_t v_hi)
{ // 0x80 in every byte of the pair that is '\n'
#if defined(__HIP_DEVICE_COMPILE__)
    if (LANES) {
        const uint32_t x_lo = __builtin_amdgcn_bitop3_b32(v_lo, 0x0A0A0A0Au, 0x7F7F7F7Fu, 0x28); // (a ^ b) & c
        const uint32_t x_hi = __builtin_amdgcn_bitop3_b32(v_hi, 0x0A0A0A0Au, 0x7F7F7F7Fu, 0x28);
        uint64_t t;
        asm("v_lshl_add_u64 %0, %1, 0, %2" : "=v"(t) : "v"(((uint64_t)x_hi << 32) | x_lo), "s"(kLow7x8));
        const uint32_t f_lo = __builtin_amdgcn_bitop3_b32((uint32_t)t, v_lo, 0x80808080u, 0x02); // ~(a | b) & c
        const uint32_t f_hi = __builtin_amdgcn_bitop3_b32((uint32_t)(t >> 32), v_hi, 0x80808080u, 0x02);
        return ((uint64_t)f_hi << 32) | f_lo;
    }
#endif
    const uint64_t v = ((uint64_t)v_hi << 32) | v_lo;
    const uint64_t t = ((v ^ kNlPattern64) & kLow7x8) + kLow7x8;
    return ~(t | v) & kTop1x8;
}
MHX_HD uint32_t nl_pair_gather(uint64_t f)
{
    const uint64_t g = (uint64_t)(uint32_t)f * kNlGatherLo + (uint64_t)(uint32_t)(f >> 32) * kNlGatherHi;
    return (uint32_t)(g >> 32);
}
template <bool LANES = true> MHX_HD uint32_t newline_mask(const uint32_t *p)
{
#ifdef MHX_NL_MUL32
    uint32_t n = 0;
#pragma unroll
    for (int d = 0; d < 8; d += 2)
        n |= flags_to_byte(byte_eq_flags(p[d], 0x0A0A0A0Au), byte_eq_flags(p[d + 1], 0x0A0A0A0Au)) << (4 * d);
    return n;
#else
    uint32_t h[4];
#pragma unroll
    for (int d = 0; d < 4; ++d) h[d] = nl_pair_gather(nl_pair_flags<LANES>(p[2 * d], p[2 * d + 1]));
#if defined(__HIP_DEVICE_COMPILE__)
    if (LANES) { // v_perm_b32 d, s0, s1, sel: selector 0..3 takes a byte of s1, 4..7 of s0, 0x0C is 0x00
        const uint32_t n01 = __builtin_amdgcn_perm(h[1], h[0], 0x0C0C0400u);
        const uint32_t n23 = __builtin_amdgcn_perm(h[3], h[2], 0x04000C0Cu);
        return n01 | n23;
    }
#endif
    return (h[0] & 0xFFu) | ((h[1] & 0xFFu) << 8) | ((h[2] & 0xFFu) << 16) | (h[3] << 24);
#endif
}
// A/C/G/T (either case) mask of the four bytes of a dword, as flags 0x80 per byte
MHX_HD uint32_t acgt_flags(uint32_t v)
{
    const uint32_t u = v & 0xDFDFDFDFu;
    return zero_byte_flags(perm_lut(kLutBase, base_index(u)) ^ u);
}

// bits of a 32-byte word starting at absolute offset A that lie inside [begin, end)
MHX_HD uint32_t inrange_mask(uint64_t A, uint64_t begin, uint64_t end)
{
    uint32_t m = 0xFFFFFFFFu;
    if (begin > A) { uint64_t lo = begin - A; m = lo >= 32 ? 0u : (m << lo); }
    if (end < A + 32) { uint64_t hi = end > A ? end - A : 0; m &= hi >= 32 ? 0xFFFFFFFFu : ((1u << hi) - 1u); }
    return m;
}

// Counts the records mash counts: those whose sequence line holds at least k bytes (feeds the
// "[N seqs]" comment of the .msh).  A sequence line starts right after the newline that ends a
// header; it is long enough iff none of its first k bytes is a newline and they all lie in the span.
struct LineLenCheck {
    const uint32_t *nlmap; // one newline bit per tile byte (+ the 64 halo bytes), span-masked
    uint64_t tile_off;     // absolute offset of tile byte 0
    uint64_t end;          // span end
    uint32_t k;
    uint32_t count;
};

// Bytes of lines whose index is 1 (mod 4), newline bytes excluded.  `line` is the line
// index at the first byte of the word.  Also verifies the 4-line layout: the line after a
// newline must start with '@' (index 0 mod 4) or '+' (index 2 mod 4).  tile_bytes/word_off
// locate the word inside the staged tile for that look-ahead (nullptr: skip the check).
MHX_HD uint32_t seqline_mask(uint32_t nl, uint32_t line, const uint8_t *tile_bytes, uint32_t word_off,
                             uint32_t check_limit, bool &bad_format, LineLenCheck *lc = nullptr)
{
    uint32_t m = 0, cur = 0xFFFFFFFFu, pend = 0;
    while (nl) {
        const uint32_t b = nl & (0u - nl);
        const uint32_t below = b - 1u;
        if ((line & 3u) == 1u) m |= cur & below;
        cur = ~(below | b);
        ++line;
        if (tile_bytes) {
            const uint32_t pos = word_off + (uint32_t)__builtin_ctz(b) + 1u;
            if (pos < check_limit) {
                const uint8_t c = tile_bytes[pos];
                if (((line & 3u) == 0u && c != '@') || ((line & 3u) == 2u && c != '+')) bad_format = true;
            }
            if (lc && (line & 3u) == 1u) pend |= b; // a sequence line starts behind this newline: measured below
        }
        nl &= nl - 1u;
    }
    // the length test of the sequence lines that start in this word, outside the per-newline loop (which
    // every lane of the wave sits through once per newline of the busiest lane)
    while (pend) {
        const uint32_t pos = word_off + (uint32_t)__builtin_ctz(pend) + 1u;
        const uint32_t wq = pos >> 5, sh = pos & 31u;
        const uint32_t window = funnel_bits(lc->nlmap[wq + 1], lc->nlmap[wq], sh); // newline bits of bytes pos..pos+31
        const uint32_t first_k = lc->k >= 32 ? 0xFFFFFFFFu : ((1u << lc->k) - 1u);
        if ((window & first_k) == 0 && lc->tile_off + pos + lc->k <= lc->end) {
            // a '\r' that ends the line is not part of the sequence (kseq drops it): if the k-th byte
            // is a CR followed by the newline (or by the end of the stream) the line has k-1 bases
            const uint32_t after = pos + lc->k;
            const bool ends_here = lc->tile_off + after >= lc->end || ((lc->nlmap[after >> 5] >> (after & 31u)) & 1u);
            if (!(tile_bytes[after - 1u] == '\r' && ends_here)) ++lc->count;
        }
        pend &= pend - 1u;
    }
    if ((line & 3u) == 1u) m |= cur;
    return m;
}

// bit p of the result is set iff bits p..p+K-1 of the window w[0..NWD] are all set (the
// last word is look-ahead only; NWD result words are returned).
// R_{2n} = R_n & (R_n >> n); R_{n+1} = R_n & (w >> n).
template <int K, int NWD> MHX_HD void run_starts(const uint32_t (&w)[NWD + 1], uint32_t (&out)[NWD])
{
    constexpr int N1 = NWD + 1;
    uint32_t cur[N1];
#pragma unroll
    for (int i = 0; i < N1; ++i) cur[i] = w[i];
    int len = 1;
    constexpr int top = K >= 32 ? 5 : K >= 16 ? 4 : K >= 8 ? 3 : K >= 4 ? 2 : K >= 2 ? 1 : 0;
#pragma unroll
    for (int b = top - 1; b >= 0; --b) {
        // double
        {
            uint32_t sh[N1];
#pragma unroll
            for (int i = 0; i < N1; ++i) {
                const uint32_t hi = (i + 1 < N1) ? cur[i + 1] : 0u;
                sh[i] = (uint32_t)(((((uint64_t)hi) << 32) | cur[i]) >> len);
            }
#pragma unroll
            for (int i = 0; i < N1; ++i) cur[i] &= sh[i];
            len *= 2;
        }
        if ((K >> b) & 1) {
            uint32_t sh[N1];
#pragma unroll
            for (int i = 0; i < N1; ++i) {
                const uint32_t hi = (i + 1 < N1) ? w[i + 1] : 0u;
                sh[i] = (uint32_t)(((((uint64_t)hi) << 32) | w[i]) >> len);
            }
#pragma unroll
            for (int i = 0; i < N1; ++i) cur[i] &= sh[i];
            len += 1;
        }
    }
#pragma unroll
    for (int i = 0; i < NWD; ++i) out[i] = cur[i];
}

// ---- MurmurHash3_x64_128, seed 42, first 8 output bytes (mash getHash) ----------------
// 64-bit values are handled so that hipcc keeps each step in its cheapest form on gfx950:
//  * a product is made opaque before it is rotated: left to itself the compiler turns rotl(k * c, r) into a SECOND
//    64x64 multiplication by (c << r) plus the shifted high word (10 instructions where 4 + 2 do);
//  * rotations and the fmix shift-xors are written on the 32-bit halves (2 v_alignbit / v_lshrrev + v_xor);
//  * h * 5 + c is v_lshl_add_u64 (5h, asm) and a 64-bit add: times5_plus.
MHX_HD uint64_t opaque64(uint64_t v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    asm("" : "+v"(v));
#endif
    return v;
}
MHX_HD uint64_t make64(uint32_t lo, uint32_t hi) { return ((uint64_t)hi << 32) | lo; }
template <int R> MHX_HD uint64_t rotl64(uint64_t x)
{
    static_assert(R > 0 && R < 64 && R != 32, "rotation amount");
    const uint32_t lo = (uint32_t)x, hi = (uint32_t)(x >> 32);
    if (R < 32) return make64(funnel_bits(lo, hi, 32 - R), funnel_bits(hi, lo, 32 - R));
    return make64(funnel_bits(hi, lo, 64 - R), funnel_bits(lo, hi, 64 - R));
}
MHX_HD uint64_t xorshift33(uint64_t k)
{ // k ^= k >> 33: only the low word changes
    const uint32_t lo = (uint32_t)k, hi = (uint32_t)(k >> 32);
    return make64(lo ^ (hi >> 1), hi);
}
// h * 5 + c.  The compiler's own best is three instructions (v_lshl_add_u32 for the high word, v_mad_u64_u32, and a 64-bit add
// of c); gfx950's v_lshl_add_u64 d, h, 2, h gives 5h in one, but no C++ spelling reaches it (h * 5 + c and (h << 2) + h + c both
// come out two instructions LONGER per window), so that one instruction is asm and the add of c is left to the compiler:
// two.  It pays only together with rotated() below.  Timed against the compiler's form at K = 21 and at K = 27 (m = 1 and 3):
// faster at each (profiles/canonical_select_ab.txt), so there is one device form for every K; the host path keeps plain C++.
MHX_HD uint64_t times5_plus(uint64_t h, uint32_t c)
{
#if defined(__HIP_DEVICE_COMPILE__)
    uint64_t r;
    asm("v_lshl_add_u64 %0, %1, 2, %1" : "=v"(r) : "v"(h));
    return r + c;
#else
    const uint32_t lo = (uint32_t)h, hi = (uint32_t)(h >> 32);
    const uint64_t t = (uint64_t)lo * 5u + c;
    return make64((uint32_t)t, ((hi << 2) + hi) + (uint32_t)(t >> 32));
#endif
}
// A rotation's result on its way into `+= h` and times5_plus.  make64's `hi << 32 | lo` is an addition to the compiler, which
// reassociates it with the `+= h` behind it: {lo, 0} + h + {0, hi}, a v_mov and two 64-bit adds where one add does -- unseen
// as long as times5_plus took the halves apart anyway, and exactly what ate the gain of the asm form there.  Opaque, the
// rotation's two v_alignbit write a register pair and the sum is one v_lshl_add_u64.
MHX_HD uint64_t rotated(uint64_t x) { return opaque64(x); }
// x * C mod 2^64 for a constant C.  hipcc's own sequence is v_mad_u64_u32 (lo * C_lo, 64 bits) + 2 x v_mul_lo_u32 (the cross
// terms) + v_add3_u32: four quarter-rate VALU instructions (4 cycles each per wave64 in isolation,
// profiles/r02_valu_class_rates_microbench.txt).  -DMHX_ASM_MUL64 selects an experiment of round 3 instead: three of them
// plus one full-rate add -- the cross sum lands in the ODD half of a register pair whose even half holds zero, and the
// last v_mad_u64_u32 takes that pair, (cross << 32), as its 64-bit addend.  The compiler cannot be talked into this by
// itself (it builds {0, cross} with two v_mov per multiply), so the four instructions are one asm block on the fixed pair
// v[70:71]; `zero` is the variable that lives in v70, threaded through every call of one hash.  A block of four with no
// hazard inside gets no s_nop brackets (round 2 wrapped single instructions and drowned in them).  Measured in the
// kernel (profiles/r03_hash_loop_asm_multiply_ab.txt): k=21 -0.3 %, k=27 +2.0 % -- no gain: 80 v_add3 became 80
// v_add_u32 per group of 8 windows, but 13 v_mov and 14 s_nop came with the fixed registers, and inside the kernel an
// instruction costs its ~3.5 issue cycles whatever its class.  The count is what matters, and four
// instructions per multiply is the floor: the 64-bit addend of v_mad_u64_u32 must be an even-aligned pair, and the value
// that has to go into its ODD half is produced in an even one.  The compiler's sequence stays the default.
template <uint64_t C> MHX_HD uint64_t mul64c(uint64_t x, uint32_t &zero)
{
#if defined(__HIP_DEVICE_COMPILE__) && defined(MHX_ASM_MUL64)
    const uint32_t lo = (uint32_t)x, hi = (uint32_t)(x >> 32);
    uint64_t p, carry;
    uint32_t y;
    asm("v_mul_lo_u32 v71, %[lo], %[chi]\n\t"
        "v_mul_lo_u32 %[y], %[hi], %[clo]\n\t"
        "v_add_u32_e32 v71, v71, %[y]\n\t"
        "v_mad_u64_u32 %[p], %[c], %[lo], %[clo], v[70:71]"
        : [p] "=&v"(p), [c] "=&s"(carry), [y] "=&v"(y), "+{v70}"(zero)
        : [lo] "v"(lo), [hi] "v"(hi), [clo] "s"((uint32_t)C), [chi] "s"((uint32_t)(C >> 32))
        : "v71");
    return p;
#else
    (void)zero;
    return opaque64(x * C);
#endif
}
// fmix64 without its last two steps, the multiplication by kFmixC2 and k ^= k >> 33 (see Murmur3Tail)
constexpr uint64_t kFmixC2 = 0xc4ceb9fe1a85ec53ull;
MHX_HD uint64_t fmix64_head(uint64_t k, uint32_t &zero)
{
    k = xorshift33(k);
    k = mul64c<0xff51afd7ed558ccdull>(k, zero);
    return xorshift33(k);
}
// The hash up to the last multiplication of its two fmix64: with a = ka * C2 and b = kb * C2 (C2 = kFmixC2, mod 2^64)
// the hash is h = xorshift33(a) + xorshift33(b).  Nearly every window is only tested against the threshold, h <= T,
// and that test needs neither product.  Multiplication distributes over addition mod 2^64: s = (ka + kb) * C2 = a + b, so
//   hi(s) = hi(a) + hi(b) + c1,  c1 = the carry of lo(a) + lo(b),
//   hi(h) = hi(a) + hi(b) + c2,  c2 = the carry of the two shift-xored low words (xorshift33 leaves the high words alone),
// and hi(h) is one of hi(s) - 1, hi(s), hi(s) + 1 (mod 2^32).  h <= T gives hi(h) <= hi(T), hence
//   (hi(s) + 1) mod 2^32 <= hi(T) + 2
// as long as the right side does not wrap; from hi(T) = 0xFFFFFFFD on the test says nothing and admission_limit
// saturates.  That is a necessary condition of h <= T for one 64-bit add, the high word of ONE multiplication, one add
// and one compare (5 instructions where the two whole products and an add of their high words took 9); it lets through
// (hi(T) + 3) / 2^32 of the windows where the exact test passes T / 2^64 of them.  Only those few do the two
// multiplications, the shift-xors and the 64-bit add (finish).  32-bit hashes (k <= 16) are tested by their exact low
// word, which needs both products whole: low32.
struct Murmur3Tail {
    uint64_t ka, kb;
    MHX_HD uint64_t finish() const
    {
        uint32_t zero = 0; // see mul64c
        return xorshift33(mul64c<kFmixC2>(ka, zero)) + xorshift33(mul64c<kFmixC2>(kb, zero));
    }
    MHX_HD uint32_t low32() const // 32-bit hashes (k <= 16)
    {
        uint32_t zero = 0;
        return (uint32_t)xorshift33(mul64c<kFmixC2>(ka, zero)) + (uint32_t)xorshift33(mul64c<kFmixC2>(kb, zero));
    }
    MHX_HD uint32_t high_bound() const { return (uint32_t)(((ka + kb) * kFmixC2) >> 32) + 1u; }
};
// largest value of Murmur3Tail::high_bound() a hash <= T can have
MHX_HD uint32_t admission_limit(uint64_t T)
{
    const uint32_t th = (uint32_t)(T >> 32);
    return th >= 0xFFFFFFFDu ? 0xFFFFFFFFu : th + 2u;
}
// h ^ k ^ K (the length K fits the low word).  h is made opaque before it is split: left to see that only the halves of
// h are used, the compiler takes the times5_plus in front apart as well and pays two v_mov per window for it.
template <int K> MHX_HD uint64_t xor_tail_len(uint64_t h, uint64_t k)
{
    h = opaque64(h);
    return make64(xor3((uint32_t)h, (uint32_t)k, (uint32_t)K), (uint32_t)(h >> 32) ^ (uint32_t)(k >> 32));
}
constexpr uint64_t kMurmurSeed = 42; // mash's hash seed
// Does the tail block's partial 8-byte word come out of a table (mhx_tail_lut.h)?  64-bit hashes whose partial word holds
// 1..5 bases: K = 17..21 (the partial k1) and K = 25..29 (the partial k2, behind a full k1).
template <int K> constexpr bool tail_lut_applies() { return K > 16 && (K & 7) >= 1 && (K & 7) <= 5; }
// The hot loop's choice: the table on the device, the multiplications on the host; -DMHX_NO_TAIL_LUT brings the
// multiplications back on the device too (the A/B of profiles/tail_lut_ab.txt).
template <int K> constexpr bool hot_tail_lut()
{
#if defined(__HIP_DEVICE_COMPILE__) && !defined(MHX_NO_TAIL_LUT)
    return tail_lut_applies<K>();
#else
    return false;
#endif
}
// K's table: as many bases as its partial word holds, the k2 form when that word is the tail block's second
template <int K> MHX_HD TailLutPtr tail_lut_of() { return tail_lut_table<K & 7, ((K & 15) > 8)>(); }
// w: the K bytes as little-endian dwords, bytes beyond K zero.
// LUT: the partial word's k from the table.  ONLY the sketch kernel's hot loop asks for it (process_group_regs): a window
// with a byte that is not A/C/G/T then hashes to the value of the letters its bytes alias to, and every such window is
// dropped behind the loop (mhx_tail_lut.h).  Everything that hashes a window for good keeps the multiplications.
// lut: tail_lut_of<K>(), fetched once by the caller for all the windows it hashes (LUT = false: unused).
// murmur3_blocks is the hash itself: with LUT it takes the partial word's k as the caller loaded it (k_lut) and reads
// only the full 8-byte words of w; murmur3_core forms the table index from w's partial word and loads.
template <int K, bool LUT> MHX_HD Murmur3Tail murmur3_blocks(const uint32_t (&w)[8], uint64_t k_lut)
{
    static_assert(!LUT || tail_lut_applies<K>(), "no table for this K");
    constexpr uint64_t c1 = kMurmurC1, c2 = kMurmurC2;
    constexpr int NBLK = K / 16, TAIL = K & 15;
    uint64_t h1 = kMurmurSeed, h2 = kMurmurSeed;
    uint32_t zero = 0; // see mul64c
#pragma unroll
    for (int b = 0; b < NBLK; ++b) {
        uint64_t k1 = make64(w[4 * b], w[4 * b + 1]);
        uint64_t k2 = make64(w[4 * b + 2], w[4 * b + 3]);
        k1 = rotl64<31>(mul64c<c1>(k1, zero)); k1 = mul64c<c2>(k1, zero); h1 ^= k1;
        h1 = rotated(rotl64<27>(h1));
        // block 0: h2 is still the seed, and (x + seed) * 5 + c = x * 5 + (c + 5 * seed) with a constant that fits 32 bits
        // still -- the 64-bit add of the seed (two instructions and a zero register per window) is folded away
        static_assert(0x52dce729ull + 5ull * kMurmurSeed <= 0xFFFFFFFFull, "folded constant of block 0 must fit times5_plus' 32-bit addend");
        if (b == 0) h1 = times5_plus(h1, (uint32_t)(0x52dce729ull + 5ull * kMurmurSeed));
        else { h1 += h2; h1 = times5_plus(h1, 0x52dce729u); }
        k2 = rotl64<33>(mul64c<c2>(k2, zero)); k2 = mul64c<c1>(k2, zero); h2 ^= k2;
        h2 = rotated(rotl64<31>(h2)); h2 += h1; h2 = times5_plus(h2, 0x38495ab5u);
    }
    // the tail block's xor and the xor of the length meet in the low word: h ^ k ^ K there is one three-input operation
    if (TAIL > 8) {
        uint64_t k2 = make64(w[(4 * NBLK + 2) & 7], w[(4 * NBLK + 3) & 7]);
        if constexpr (LUT) k2 = k_lut;
        else { k2 = rotl64<33>(mul64c<c2>(k2, zero)); k2 = mul64c<c1>(k2, zero); }
        h2 = xor_tail_len<K>(h2, k2);
    } else {
        h2 ^= (uint64_t)K;
    }
    if (TAIL > 0) {
        uint64_t k1 = make64(w[(4 * NBLK) & 7], w[(4 * NBLK + 1) & 7]);
        if constexpr (LUT && TAIL <= 8) k1 = k_lut;
        else { k1 = rotl64<31>(mul64c<c1>(k1, zero)); k1 = mul64c<c2>(k1, zero); }
        h1 = xor_tail_len<K>(h1, k1);
    } else {
        h1 ^= (uint64_t)K;
    }
    h1 += h2; h2 += h1;
    uint64_t ka = fmix64_head(h1, zero), kb = fmix64_head(h2, zero);
    // 64-bit hashes add the two (Murmur3Tail::high_bound).  The shift-xor's make64 is an addition to the compiler (see rotated()),
    // which reassociates it with that sum -- two v_mov and a second 64-bit add per window in the queue form; opaque, each
    // is a register pair and the sum one v_lshl_add_u64.  32-bit hashes never add them and keep the code they had.
    if (K > 16) { ka = opaque64(ka); kb = opaque64(kb); }
    return Murmur3Tail{ka, kb};
}
template <int K, bool LUT = false> MHX_HD Murmur3Tail murmur3_core(const uint32_t (&w)[8], TailLutPtr lut = nullptr)
{
    // the gather is issued first, as soon as the partial word's dwords exist, and consumed at the xor behind the blocks
    uint64_t k_lut = 0;
    if constexpr (LUT) k_lut = lut[tail_lut_index<K & 7>(w[(K / 8) * 2], w[((K / 8) * 2 + 1) & 7])];
    return murmur3_blocks<K, LUT>(w, k_lut);
}
template <int K> MHX_HD uint64_t murmur3_h1(const uint32_t (&w)[8]) { return murmur3_core<K>(w).finish(); }

// ---- phases -------------------------------------------------------------------------

// P1: stage the tile.  chunk c (16 B) of the tile is loaded by thread c % 256.
MHX_HD void phase_stage(TileSmem &sm, int tid, const uint8_t *base, uint64_t tile_off, uint64_t end)
{
    const uint64_t lim = (end + 15) & ~(uint64_t)15; // last readable 16-byte chunk boundary
    constexpr int kChunks = kTileBytes / 16;          // 1024
#ifndef MHX_STAGE_SERIAL
    // tile and halo inside the readable span (wave-uniform; every tile but the last): all loads of a lane are issued
    // before the first LDS write -- behind the per-chunk bound test below hipcc waits for each load (s_waitcnt vmcnt(0))
    // before it issues the next, four HBM round trips in a row at the head of every tile
    if (tile_off + (uint64_t)(kTileBytes + kHaloBytes) <= lim) {
        const uint4 *src = reinterpret_cast<const uint4 *>(base + tile_off) + tid;
        uint4 v[kChunks / kBlock], h = {0, 0, 0, 0};
#pragma unroll
        for (int j = 0; j < kChunks / kBlock; ++j) v[j] = src[j * kBlock];
        if (tid < kHaloBytes / 16) h = src[kChunks];
#pragma unroll
        for (int j = 0; j < kChunks / kBlock; ++j) sm.bytes[j * kBlock + tid] = v[j];
        if (tid < kHaloBytes / 16) sm.bytes[kChunks + tid] = h;
        return;
    }
#endif
#pragma unroll
    for (int j = 0; j < kChunks / kBlock; ++j) {
        const int c = j * kBlock + tid;
        const uint64_t off = tile_off + (uint64_t)c * 16;
        uint4 v = {0, 0, 0, 0};
        if (off < lim) v = *reinterpret_cast<const uint4 *>(base + off);
        sm.bytes[c] = v;
    }
    if (tid < kHaloBytes / 16) {
        const int c = kChunks + tid;
        const uint64_t off = tile_off + (uint64_t)c * 16;
        uint4 v = {0, 0, 0, 0};
        if (off < lim) v = *reinterpret_cast<const uint4 *>(base + off);
        sm.bytes[c] = v;
    }
}

// P2a: newline mask of this thread's 128 bytes (and, for thread 0, of the halo).  `interior`: the tile and its
// halo lie inside the span, so no byte has to be masked out (wave-uniform: all tiles but the first and the last)
MHX_HD void phase_classify(TileSmem &sm, int tid, ThreadState &st, uint64_t tile_off, uint64_t begin, uint64_t end, bool interior)
{
    const uint32_t *p = reinterpret_cast<const uint32_t *>(sm.bytes) + tid * (kBytesPerThread / 4);
    uint32_t total = 0;
#pragma unroll
    for (int w = 0; w < kWordsPerThread; ++w) {
        st.in[w] = interior ? 0xFFFFFFFFu : inrange_mask(tile_off + (uint64_t)tid * kBytesPerThread + 32u * w, begin, end);
        st.nl[w] = newline_mask(p + 8 * w) & st.in[w];
        total += (uint32_t)__builtin_popcount(st.nl[w]);
        tile_nlmap(sm)[tid * kWordsPerThread + w] = st.nl[w];
    }
    st.nlcount = total;
    if (tid == 0) {
        const uint32_t *h = reinterpret_cast<const uint32_t *>(sm.bytes) + kTileBytes / 4;
#pragma unroll
        for (int w = 0; w < 2; ++w) {
            st.hin[w] = interior ? 0xFFFFFFFFu : inrange_mask(tile_off + kTileBytes + 32u * w, begin, end);
            // one lane's bytes: told so, the compiler does the word on the scalar unit in every kernel form (left to itself it
            // did in the FASTQ forms and kept 90 VALU instructions for the two words in the others)
            uint32_t hw[8];
#pragma unroll
            for (int d = 0; d < 8; ++d) hw[d] = wave_uniform(h[8 * w + d]);
            st.hnl[w] = newline_mask<false>(hw) & st.hin[w];
            tile_nlmap(sm)[kTileBytes / 32 + w] = st.hnl[w];
        }
    }
}


// FASTQ line phase of a tile WITHOUT its predecessors: the line index (mod 4) of the tile's first byte, or 4 if the tile
// cannot tell.  A header is the only line that starts with '@', is followed by a line that does not, and then by a line
// that starts with '+' (a quality line may start with '@', but the line after it is a header and starts with '@' too), so
// the first such triple among the tile's first six line starts fixes the phase: with i newlines in front of the header
// line the tile's first byte lies in line -i (mod 4).  Needs six newlines within the staged, in-span bytes -- reads of up
// to ~2.7 kb; tiles of longer lines take the look-back pass instead.  The per-record layout check of phase_good still
// runs over every line, so a phase derived from a malformed file is caught there.
MHX_HD uint32_t phase_selfsync(TileSmem &sm, uint32_t check_limit)
{
    const uint32_t *nlmap = tile_nlmap(sm);
    const uint8_t *b = reinterpret_cast<const uint8_t *>(sm.bytes);
    uint32_t pos[6];
    int n = 0;
    for (int w = 0; w < kTileBytes / 32 + 2 && n < 6; ++w) {
        uint32_t m = nlmap[w];
        while (m && n < 6) {
            pos[n++] = 32u * (uint32_t)w + (uint32_t)__builtin_ctz(m);
            m &= m - 1u;
        }
    }
    for (int i = 0; i + 2 < n && i < 4; ++i) {
        const uint32_t p0 = pos[i] + 1u, p1 = pos[i + 1] + 1u, p2 = pos[i + 2] + 1u;
        if (p2 >= check_limit) break;
        if (b[p0] == '@' && b[p1] != '@' && b[p1] != '+' && b[p2] == '+') return (4u - ((uint32_t)(i + 1) & 3u)) & 3u;
    }
    return 4u;
}

// What a tile leaves behind for the chain check: the line phase of its first byte and of the first byte of the next
// tile.  phase_verify_kernel compares neighbours, so that the phases the tiles found by themselves are the ones a
// running line count from the start of the span gives -- a file on which they are not (a record cut short in front of
// a tile border, which kseq reads as a record without qualities) is flagged and goes to the general parser.
constexpr uint8_t kPhaseKnown = 0x10;
MHX_HD uint8_t phase_record(uint32_t start_phase, uint32_t tile_lines)
{
    return (uint8_t)(kPhaseKnown | (start_phase & 3u) | (((start_phase + tile_lines) & 3u) << 2));
}
MHX_HD bool phase_chain_broken(uint8_t prev, uint8_t cur)
{
    return (prev & kPhaseKnown) && (cur & kPhaseKnown) && ((prev >> 2) & 3u) != (cur & 3u);
}

// P2c: bytes a k-mer may cover -> good map: FASTQ: the bytes of sequence lines; sequence stream: everything but the
// record separators.  (Whether they are A/C/G/T is checked for the few windows that pass the threshold.)
// returns the number of records of this thread's bytes whose sequence line holds >= k bytes
template <bool FASTQ>
MHX_HD uint32_t phase_good(TileSmem &sm, int tid, const ThreadState &st, uint32_t line_base, uint32_t excl,
                           uint32_t tile_total, uint32_t check_limit, bool &bad_format, uint64_t tile_off, uint64_t end, uint32_t k)
{
    const uint8_t *tb = reinterpret_cast<const uint8_t *>(sm.bytes);
    LineLenCheck lc{tile_nlmap(sm), tile_off, end, k, 0u};
    uint32_t line = line_base + excl;
#pragma unroll
    for (int w = 0; w < kWordsPerThread; ++w) {
        uint32_t g;
        if (FASTQ) {
            g = st.in[w] & seqline_mask(st.nl[w], line, tb, (uint32_t)tid * kBytesPerThread + 32u * w, check_limit, bad_format, &lc);
            line += (uint32_t)__builtin_popcount(st.nl[w]);
        } else {
            g = st.in[w] & ~st.nl[w];
        }
        tile_good(sm)[tid * kWordsPerThread + w] = g;
    }
    if (tid == 0) {
        uint32_t hl = line_base + tile_total;
#pragma unroll
        for (int w = 0; w < 2; ++w) {
            uint32_t g;
            if (FASTQ) {
                bool ignore = false;
                g = st.hin[w] & seqline_mask(st.hnl[w], hl, nullptr, 0, 0, ignore);
                hl += (uint32_t)__builtin_popcount(st.hnl[w]);
            } else {
                g = st.hin[w] & ~st.hnl[w];
            }
            tile_good(sm)[kTileBytes / 32 + w] = g;
        }
        tile_good(sm)[kTileBytes / 32 + 2] = 0;
        tile_good(sm)[kTileBytes / 32 + 3] = 0;
    }
    return lc.count;
}

// ---- P2c for FASTQ without a trip per newline -------------------------------------------
// seqline_mask walks the newlines of a word one by one, and a wave sits through as many trips as its busiest lane
// needs: the '+' line puts two newlines two bytes apart, so on ordinary reads EVERY wave takes two trips per word (and
// one more of the length loop), each with an LDS round trip inside.  The form below gives the same good map, bad-format
// flag and record count (tests/emul/tile_parse_emul.cpp compares them tile by tile) in two loop-free parts:
//   mask    the line index of byte i is line + popcount(nl below i): its two low bits are prefix parities of the
//           newline mask, pure register arithmetic (seqline_mask_bits);
//   checks  the newlines of the tile are listed by position (phase_events; sm.valid is free until phase_runs), and
//           after the barrier lane e takes newline e: the line that starts behind it has index line_base + e + 1, which
//           says what to test there ('@', '+', or the length of a sequence line) -- one lane per line instead of one
//           loop trip per line.
// The list holds kEventCap positions; a tile with more newlines (lines of under 16 bytes on average) keeps phase_good.
constexpr uint32_t kEventCap = kGroupsPerTile / 2; // 16-bit entries of sm.valid: one per 16 tile bytes
static_assert(kEventCap * 2 == sizeof(TileSmem::valid) && kEventCap % kBlock == 0, "event list = sm.valid");
static_assert(kTileBytes + kHaloBytes <= 65536, "event positions are 16-bit");
MHX_HD bool parse_events_fit(uint32_t tile_total) { return tile_total <= kEventCap; }

// bit i = parity of the bits of x below i
MHX_HD uint32_t prefix_parity_excl(uint32_t x)
{
    x ^= x << 1; x ^= x << 2; x ^= x << 4; x ^= x << 8; x ^= x << 16;
    return x << 1;
}
// seqline_mask's result (bytes of lines with index 1 mod 4, newlines excluded) by bit arithmetic
MHX_HD uint32_t seqline_mask_bits(uint32_t nl, uint32_t line)
{
    const uint32_t b0 = prefix_parity_excl(nl) ^ (0u - (line & 1u));               // low bit of every byte's line index
    const uint32_t b1 = prefix_parity_excl(nl & b0) ^ (0u - ((line >> 1) & 1u));   // second bit: flips where the low bit carries
    return b0 & ~b1 & ~nl;
}

// tile positions of this thread's newlines -> events[excl ..) (16-bit entries in sm.valid).  Two per word without a
// loop -- ordinary reads never have more in 32 bytes --, the rest in a loop no wave of such a file enters.
// Needs parse_events_fit(tile_total): excl + rank < tile_total <= kEventCap.
MHX_HD void phase_events(TileSmem &sm, int tid, const ThreadState &st, uint32_t excl)
{
    uint16_t *ev = reinterpret_cast<uint16_t *>(sm.valid);
    uint32_t at = excl;
#pragma unroll
    for (int w = 0; w < kWordsPerThread; ++w) {
        const uint32_t off = (uint32_t)tid * kBytesPerThread + 32u * w;
        uint32_t nl = st.nl[w];
        if (nl) {
            ev[at] = (uint16_t)(off + (uint32_t)__builtin_ctz(nl));
            nl &= nl - 1u;
            if (nl) {
                ev[at + 1u] = (uint16_t)(off + (uint32_t)__builtin_ctz(nl));
                nl &= nl - 1u;
                for (uint32_t j = 2; MHX_UNLIKELY(nl != 0); ++j, nl &= nl - 1u) ev[at + j] = (uint16_t)(off + (uint32_t)__builtin_ctz(nl));
            }
        }
        at += (uint32_t)__builtin_popcount(st.nl[w]);
    }
}

// ---- phase_selfsync from the newline list ------------------------------------------------------------------------------
// phase_selfsync walks the newline map word by word on one lane, on the way to the barrier all four waves wait at.  Where
// phase_events has listed the tile's newlines, its first six positions are the first six entries of the list, and the
// four triples are tested side by side: lane i (0..3) takes the entries i, i + 1, i + 2 (selfsync_triple), the lowest
// lane that passes gives the phase (selfsync_phase of the four-bit ballot).  The same answer as phase_selfsync on the same
// bytes: the positions rise with i, so `p2 >= check_limit` at one i holds at every later one -- the search's `break` and a
// failed test on that lane and all above it are one thing.
// Taken where the first wave's own newline count (sm.cnt[0] behind block_scan_excl) is kSelfsyncNewlines at least: entries
// 0..5 then come from lanes of the first wave, whose LDS operations complete in order, so that wave reads them behind
// phase_events without a barrier (as the line path reads what its lane 0 stores).  Every other tile keeps the search.
// -DMHX_SELFSYNC_MAP: no tile takes the list, the A/B builds of tools/build_variants.sh.
constexpr uint32_t kSelfsyncNewlines = 6, kSelfsyncTriples = 4;
#ifdef MHX_SELFSYNC_MAP
constexpr bool kSelfsyncList = false;
#else
constexpr bool kSelfsyncList = true;
#endif
// workgroup-uniform part of the choice; wave0_newlines: the newlines of the tile's first kBlock / 4 threads
MHX_HD bool selfsync_from_list(bool fast_parse, bool first_tile_of_span, uint32_t wave0_newlines)
{
    return kSelfsyncList && fast_parse && !first_tile_of_span && wave0_newlines >= kSelfsyncNewlines;
}
MHX_HD bool selfsync_triple(const TileSmem &sm, uint32_t i, uint32_t check_limit)
{ // i < kSelfsyncTriples; needs entries i .. i + 2 of the list
    const uint16_t *ev = reinterpret_cast<const uint16_t *>(sm.valid);
    const uint8_t *b = reinterpret_cast<const uint8_t *>(sm.bytes);
    // the three entries, then the three bytes, then one verdict without a branch: two LDS round trips, not one per test
    // (p2 <= kTileBytes is staged whatever check_limit says; a byte beyond the limit is read and not used)
    const uint32_t p0 = (uint32_t)ev[i] + 1u, p1 = (uint32_t)ev[i + 1u] + 1u, p2 = (uint32_t)ev[i + 2u] + 1u;
    const uint32_t c0 = b[p0], c1 = b[p1], c2 = b[p2];
    return (p2 < check_limit) & (c0 == '@') & (c1 != '@') & (c1 != '+') & (c2 == '+');
}
MHX_HD uint32_t selfsync_phase(uint32_t passing)
{ // bit i: triple i passes
    passing &= (1u << kSelfsyncTriples) - 1u;
    if (!passing) return 4u;
    return (4u - (((uint32_t)__builtin_ctz(passing) + 1u) & 3u)) & 3u;
}
// The tiles the four lanes cannot take -- under six newlines in the first wave's bytes -- are the ones on which the search
// of the map is slow: it reads the map word by word, one LDS round trip each, up to the sixth newline, and through all 514
// words where the tile has fewer (reads of 10 kb: every tile, in both launches; some 25 us a tile, more than its hash loop).
// The list holds the same positions in order; behind ONE more barrier, which completes it, thread 0 takes the first six
// from it and, where the tile has fewer, goes on in the two halo words it has in registers (the map holds them, the
// list does not).  phase_selfsync's answer on the same bytes, position for position.  Needs parse_events_fit(tile_total).
MHX_HD uint32_t phase_selfsync_list(const TileSmem &sm, const ThreadState &st0, uint32_t tile_total, uint32_t check_limit)
{
    const uint16_t *ev = reinterpret_cast<const uint16_t *>(sm.valid);
    const uint8_t *b = reinterpret_cast<const uint8_t *>(sm.bytes);
    // both loops unrolled, every index of pos a constant: an array indexed at run time would live in scratch memory
    uint64_t halo = make64(st0.hnl[0], st0.hnl[1]);
    uint32_t pos[6], n = 0;
#pragma unroll
    for (uint32_t j = 0; j < 6; ++j) {
        pos[j] = 0;
        if (j < tile_total) {
            pos[j] = ev[j];
            n = j + 1u;
        } else if (halo) {
            pos[j] = (uint32_t)kTileBytes + (uint32_t)__builtin_ctzll(halo);
            halo &= halo - 1u;
            n = j + 1u;
        }
    }
#pragma unroll
    for (uint32_t i = 0; i < 4; ++i) {
        if (i + 2u >= n) break;
        const uint32_t p0 = pos[i] + 1u, p1 = pos[i + 1] + 1u, p2 = pos[i + 2] + 1u;
        if (p2 >= check_limit) break;
        if (b[p0] == '@' && b[p1] != '@' && b[p1] != '+' && b[p2] == '+') return (4u - ((i + 1u) & 3u)) & 3u;
    }
    return 4u;
}

// LineLenCheck's test for the sequence line that starts at tile position pos: does the record count?
MHX_HD bool seqline_is_long(const uint32_t *nlmap, const uint8_t *tile_bytes, uint32_t pos, uint64_t tile_off, uint64_t end, uint32_t k)
{
    const uint32_t wq = pos >> 5, sh = pos & 31u;
    const uint32_t window = funnel_bits(nlmap[wq + 1], nlmap[wq], sh); // newline bits of bytes pos..pos+31
    const uint32_t first_k = k >= 32 ? 0xFFFFFFFFu : ((1u << k) - 1u);
    if ((window & first_k) != 0 || tile_off + pos + k > end) return false;
    // the CR rule of seqline_mask: a '\r' in front of the line end is not a base
    const uint32_t after = pos + k;
    const bool ends_here = tile_off + after >= end || ((nlmap[after >> 5] >> (after & 31u)) & 1u);
    return !(tile_bytes[after - 1u] == '\r' && ends_here);
}

// phase_good<true> for a tile whose newlines phase_events has listed (a barrier in between), in its two halves: the
// good map (phase_good_events_map) and the checks, one lane per newline (phase_event_checks); the sum of the checks'
// return values over the workgroup is the tile's number of long records (which lane counts a record differs from
// phase_good).  The line-item form below skips the map and keeps the '@' / '+' checks (phase_event_checks<false>); its
// long records are counted from the ends of the lines (line_span_long_record).
MHX_HD void phase_good_events_map(TileSmem &sm, int tid, const ThreadState &st, uint32_t line_base, uint32_t excl, uint32_t tile_total)
{
    uint32_t line = line_base + excl;
#pragma unroll
    for (int w = 0; w < kWordsPerThread; ++w) {
        tile_good(sm)[tid * kWordsPerThread + w] = st.in[w] & seqline_mask_bits(st.nl[w], line);
        line += (uint32_t)__builtin_popcount(st.nl[w]);
    }
    if (tid == 0) {
        uint32_t hl = line_base + tile_total;
#pragma unroll
        for (int w = 0; w < 2; ++w) {
            tile_good(sm)[kTileBytes / 32 + w] = st.hin[w] & seqline_mask_bits(st.hnl[w], hl);
            hl += (uint32_t)__builtin_popcount(st.hnl[w]);
        }
        tile_good(sm)[kTileBytes / 32 + 2] = 0;
        tile_good(sm)[kTileBytes / 32 + 3] = 0;
    }
}
// SEQ_LEN = false: the '@' / '+' tests alone, for the line path, which counts the long records from the ends of the lines
// it reads anyway (phase_line_span); the return value is 0 then.  A form of its own, not a run-time switch.
template <bool SEQ_LEN = true>
MHX_HD uint32_t phase_event_checks(TileSmem &sm, int tid, uint32_t line_base, uint32_t tile_total, uint32_t check_limit,
                                   bool &bad_format, uint64_t tile_off, uint64_t end, uint32_t k)
{
    const uint8_t *tb = reinterpret_cast<const uint8_t *>(sm.bytes);
    const uint16_t *ev = reinterpret_cast<const uint16_t *>(sm.valid);
    uint32_t count = 0;
#pragma unroll
    for (uint32_t r = 0; r < kEventCap / kBlock; ++r) { // unrolled; ordinary reads (lines of 64 bytes and more) need the first round only
        if (r == 1 && tile_total <= (uint32_t)kBlock) break; // workgroup-uniform
        const uint32_t e = r * kBlock + (uint32_t)tid;
        if (e < tile_total) {
            const uint32_t pos = (uint32_t)ev[e] + 1u;     // first byte of the line behind newline e (<= kTileBytes: staged)
            const uint32_t idx = (line_base + e + 1u) & 3u; // that line's index
            if (SEQ_LEN && idx == 1u) {
                if (seqline_is_long(tile_nlmap(sm), tb, pos, tile_off, end, k)) ++count;
            } else if ((SEQ_LEN ? idx != 3u : !(idx & 1u)) && pos < check_limit) {
                if (tb[pos] != (idx == 0u ? '@' : '+')) bad_format = true;
            }
        }
    }
    return count;
}
MHX_HD uint32_t phase_good_events(TileSmem &sm, int tid, const ThreadState &st, uint32_t line_base, uint32_t excl,
                                  uint32_t tile_total, uint32_t check_limit, bool &bad_format, uint64_t tile_off, uint64_t end, uint32_t k)
{
    phase_good_events_map(sm, tid, st, line_base, excl, tile_total);
    return phase_event_checks(sm, tid, line_base, tile_total, check_limit, bad_format, tile_off, end, k);
}

// ---- FASTQ work list from the line list, not from byte maps ------------------------------------------------------------
// For an interior FASTQ tile whose newlines phase_events has listed, the work list and the start masks follow from the lines
// themselves (DESIGN.md 3.1 has the reasoning, the bounds and the measurements).  With n_0 < .. < n_{t-1} the tile's newlines
// (t = tile_total) and h the first newline of the halo (none: beyond it), line i (0 <= i <= t) spans [a_i, b_i): a_0 = 0,
// a_i = n_{i-1} + 1; b_i = n_i, b_t = h; its index is line_base + i.  For every line with index 1 (mod 4),
// pmax = min(b_i - K, kTileBytes - 1); if pmax >= a_i
//     the valid starts are a_i .. pmax, the items the groups a_i >> 3 .. pmax >> 3,
//     bit j of group g's byte in sm.valid is set iff a_i <= 8 g + j <= pmax, and the tile has pmax - a_i + 1 k-mers more
// (a CR in front of the newline is a line byte, as in seqline_mask): bit for bit what the maps give, in another order of sm.list.
// Invariants: for K >= 8 two sequence lines never share a group (one writer per mask byte); a lane reads its line's two ends
// (phase_line_span) BEFORE the barrier behind which the list and the masks are written over the events and the newline map
// (phase_line_items).  One lane per sequence line, all in the first wave.  Taken where the tile is interior, its newlines are
// listed, it holds kLineItemMinNewlines newlines at least and kLineItemLines sequence lines at most, and no sequence line has
// more than kLineItemGroups groups; a lane that finds its line too long sends the whole workgroup back to the maps.
constexpr uint32_t kLineItemLines = 64;
constexpr uint32_t kLineItemGroups = 40;
// Tiles with fewer newlines do not try: records whose lines are as long as 40 groups allow (320 + K - 1 bytes) put 48 into a
// tile, so reads of 600 to 2700 bases, which self-synchronise, are spared the attempt and its extra barrier on every tile.
constexpr uint32_t kLineItemMinNewlines = 48;
static_assert(kLineItemLines <= 64, "the sequence lines of a tile take the lanes of one wave");
// which K have the form at all (-DMHX_PARSE_MAPS: none, the A/B builds of tools/build_variants.sh)
template <int K> constexpr bool line_items_apply()
{
#ifdef MHX_PARSE_MAPS
    return false;
#else
    return K >= 8;
#endif
}
// ... and which kernel forms of such a K (fmt, queue: sketch_tile_kernel's FMT and QUEUE), as pair_words_form has it:
//   a form takes the path only where it stays at 22 720 B of LDS, 72 VGPRs, no scratch and seven waves per SIMD: the queue
//       forms of K = 29 stand at 72 VGPRs and take 16 bytes of scratch with it, they keep the maps;
//   the look-back kernels (FMT 1) keep the maps: with the path compiled into them a FASTQ of 10 kb reads, all of whose tiles
//       they hash (on the map path), ran 4 % slower than the parent in every round, and level with it without
//       (profiles/line_items_ab.txt, section 4).  In a real run they work on tiles of under six newlines, which never qualify.
template <int K> constexpr bool line_items_form(int fmt, bool queue) { return line_items_apply<K>() && fmt == 2 && !(K == 29 && queue); }
MHX_HD uint32_t seqline_first(uint32_t line_base) { return (1u - line_base) & 3u; } // i of the tile's first sequence line
MHX_HD uint32_t seqline_count(uint32_t line_base, uint32_t tile_total)
{
    const uint32_t i0 = seqline_first(line_base);
    return i0 <= tile_total ? (tile_total - i0) / 4u + 1u : 0u;
}
// the workgroup-uniform part of the choice
MHX_HD bool line_items_try(bool fast_parse, bool interior, uint32_t line_base, uint32_t tile_total)
{
    return fast_parse && interior && tile_total >= kLineItemMinNewlines && seqline_count(line_base, tile_total) <= kLineItemLines;
}
// ngroups = 0: no valid start; long_record: 1 iff the line starts in this tile and its record counts (seqline_is_long)
struct LineSpan { uint32_t a, pmax, ngroups, kmers, long_record; };
// The record count of the line path.  phase_event_checks<true> gives the newline in front of every sequence line a lane,
// which looks the line's first K bytes up in the newline map (seqline_is_long: 19 instructions and three LDS reads that all
// four waves sit through).  On an interior tile the two ends [a, b) phase_line_span holds say the same:
//     no newline among the first K bytes, all of them in the span    <=>  b - a >= K   (b is the next newline, or the end of
//                                                                         the halo, which lies in the span and beyond a + K)
//     the CR rule: the K-th byte is a '\r' and the line ends there   <=>  bytes[a + K - 1] == '\r' && b == a + K
// and the checks count a line in the tile that holds the newline in front of it, so line i = 0 is not counted here (the
// tile in front has it; in the tile that starts the span line 0 is a header) while line i = tile_total, which starts at
// kTileBytes at the latest and has no k-mer start of this tile, is.
// INVARIANT: a record is counted once, by the lane of its line, in front of the line-phase barrier, and by nothing else on
// this path -- the checks run as phase_event_checks<false> there.  The count does not depend on the length bound of
// phase_line_items, so a tile that falls back to the maps behind the barrier (sm.misc[6]) has its records counted already
// and phase_good_events_map, which it then runs, counts nothing.
template <int K> MHX_HD uint32_t line_span_long_record(const uint8_t *tile_bytes, uint32_t i, uint32_t a, uint32_t b)
{
    if (i == 0u || b - a < (uint32_t)K) return 0u; // b >= a: a line's end is not in front of its start
    return (b == a + (uint32_t)K && tile_bytes[a + (uint32_t)K - 1u] == '\r') ? 0u : 1u;
}
// the tile's j-th sequence line, from its two events (or the halo words of the newline map): before the barrier behind
// which phase_line_items writes over both
template <int K> MHX_HD LineSpan phase_line_span(const TileSmem &sm, uint32_t j, uint32_t line_base, uint32_t tile_total)
{
    const uint16_t *ev = reinterpret_cast<const uint16_t *>(sm.valid);
    const uint32_t i = seqline_first(line_base) + 4u * j;
    LineSpan s{0u, 0u, 0u, 0u, 0u};
    if (i > tile_total) return s;
    const uint32_t a = i ? (uint32_t)ev[i - 1u] + 1u : 0u;
    uint32_t b;
    if (i < tile_total) {
        b = ev[i];
    } else { // the line that runs into the halo
        const uint32_t h0 = sm.maps[kTileBytes / 32], h1 = sm.maps[kTileBytes / 32 + 1];
        b = h0 ? (uint32_t)kTileBytes + (uint32_t)__builtin_ctz(h0) : h1 ? (uint32_t)kTileBytes + 32u + (uint32_t)__builtin_ctz(h1) : (uint32_t)(kTileBytes + kHaloBytes);
    }
    s.long_record = line_span_long_record<K>(reinterpret_cast<const uint8_t *>(sm.bytes), i, a, b);
    int32_t pmax = (int32_t)b - K;
    if (pmax > kTileBytes - 1) pmax = kTileBytes - 1;
    if (pmax < (int32_t)a) return s;
    s.a = a;
    s.pmax = (uint32_t)pmax;
    s.ngroups = ((uint32_t)pmax >> 3) - (a >> 3) + 1u;
    s.kmers = (uint32_t)pmax - a + 1u;
    return s;
}
MHX_HD bool line_span_too_long(const LineSpan &s) { return s.ngroups > kLineItemGroups; }
// the line's groups -> sm.list[at .. at + ngroups), their start masks -> sm.valid
MHX_HD void phase_line_items(TileSmem &sm, const LineSpan &s, uint32_t at)
{
    if (!s.ngroups) return;
    uint8_t *vb = reinterpret_cast<uint8_t *>(sm.valid);
    const uint32_t g0 = s.a >> 3, g1 = s.pmax >> 3;
    const uint32_t first = (0xFFu << (s.a & 7u)) & 0xFFu, last = 0xFFu >> (7u - (s.pmax & 7u));
    sm.list[at] = (uint16_t)g0;
    vb[g0] = (uint8_t)(g0 == g1 ? first & last : first);
    if (g0 == g1) return;
    // every further group whole, and the last one's mask over it afterwards (same lane, same byte: LDS keeps the order)
    for (uint32_t g = g0 + 1u; g <= g1; ++g) {
        sm.list[++at] = (uint16_t)g;
        vb[g] = 0xFFu;
    }
    vb[g1] = (uint8_t)last;
}

// ---- line-relative items: the groups of a sequence line counted from its first valid start ------------------------------
// phase_line_items lists the tile-aligned groups a line's starts a .. pmax touch: (n + 7) / 8 of them on average for n starts
// at a random offset, the first and the last with about seven dead windows between them, all of which the hash loop runs.
// Grouped from a instead, the line has n >> 3 FULL items at the byte positions a, a + 8, .. with eight valid windows each and,
// if c = n & 7 is not 0, one TAIL item at a + 8 (n >> 3) with its first c windows valid.  An entry of sm.list is the item's
// byte position (14 bits; no multiple of 4 any more: line_rel_source) with kLineRelFull set for a full item, which has no
// mask byte; a tail's mask (1 << c) - 1 is byte position >> 3 of sm.valid (for K >= 8 two sequence lines never share a group
// and the positions of one line lie in it, so one writer per byte as before).  All full items of the tile stand in front of
// all its tails, so a wave's trip of 64 consecutive entries is made of full items, or of tails alone, but for the one trip
// that holds the boundary: the kernel runs a trip that begins among the full items on its hot body and a trip that begins
// among the tails on one that stops behind the longest tail of the trip (process_group_regs, TAIL).
// (Telling full from tail by the entry's index instead of a flag, with the trip's first index carried on the scalar unit and
// the masks looked at only in the trip that holds the boundary, is 631 VALU a trip where this is 635 -- and takes the inline
// kernels of K = 21 to 36 bytes of scratch in each of three spellings tried: profiles/line_rel_items_ab.txt, section 1.)
// All offsets of a lane come from ONE sum: line_rel_counts packs three counts of the line into a word -- its full items (13
// bits: at most 2048 in a tile), its tail (7 bits: at most 64) and how many aligned groups it touches beyond those, 0 or 1 (7
// bits) -- the kernel's one LDS atomic adds the words up (a wave scan, as it was for the groups), and what it returns and leaves
// behind are the packed offsets and the packed totals: of the new items, and, as their sum, of the aligned list.
// Never more entries than the aligned list: (n >> 3) + (c != 0) <= the groups a .. pmax touch.  The bounds that select the
// path (line_items_try, line_span_too_long: on the ALIGNED group count, which the span holds anyway) are the same.
// THE CHOICE PER TILE (line_rel_choose, workgroup-uniform behind the barrier, from the totals): trips are whole, and a trip of
// the new hot body is a few instructions longer than one over aligned items and carries two replayed reads, so the new items
// pay only where they save a trip of the hot body: where the full items alone fill fewer trips of 64 than the aligned groups,
// ceil(full / 64) < ceil(aligned / 64).  The tails then ride in the rest of the last trip or take a short one.  A tile that does
// not save one -- 148-base reads at K = 21: 128 starts a line, 843 full items, no tails, 14 trips either way -- lists its
// aligned groups (phase_line_items, at the offset line_rel_aligned of the same packed prefix) and runs the loop it ran before.
constexpr uint32_t kLineRelFull = 0x8000u, kLineRelPos = 0x3FFFu;
static_assert(kTileBytes - 1 <= (int)kLineRelPos, "an item's byte position fits under the flag");
// which kernel forms of the line path take the items this way (-DMHX_LINE_ITEMS_ALIGNED: none, the A/B builds; the emulator
// of tests/emul/line_rel_items_emul.cpp runs both item forms in one build), by the rule of line_items_form: 22 720 B of LDS, <= 72 VGPRs, no scratch, seven waves.
// With the two further loop bodies in them the inline forms of K = 18, 23, 28, 30, 31 and 32 (the plain and the split kernel:
// 8 to 36 bytes) and the queue forms of K = 26 (16 bytes) took scratch at 72 VGPRs in one of the two builds counted: they keep
// the aligned items and are the kernels they were (profiles/line_rel_items_ab.txt, section 1).
template <int K> constexpr bool line_rel_form(int fmt, bool queue)
{
#ifdef MHX_LINE_ITEMS_ALIGNED
    return false;
#else
    return line_items_form<K>(fmt, queue) && !(queue ? K == 26 : K == 18 || K == 23 || K == 28 || K >= 30);
#endif
}
MHX_HD uint32_t line_rel_counts(const LineSpan &s)
{
    const uint32_t full = s.kmers >> 3, tail = (s.kmers & 7u) ? 1u : 0u;
    return full | (tail << 13) | ((s.ngroups - full - tail) << 20); // ngroups is ceil(kmers / 8) or one more
}
MHX_HD uint32_t line_rel_full(uint32_t packed) { return packed & 0x1FFFu; }
MHX_HD uint32_t line_rel_tails(uint32_t packed) { return (packed >> 13) & 0x7Fu; }
MHX_HD uint32_t line_rel_items(uint32_t packed) { return line_rel_full(packed) + line_rel_tails(packed); }
MHX_HD uint32_t line_rel_aligned(uint32_t packed) { return line_rel_items(packed) + (packed >> 20); }
MHX_HD bool line_rel_choose(uint32_t total)
{
#ifdef MHX_LINE_REL_ALWAYS   // A/B builds: every tile of the path takes the new items (profiles/line_rel_items_ab.txt, section 4)
    return true;
#else
    return ((line_rel_full(total) + 63u) >> 6) < ((line_rel_aligned(total) + 63u) >> 6);
#endif
}
// the line's items: at = the packed counts of the lanes in front, total = those of the whole tile
MHX_HD void phase_line_rel_items(TileSmem &sm, const LineSpan &s, uint32_t at, uint32_t total)
{
    if (!s.kmers) return;
    uint32_t pos = s.a, i = line_rel_full(at);
    // one 16-bit store and two additions per trip, as written: left to itself the compiler makes eight entries at a time with
    // packed arithmetic and stores them 16 bytes wide at addresses that are multiples of 2 (+145 VALU in the kernel's text)
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang loop vectorize(disable) interleave(disable) unroll(disable)
#endif
    for (uint32_t n = s.kmers >> 3; n; --n, pos += 8u) sm.list[i++] = (uint16_t)(pos | kLineRelFull);
    const uint32_t c = s.kmers & 7u;
    if (c) {
        sm.list[line_rel_full(total) + line_rel_tails(at)] = (uint16_t)pos;
        reinterpret_cast<uint8_t *>(sm.valid)[pos >> 3] = (uint8_t)((1u << c) - 1u);
    }
}

// P3: valid k-mer starts of this thread's positions -> sm.valid, #items -> sm.cnt
template <int K> MHX_HD uint32_t phase_runs(TileSmem &sm, int tid, uint32_t &items_out)
{
    constexpr int NWD = kWordsPerThread;
    uint32_t w[NWD + 1], v[NWD];
#pragma unroll
    for (int i = 0; i < NWD + 1; ++i) w[i] = tile_good(sm)[tid * NWD + i];
    run_starts<K, NWD>(w, v);
    uint32_t items = 0, kmers = 0;
#pragma unroll
    for (int i = 0; i < NWD; ++i) {
        sm.valid[tid * NWD + i] = v[i];
        kmers += (uint32_t)__builtin_popcount(v[i]);
        items += 4u - (uint32_t)__builtin_popcount(zero_byte_flags(v[i]));
    }
    items_out = items;
    return kmers;
}

// P4: append this thread's non-empty groups to the work list
MHX_HD void phase_compact(TileSmem &sm, int tid, uint32_t excl)
{
    uint32_t pos = excl;
#pragma unroll
    for (int i = 0; i < kWordsPerThread; ++i) {
        const uint32_t v = sm.valid[tid * kWordsPerThread + i];
#pragma unroll
        for (int b = 0; b < 4; ++b)
            if ((v >> (8 * b)) & 0xFFu) sm.list[pos++] = (uint16_t)((tid * kWordsPerThread + i) * 4 + b);
    }
    if (tid == kBlock - 1) sm.misc[1] = pos;
}

// ASCII complement of four folded bases at once: bits 1..2 of a base tell 'A','C','T','G' apart (0,1,2,3) and the
// complement comes out of a 4-byte table in one v_perm_b32.  Bytes that are not A/C/G/T come out as one of
// the four letters as well; a window that holds one never reaches the table (process_deferred checks the bases).
MHX_HD uint32_t complement4(uint32_t u) { return perm_lut(kLutComp, base_index(u)); }

// 64 bits starting at byte offset `off` (compile-time) of the dword array a
template <int OFF, int N> MHX_HD uint64_t load64(const uint32_t (&a)[N])
{
    constexpr int q = OFF / 4, sh = OFF % 4;
    static_assert(q + (sh ? 2 : 1) < N, "load64 out of range");
    const uint32_t lo = sh ? funnel(a[q + 1], a[q], sh) : a[q];
    const uint32_t hi = sh ? funnel(a[q + 2], a[q + 1], sh) : a[q + 1];
    return ((uint64_t)hi << 32) | lo;
}

// memcmp(fwd, rc, K) > 0, on the already extracted little-endian words (slow, exact)
template <int NW> MHX_HD bool rc_is_smaller_full(const uint32_t (&wf)[8], const uint32_t (&wr)[8])
{
    bool rc_less = false, decided = false;
#pragma unroll
    for (int i = 0; i < NW; ++i) {
        const uint32_t a = __builtin_bswap32(wf[i]), b = __builtin_bswap32(wr[i]);
        rc_less = decided ? rc_less : (b < a);
        decided = decided || (a != b);
    }
    return rc_less;
}

// K bytes at byte offset OFF of the dword array src, as zero-padded little-endian words
template <int K, int OFF, int N> MHX_HD void extract_words(const uint32_t (&src)[N], uint32_t (&w)[8])
{
    constexpr int NW = (K + 3) / 4;
#pragma unroll
    for (int i = 0; i < 8; ++i) w[i] = i < NW ? funnel(src[OFF / 4 + i + 1], src[OFF / 4 + i], OFF % 4) : 0u;
    if (K % 4) w[NW - 1] &= (1u << (8 * (K % 4))) - 1u;
}

// The strand of one window of K >= 8 bases: true = the reverse complement is the smaller one.  U = folded forward chunk,
// R = its reverse complement: the two views the hash reads, and the decision reads nothing else.  The words themselves are
// made by canonical_words, or by PairWords for two windows at once.
// memcmp(fwd, rc) compares big-endian, and the first 8 bases decide all but 4^-8 of the windows.  With u[] the folded bytes
// of the chunk, R[j] = comp(u[4 ND - 1 - j]).  The first 8 bases of the forward strand, most significant first, are the 8
// little-endian bytes at byte 4 ND - 8 - J of the byte-reversed chunk: the bytewise complement of B, the 8 bytes of R at
// that offset.  The first 8 bases of the reverse strand are the complements of the window's last 8 bytes, the 8 bytes A of
// U at byte J + K - 8.  On {A, C, G, T} the complement reverses the order (A < C < G < T <-> T > G > C > A) and is
// one-to-one, and the first differing byte decides a big-endian comparison, so
//     comp(A) < comp(B)  <=>  A > B        comp(A) == comp(B)  <=>  A == B:
// rc = B < A, and A == B falls back to the full comparison, is memcmp's answer for every window whose K bytes are A/C/G/T in
// either case.  A window that holds any other byte may get either answer (U keeps the raw folded byte where the complement
// table yields one of the four letters).  It does not matter: such a window is no set bit of the start mask (run_starts) or
// fails window_is_acgt / process_deferred's base check, so whatever it hashes to is thrown away -- the argument of the
// deferred base check and of the tail table.
template <int K, int J, int ND>
MHX_HD bool canonical_strand(const uint32_t (&U)[ND + 1], const uint32_t (&R)[ND + 1])
{
    static_assert(K >= 8, "shorter windows compare their extracted words");
    constexpr int NW = (K + 3) / 4;
    constexpr int OF = J;               // forward window starts at U byte OF
    constexpr int OR = ND * 4 - K - J;  // its reverse complement starts at R byte OR
    static_assert(J >= 0 && J + K <= 4 * ND, "the window lies inside the chunk");
    static_assert(J + K - 8 >= 0 && J + K <= 4 * (ND + 1), "A: 8 bytes inside U[0..ND]");
    static_assert(4 * ND - 8 - J >= 0 && 4 * ND - J <= 4 * (ND + 1), "B: 8 bytes inside R[0..ND]");
    if constexpr (K == 8 && J % 4 == 0) {
        // A and B are the two strands' own dword pairs as they stand, those of windows 0 and 4 one dword apart.  Written as
        // 64-bit values the compiler merges each pair into one 64-bit load of U resp. R, the overlapping loads keep both
        // arrays in memory, and every K = 8 kernel gets 32 bytes of scratch.  Compared half by half they stay registers.
        constexpr int QA = J / 4, QB = ND - 2 - J / 4;
        return R[QB + 1] < U[QA + 1] || (R[QB + 1] == U[QA + 1] && R[QB] < U[QA]);
    }
    const uint64_t top_a = load64<J + K - 8>(U);      // the window's last 8 bytes
    const uint64_t top_b = load64<ND * 4 - 8 - J>(R); // the reverse complement's last 8 bytes
    bool rc = top_b < top_a;
    if (MHX_UNLIKELY(K > 8 && top_a == top_b)) { // cold: exact comparison
        // the copies go through an opaque barrier so that the compiler cannot hoist the
        // word extraction of this 4^-8 case in front of the branch (it did: ~19 wasted
        // instructions per window on the hot path)
        uint32_t Uc[ND + 1], Rc[ND + 1];
#pragma unroll
        for (int i = 0; i < ND + 1; ++i) { Uc[i] = opaque(U[i]); Rc[i] = opaque(R[i]); }
        // word by word, most significant first: two temporaries instead of two extracted windows (the hash loop has no
        // registers to spare, and a spill here gives the whole kernel a scratch allocation)
        constexpr uint32_t last_mask = (K % 4) ? (1u << (8 * (K % 4))) - 1u : 0xFFFFFFFFu;
        bool rc_less = false, decided = false;
#pragma unroll
        for (int i = 0; i < NW; ++i) {
            uint32_t f = funnel(Uc[OF / 4 + i + 1], Uc[OF / 4 + i], OF % 4);
            uint32_t r = funnel(Rc[OR / 4 + i + 1], Rc[OR / 4 + i], OR % 4);
            if (i == NW - 1) { f &= last_mask; r &= last_mask; }
            const uint32_t fb = opaque(__builtin_bswap32(f)), rb = opaque(__builtin_bswap32(r));
            rc_less = decided ? rc_less : (rb < fb);
            decided = decided || (fb != rb);
        }
        rc = rc_less;
    }
    return rc;
}
// (the signature from when the decision read two views of its own, the forward chunk byte-reversed and complemented: the
// CPU emulators under tests/emul call it)
template <int K, int J, int ND>
MHX_HD bool canonical_strand(const uint32_t (&U)[ND + 1], const uint32_t (&R)[ND + 1], const uint32_t (&)[ND + 1], const uint32_t (&)[ND + 1])
{
    return canonical_strand<K, J, ND>(U, R);
}

// One window: the K bytes of its canonical strand as little-endian words.  U = folded forward chunk, R = its
// reverse complement.  Returns the strand: true = the reverse complement.
// BODY_ONLY (the hot loop with the tail block's partial word from packed digits, TailDigits below): only the full 8-byte
// words in front of the partial word, w[0 .. 2 * (K / 8)), are made; the rest of w is zero, and the source dwords and the
// funnel shifts that only the partial word read are not selected or made at all.
template <int K, int J, int ND, bool BODY_ONLY = false>
MHX_HD bool canonical_words(const uint32_t (&U)[ND + 1], const uint32_t (&R)[ND + 1], uint32_t (&w)[8])
{
    static_assert(!BODY_ONLY || K > 16, "the body-only form belongs to the tail table (64-bit hashes)");
    constexpr int NW = (K + 3) / 4;
    constexpr int OF = J;               // forward window starts at U byte OF
    constexpr int OR = ND * 4 - K - J;  // its reverse complement starts at R byte OR
    if constexpr (K >= 8) {
        const bool rc = canonical_strand<K, J, ND>(U, R);
        // select the source dwords first, extract once.  The last word keeps TB bytes, and a strand whose byte shift s has
        // s + TB <= 4 takes them all from S[NW - 1]: what it would pull in from S[NW] is masked away.  Both shifts are
        // compile-time constants (only WHICH of them applies is a per-lane run-time value, so the compiler cannot see it):
        //   neither strand reads S[NW]: it is not selected, and the last word is one bit-field extract of S[NW - 1];
        //   one strand reads it: that strand's dword is taken as it is, the other strand's garbage is masked away.
        if constexpr (BODY_ONLY) {
            constexpr int NBW = 2 * (K / 8); // dwords of the full 8-byte words; NBW < NW, so S[NBW] is a dword of the window
            static_assert(NBW < NW, "a partial word follows the body");
            uint32_t S[NBW + 1];
#pragma unroll
            for (int i = 0; i < NBW + 1; ++i) S[i] = rc ? R[OR / 4 + i] : U[OF / 4 + i];
            const uint32_t sh = rc ? 8u * (OR % 4) : 8u * (OF % 4);
#pragma unroll
            for (int i = 0; i < 8; ++i) w[i] = i < NBW ? funnel_bits(S[i + 1], S[i], sh) : 0u;
        } else {
            constexpr int TB = K - 4 * (NW - 1); // 1..4
            constexpr bool need_f = OF % 4 + TB > 4, need_r = OR % 4 + TB > 4;
            uint32_t S[NW];
#pragma unroll
            for (int i = 0; i < NW; ++i) S[i] = rc ? R[OR / 4 + i] : U[OF / 4 + i];
            const uint32_t sh = rc ? 8u * (OR % 4) : 8u * (OF % 4);
#pragma unroll
            for (int i = 0; i < 8; ++i)
                w[i] = i < NW - 1 ? funnel_bits(S[i + 1], S[i], sh) : 0u;
            if constexpr (!need_f && !need_r) {
                if constexpr (TB == 4) w[NW - 1] = S[NW - 1]; // both shifts are 0
                else w[NW - 1] = bit_field<8 * TB>(S[NW - 1], sh);
            } else {
                const uint32_t last = need_f && need_r ? (rc ? R[OR / 4 + NW] : U[OF / 4 + NW]) : need_f ? U[OF / 4 + NW] : R[OR / 4 + NW];
                w[NW - 1] = funnel_bits(last, S[NW - 1], sh);
                if constexpr (TB < 4) w[NW - 1] &= (1u << (8 * TB)) - 1u;
            }
        }
        return rc;
    } else {
        uint32_t wf[8], wr[8];
        extract_words<K, OF>(U, wf);
        extract_words<K, OR>(R, wr);
        const bool rc = rc_is_smaller_full<NW>(wf, wr);
#pragma unroll
        for (int i = 0; i < 8; ++i) w[i] = rc ? wr[i] : wf[i];
        return rc;
    }
}
// (the four-view signature, as canonical_strand's)
template <int K, int J, int ND, bool BODY_ONLY = false>
MHX_HD bool canonical_words(const uint32_t (&U)[ND + 1], const uint32_t (&R)[ND + 1], const uint32_t (&)[ND + 1], const uint32_t (&)[ND + 1],
                            uint32_t (&w)[8])
{
    return canonical_words<K, J, ND, BODY_ONLY>(U, R, w);
}

// P5: one work item = 8 consecutive window starts sharing one register chunk.
template <int K> struct GroupGeom {
    static constexpr int NB = kGroup + K - 1; // bytes touched
    static constexpr int ND = (NB + 3) / 4;   // dwords loaded
};

// complement4 of a group's dwords without the index shift: v & 0x06060606 (bits 1..2 of every byte where they stand; the
// case bit is not among them, so the raw bytes do) already tells 'A','C','T','G' apart, as the even selectors 0, 2, 4, 6
// of v_perm_b32's EIGHT-byte table: {'T', -, 'G', -} in the low dword, {'A', -, 'C', -} in the high one.  v_and + v_perm
// where base_index + perm_lut take v_lshrrev + v_and + v_perm, and the same byte for every input byte.  The two halves of
// the table differ and a VOP3 instruction of gfx950 reads one scalar operand, so the low half lives in a VGPR for the
// whole hash loop (opaque, or the compiler folds it back into a literal and a v_mov in front of every v_perm).
constexpr uint32_t kLutComp8Lo = 0x00470054u, kLutComp8Hi = 0x00430041u;
MHX_HD uint32_t complement_lut_lo()
{
    uint32_t lo = kLutComp8Lo;
#if defined(__HIP_DEVICE_COMPILE__)
    asm("" : "+v"(lo));
#endif
    return lo;
}
MHX_HD uint32_t complement4_raw(uint32_t v, uint32_t lut_lo)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_perm(kLutComp8Hi, lut_lo, v & 0x06060606u);
#else // the same look-up byte by byte: selectors 0..3 take the low dword's bytes, 4..7 the high one's
    const uint64_t lut = ((uint64_t)kLutComp8Hi << 32) | lut_lo;
    uint32_t o = 0;
    for (int i = 0; i < 4; ++i) o |= (uint32_t)((lut >> (8 * ((v >> (8 * i)) & 6u))) & 0xFFu) << (8 * i);
    return o;
#endif
}

// The two views of a group's chunk that canonical_strand, canonical_words and PairWords take: the folded forward chunk and
// its reverse complement (one dword of zero padding behind each)
template <int ND> MHX_HD void strand_views(const uint32_t (&src)[ND], uint32_t (&U)[ND + 1], uint32_t (&R)[ND + 1])
{
    const uint32_t lut_lo = complement_lut_lo();
#pragma unroll
    for (int d = 0; d < ND; ++d) {
        U[d] = src[d] & 0xDFDFDFDFu; // fold case: mash upper-cases before hashing
        R[d] = __builtin_bswap32(complement4_raw(src[ND - 1 - d], lut_lo));
    }
    U[ND] = R[ND] = 0;
}
// (the four-view signature, as canonical_strand's: Wr = the forward chunk byte-reversed, Cc = the forward chunk complemented,
// which nothing reads any more)
template <int ND>
MHX_HD void strand_views(const uint32_t (&src)[ND], uint32_t (&U)[ND + 1], uint32_t (&R)[ND + 1], uint32_t (&Wr)[ND + 1], uint32_t (&Cc)[ND + 1])
{
    strand_views<ND>(src, U, R);
#pragma unroll
    for (int d = 0; d < ND; ++d) {
        Wr[d] = __builtin_bswap32(U[ND - 1 - d]);
        Cc[d] = __builtin_bswap32(R[ND - 1 - d]);
    }
    Wr[ND] = Cc[ND] = 0;
}

// ---- the tail table's index from digits packed once per group --------------------------------------------------------
// The partial word of window J (T = K mod 8 bases behind K / 8 full words) is bytes J + 8 (K / 8) .. of U on the forward
// strand and bytes OR_J + 8 (K / 8) .., OR_J = 4 ND - K - J, of R on the reverse one.  Over J = 0..7 either range is T + 7
// bytes at a fixed place: from the dword-aligned byte 8 (K / 8) of U on, and the last T + 7 bytes of R -- inside NDW = 2
// (T = 1) or 3 consecutive dwords of each.  Their digits are packed once per group (tail_lut_pack) and kept as one 64-bit
// value, the reverse strand's word above the forward strand's, both shifted left by 3: a window's byte offset into the
// table is then v_cndmask (the shift: two inline constants per J, the reverse one 32 more), v_lshrrev_b64, v_and_b32 --
// three instructions where tail_lut_index took five on top of the select and the two funnel shifts that made the partial
// word itself.  (Selecting the word and the shift apart and extracting with v_bfe_u32 takes four, and measured a third less
// of the gain: profiles/tail_digits_ab.txt.)  What the shift brings down from the other word lands above the field.
// The offset equals 8 * tail_lut_index<T> of the partial word canonical_words yields: both are bits 1..2 of the same bytes
// (tests/emul/tail_digits_emul.cpp checks every K, J, strand and byte value).
template <int K> struct TailDigits {
    static constexpr int T = K & 7, Q = K / 8, ND = GroupGeom<K>::ND;
    static constexpr int NDW = (T + 7 + 3) / 4;  // dwords that hold the T + 7 bytes
    static constexpr int FD = 2 * Q;             // first of them in U
    static constexpr int RD = ND - NDW;          // first of them in R
    static_assert(T >= 1 && T <= 5 && NDW <= 3, "partial words of 1..5 bases: 8..12 bytes per strand");
    static_assert(FD + NDW <= ND + 1 && RD >= 0, "the packed dwords lie inside U[0..ND] and R[0..ND)");
    static_assert(4 * ND - K - 7 + 8 * Q >= 4 * RD, "reverse window 7 starts inside the packed dwords");
    static_assert(7 + 8 * Q + T <= 4 * (FD + NDW), "forward window 7 ends inside the packed dwords");
    template <int J> static constexpr uint32_t shift_f() { return 2u * J; }
    template <int J> static constexpr uint32_t shift_r() { return 2u * (uint32_t)(4 * ND - K - J + 8 * Q - 4 * RD); }
    uint64_t both; // {pr : pf} << 3
    MHX_HD TailDigits(const uint32_t (&U)[ND + 1], const uint32_t (&R)[ND + 1])
        : both(opaque64(make64(tail_lut_pack<NDW>(U[FD], U[FD + 1], U[FD + NDW - 1]), tail_lut_pack<NDW>(R[RD], R[RD + 1], R[RD + NDW - 1])) << 3)) {}
    // (neither word reaches its top three bits, so the compiler shifts the halves apart: two v_lshlrev_b32 in every kernel form)
    template <int J> MHX_HD uint32_t byte_offset(bool rc) const
    {
        static_assert(shift_f<J>() + 2 * T <= 8 * NDW && shift_r<J>() + 2 * T <= 8 * NDW, "the field lies inside the packed word");
        static_assert(8 * NDW + 3 <= 32 && 2 * T + 3 <= 32 - (int)shift_f<7>(), "what the other word shifts in stays above the field");
        uint32_t low = (uint32_t)(both >> (rc ? 32u + shift_r<J>() : shift_f<J>()));
#if defined(__HIP_DEVICE_COMPILE__)
        // opaque: left to see the truncation, the compiler masks the 64-bit value instead, and a 64-bit offset takes the
        // gather from its scalar-base form to a v_lshl_add_u64 and a load from a register pair
        asm("" : "+v"(low));
#endif
        return low & (((1u << (2 * T)) - 1u) << 3);
    }
};
// Which K of the hot loop take the index this way: K = 21 alone.  Packing costs the group 15 instructions, and only a
// partial word of five bases behind a full k1 word (tail_lut_index: 8 per window with its select and funnel shifts) pays
// that back: -23 of 648 hot VALU per group at K = 21.  With fewer bases the per-window index was cheap already (K = 17..20:
// +4..+12 per group), and the K = 25..29 kernels stand at 70..72 VGPRs, where the packed pair costs copies in the window blocks
// (K = 25..28: +4..+22) or, at K = 29, a scratch allocation in the inline form (profiles/tail_digits_ab.txt, section 1).
// Counted again with the strand decision on U and R alone: K = 25..28 +1..+22, K = 29 16 bytes of scratch in the queue forms
// (profiles/strand_views_ab.txt, section 1).
template <int K> constexpr bool tail_digits_apply() { return K == 21; }
struct NoTailDigits { // stands in where the index is not taken from packed digits
    template <class A, class B> MHX_HD NoTailDigits(const A &, const B &) {}
};
// One window of the hot loop, up to the last multiplication of the hash.  LUT: the tail block's partial word from the
// table (the device's hot loop, hot_tail_lut<K>()); with a TailDigits<K> its index comes from the group's packed digits
// and only the body words of the canonical strand are extracted, otherwise from the partial word itself.
template <int K, int J, int ND, bool LUT, class Digits>
MHX_HD Murmur3Tail window_partial_hash(const uint32_t (&U)[ND + 1], const uint32_t (&R)[ND + 1], const Digits &digits, TailLutPtr lut)
{
    uint32_t w[8];
    if constexpr (LUT && std::is_same<Digits, TailDigits<K>>::value) {
        const bool rc = canonical_words<K, J, ND, true>(U, R, w);
        return murmur3_blocks<K, true>(w, tail_lut_at(lut, digits.template byte_offset<J>(rc)));
    } else {
        canonical_words<K, J, ND>(U, R, w);
        return murmur3_core<K, LUT>(w, lut);
    }
}
// (the four-view signature, as canonical_strand's)
template <int K, int J, int ND, bool LUT, class Digits>
MHX_HD Murmur3Tail window_partial_hash(const uint32_t (&U)[ND + 1], const uint32_t (&R)[ND + 1], const uint32_t (&)[ND + 1],
                                       const uint32_t (&)[ND + 1], const Digits &digits, TailLutPtr lut)
{
    return window_partial_hash<K, J, ND, LUT>(U, R, digits, lut);
}

// ---- the words of windows J and J + 4 from one funnel shift per strand -----------------------------------------------
// canonical_words selects the strand's source dwords per window and funnels afterwards, because WHICH strand applies is a
// per-lane run-time value.  The two byte shifts themselves are compile-time constants, J % 4 forward and (4 ND - K - J) % 4
// reverse, and windows J and J + 4 (J = 0..3) share both: forward window J + 4 starts one dword behind window J, reverse
// window J + 4 one dword in front of it.  So each strand is funnelled once per pair, NWD + 1 dwords for the NWD dwords of
// either window -- F[0..NWD) / G[1..NWD] for J, F[1..NWD] / G[0..NWD) for J + 4 -- and a strand whose shift is 0 is its
// source dwords as they stand.  A window is then its strand decision and one select per dword: per group of eight 30
// funnel shifts and 32 selects at K = 21 where 8 x (6 selects + 4 funnel shifts) stood.
// BODY_ONLY: NWD = 2 (K / 8), the full 8-byte words in front of the partial word, as canonical_words' form of that name
// (the K whose table index comes from TailDigits); otherwise all (K + 3) / 4 dwords, the last one masked to its bytes.
// (tests/emul/pair_words_emul.cpp compares the words with canonical_words' for every K, J and strand.)
template <int K, int J, int ND, bool BODY_ONLY> struct PairWords {
    static constexpr int NW = (K + 3) / 4;
    static constexpr int NWD = BODY_ONLY ? 2 * (K / 8) : NW; // dwords of one window made here
    static constexpr int OF = J, OR = 4 * ND - K - J;  // window J: first byte in U, first byte in R
    static constexpr int SF = OF % 4, SR = OR % 4;     // the pair's two byte shifts
    static constexpr int FD = OF / 4, RD = OR / 4 - 1; // first source dword: forward of window J, reverse of window J + 4
    static_assert(J >= 0 && J < 4 && K > 16, "pairs (J, J + 4) of the 64-bit hashes");
    static_assert(NWD > 0 && NWD <= 8 && 4 * NWD <= K + 3, "the dwords made lie inside the window");
    static_assert((OF + 4) % 4 == SF && (OF + 4) / 4 == FD + 1, "forward window J + 4 starts one dword behind window J");
    static_assert(OR - 4 >= 0 && (OR - 4) % 4 == SR && (OR - 4) / 4 == RD, "reverse window J + 4 starts at byte OR - 4 >= 0, one dword in front");
    static_assert(FD + NWD + (SF ? 1 : 0) <= ND && RD + NWD + (SR ? 1 : 0) <= ND, "the source dwords lie inside U[0..ND] and R[0..ND]");
    uint32_t F[NWD + 1], G[NWD + 1];
    MHX_HD PairWords(const uint32_t (&U)[ND + 1], const uint32_t (&R)[ND + 1])
    {
#pragma unroll
        for (int i = 0; i < NWD + 1; ++i) {
            F[i] = SF ? funnel(U[FD + i + 1], U[FD + i], SF) : U[FD + i];
            G[i] = SR ? funnel(R[RD + i + 1], R[RD + i], SR) : R[RD + i];
        }
    }
    // the words of window J (SECOND = false) or J + 4 on the strand rc, as canonical_words<K, J (+ 4), ND, BODY_ONLY> yields them
    template <bool SECOND> MHX_HD void words(bool rc, uint32_t (&w)[8]) const
    {
#pragma unroll
        for (int i = 0; i < 8; ++i) w[i] = i < NWD ? (rc ? G[i + (SECOND ? 0 : 1)] : F[i + (SECOND ? 1 : 0)]) : 0u;
        if constexpr (!BODY_ONLY && K % 4 != 0) w[NW - 1] &= (1u << (8 * (K % 4))) - 1u;
    }
};
// Which K take their words from PairWords, and which kernel forms of such a K (fmt, queue: sketch_tile_kernel's FMT and
// QUEUE).  The hot loop has no register to spare and the pair is alive across two windows, so a form takes the route only
// where it stays at 72 VGPRs, no scratch and seven waves per SIMD, and a K only where the loop then loses at least 10 VALU
// instructions per group (profiles/pair_words_ab.txt, section 1):
//   K = 17, 18, 19, 21, 23: every form but the inline ones of the look-back repair kernel (FMT 1), which stand at 72 VGPRs
//       already (K = 21: 12 bytes of scratch with the pair);
//   K = 25, 26, 27, 29: the queue forms; the inline forms spill (12..68 bytes);
//   K = 20, 24, 28: -6 per group, left alone; K = 22: left alone as the control of the A/B runs; K = 30..32: forms of these
//       spill as they are, left alone.
// (The figures are those of when the switch was set.  Since the strand decision reads U and R alone, the FMT 1 inline forms of
// K = 17, 18, 19, 21, 23 and the inline forms of K = 25 would pass the rule, those of K = 26, 27, 29 still take scratch, and
// K = 30..32 no longer spill: profiles/strand_views_ab.txt, section 1.  The switch stands as tests/test_pair_words.py pins it.)
template <int K> constexpr bool pair_words_apply()
{
    return K == 17 || K == 18 || K == 19 || K == 21 || K == 23 || K == 25 || K == 26 || K == 27 || K == 29;
}
template <int K> constexpr bool pair_words_form(int fmt, bool queue)
{
    return pair_words_apply<K>() && (K > 24 ? queue : fmt != 1 || queue);
}
// Windows J (SECOND = false) and J + 4 of the hot loop by that route, up to the last multiplication of the hash: the
// counterpart of window_partial_hash
template <int K, int J, int ND, bool SECOND, bool LUT, bool BODY_ONLY, class Digits>
MHX_HD Murmur3Tail window_pair_hash(const PairWords<K, J, ND, BODY_ONLY> &pair, const uint32_t (&U)[ND + 1], const uint32_t (&R)[ND + 1],
                                    const Digits &digits, TailLutPtr lut)
{
    constexpr int JW = J + (SECOND ? 4 : 0);
    uint32_t w[8];
    const bool rc = canonical_strand<K, JW, ND>(U, R);
    pair.template words<SECOND>(rc, w);
    if constexpr (BODY_ONLY) {
        static_assert(LUT && std::is_same<Digits, TailDigits<K>>::value, "the body-only form takes the table index from packed digits");
        return murmur3_blocks<K, true>(w, tail_lut_at(lut, digits.template byte_offset<JW>(rc)));
    } else {
        return murmur3_core<K, LUT>(w, lut);
    }
}

// Cold path, reached by one window in ~2^64 / T: are bytes J .. J+K-1 of the chunk all A/C/G/T (either case)?
// mash skips every window that holds anything else (Sketch.cpp addMinHashes).
// (chunk: the raw or the case-folded bytes, the test folds anyway)
template <int K, int J, int ND> MHX_HD bool window_is_acgt(const uint32_t (&chunk)[ND + 1])
{
    uint64_t m = 0;
#pragma unroll
    for (int d = 0; d < ND; ++d) m |= (uint64_t)flags_to_nibble(acgt_flags(chunk[d])) << (4 * d);
    constexpr uint64_t want = (K >= 64 ? ~0ull : ((1ull << K) - 1ull)) << J;
    return (m & want) == want;
}

// vm: bits 0..7 the candidate-start mask of the group, bits 8.. the group's number (it rides along in the same register:
// the hash loop has none to spare).  A window that is a valid start and whose partial hash passes the admission test
// (`limit` = admission_limit(T); 32-bit hashes: the exact low word against T) is
//   QUEUE = false: finished where it is found: ins(h) if its bases are all A/C/G/T and h <= T (returns their number);
//   QUEUE = true : handed to cand(group, J) (queued, finished later by process_deferred).
// Two forms because each costs the other's workload something: with a small sketch (s = 1000, one candidate in 10^4
// windows) the inline form is 0.8 % faster (the queue's cold branch changes the register allocation of the hot path by
// one v_mov per window); with a large one (s = 50 000) the queue is 7 % faster.
// lut: hot_tail_table<K>(), fetched by the caller in front of its loop over the groups (nullptr: formed here).
// PAIRS: the words of windows J and J + 4 from one PairWords (the kernel forms pair_words_form names).  The windows then
// run (0,4)(1,5)(2,6)(3,7); what is done with each stays per window.
// TAIL: a trip made of tail items alone (line-relative items, phase_line_rel_items: the masks are (1 << c) - 1): the windows
// run 0..7 one by one, without pairs, and the wave leaves in front of the first window no lane of it has -- a scalar test.
template <int K, bool QUEUE, bool PAIRS = false, bool TAIL = false, class Ins, class Cand>
MHX_HD uint32_t process_group_regs(const uint32_t (&src)[GroupGeom<K>::ND], uint32_t vm, uint64_t T, uint32_t limit, Ins &ins, Cand &cand,
                                   TailLutPtr lut)
{
    constexpr int ND = GroupGeom<K>::ND;
    uint32_t U[ND + 1], R[ND + 1];
    strand_views<ND>(src, U, R);
    constexpr bool kHash32 = K <= 16; // mash keeps 32 bits when 4^k <= 2^32
    uint32_t ninserted = 0;
    constexpr bool kLut = hot_tail_lut<K>();
    // a K that keeps the per-window index also keeps the address where it was formed, here (hot_tail_table)
    if constexpr (kLut && !tail_digits_apply<K>()) lut = tail_lut_of<K>();
    const std::conditional_t<kLut && tail_digits_apply<K>(), TailDigits<K>, NoTailDigits> digits(U, R);
    constexpr bool kDigits = kLut && tail_digits_apply<K>();
    constexpr bool kPairs = PAIRS && !TAIL && pair_words_apply<K>();
#define MHX_WINDOW(J) MHX_WINDOW_OF(J, (window_partial_hash<K, J, ND, kLut>(U, R, digits, lut)))
#define MHX_PAIR(J)                                                                           \
    {                                                                                         \
        const PairWords<K, J, ND, kDigits> pair(U, R);                                        \
        MHX_WINDOW_OF(J, (window_pair_hash<K, J, ND, false, kLut>(pair, U, R, digits, lut)))          \
        MHX_WINDOW_OF(J + 4, (window_pair_hash<K, J, ND, true, kLut>(pair, U, R, digits, lut)))       \
    }
#define MHX_WINDOW_OF(J, HASH)                                                                \
    {                                                                                         \
        if constexpr (TAIL && (J) > 0) { if (!wave_any(((vm & 0xFFu) >> (J)) != 0u)) goto windows_done; } \
        const Murmur3Tail tail = HASH;                                                        \
        /* necessary condition of h <= T, see Murmur3Tail (32-bit hashes: the exact low word) */ \
        const uint32_t low = kHash32 ? tail.low32() : 0u;                                     \
        const bool candidate = kHash32 ? low <= (uint32_t)T : tail.high_bound() <= limit;     \
        if (MHX_UNLIKELY(candidate)) {                                                        \
            if constexpr (QUEUE) {                                                            \
                if ((vm >> J) & 1u) cand(vm >> 8, J);                                         \
            } else {                                                                          \
                const uint64_t h = kHash32 ? (uint64_t)low : tail.finish();                   \
                if (((vm >> J) & 1u) && h <= T && window_is_acgt<K, J, ND>(U)) { ins(h); ++ninserted; } \
            }                                                                                 \
        }                                                                                     \
    }
    if constexpr (kPairs) {
        MHX_PAIR(0) MHX_PAIR(1) MHX_PAIR(2) MHX_PAIR(3)
    } else {
        MHX_WINDOW(0) MHX_WINDOW(1) MHX_WINDOW(2) MHX_WINDOW(3) MHX_WINDOW(4) MHX_WINDOW(5) MHX_WINDOW(6) MHX_WINDOW(7)
    }
#undef MHX_WINDOW_OF
#undef MHX_PAIR
#undef MHX_WINDOW
    static_assert(kGroup == 8, "process_group unrolls 8 windows");
windows_done:
    return ninserted;
}

// The tail table as the kernel fetches it in front of its loop over the groups, once per workgroup: fetched inside
// process_group_regs, the address is formed anew in the header of every trip (tail_lut_table: s_getpc_b64, two adds, a
// load from the GOT and a wait).  Only for the K that pack their digits; nullptr for every other K, whose kernels stay
// the instructions they were: with the address in front of the loop for every K with a table, the queue form of K = 27
// -- the same VALU count block for block, other registers -- measured 0.2..0.3 % slower than two builds of the commit
// before in each of six rounds (profiles/tail_digits_ab.txt, section 3), so those K form it where they did.
template <int K> MHX_HD TailLutPtr hot_tail_table()
{
    if constexpr (hot_tail_lut<K>() && tail_digits_apply<K>()) return tail_lut_of<K>();
    else return nullptr;
}

// work item g of a staged tile (LDS source)
template <int K, bool QUEUE, bool PAIRS = false, class Ins, class Cand>
MHX_HD uint32_t process_group(const TileSmem &sm, uint32_t g, uint64_t T, uint32_t limit, Ins &ins, Cand &cand, TailLutPtr lut)
{
    constexpr int ND = GroupGeom<K>::ND;
    const uint32_t vm = reinterpret_cast<const uint8_t *>(sm.valid)[g] | (g << 8);
    const uint32_t *p = reinterpret_cast<const uint32_t *>(sm.bytes) + 2 * g;
    uint32_t src[ND];
#pragma unroll
    for (int d = 0; d < ND; ++d) src[d] = p[d];
    return process_group_regs<K, QUEUE, PAIRS>(src, vm, T, limit, ins, cand, lut);
}
template <int K, bool QUEUE, class Ins, class Cand>
MHX_HD uint32_t process_group(const TileSmem &sm, uint32_t g, uint64_t T, uint32_t limit, Ins &ins, Cand &cand)
{
    return process_group<K, QUEUE>(sm, g, T, limit, ins, cand, hot_tail_table<K>());
}

// ---- a line-relative item (phase_line_rel_items) of a staged tile --------------------------------------------------------
// The item's 4 ND source bytes begin at its byte position, which is no multiple of 4 any more (at most kTileBytes - 1, and
// 4 ND <= 40: inside the halo).  One copy of 4 ND bytes at alignment 1, which the compiler makes wide DS reads of at the byte
// address (ds_read_b96 + ds_read_b128 at K = 21).  Of the three spellings measured at the bench setting this is the fastest
// (profiles/line_rel_items_ab.txt, section 5): ND + 1 aligned dwords with one v_alignbyte_b32 per source dword gave about a
// quarter of the gain back, one dword read per source dword at the byte address was 4 % slower than the commit before.
template <int ND> MHX_HD void line_rel_source(const TileSmem &sm, uint32_t pos, uint32_t (&src)[ND])
{
    __builtin_memcpy(src, reinterpret_cast<const uint8_t *>(sm.bytes) + pos, 4 * ND);
}
// the item's mask and position as process_group_regs takes them (vm: the mask below the position, which stands where the
// group's number stood: a candidate of window J is the byte position (vm >> 8) + J)
MHX_HD uint32_t line_rel_vm(const TileSmem &sm, uint32_t entry)
{
    const uint32_t pos = entry & kLineRelPos;
    uint32_t mask = 0xFFu;
    if (!(entry & kLineRelFull)) mask = reinterpret_cast<const uint8_t *>(sm.valid)[pos >> 3];
    return mask | (pos << 8);
}
template <int K, bool QUEUE, bool PAIRS, bool TAIL, class Ins, class Cand>
MHX_HD uint32_t process_line_rel_item(const TileSmem &sm, uint32_t entry, uint64_t T, uint32_t limit, Ins &ins, Cand &cand, TailLutPtr lut)
{
    constexpr int ND = GroupGeom<K>::ND;
    static_assert(kTileBytes - 1 + 4 * ND <= kTileBytes + kHaloBytes, "an item's source bytes are staged");
    const uint32_t vm = line_rel_vm(sm, entry);
    uint32_t src[ND];
    line_rel_source<ND>(sm, vm >> 8, src);
    return process_group_regs<K, QUEUE, PAIRS, TAIL>(src, vm, T, limit, ins, cand, lut);
}

// A queued candidate (code = (group << 3) | window), finished from the staged bytes with a window offset known only at
// run time: the K bytes by funnel shifts out of LDS, base check, reverse complement of those K bytes, the exact strand
// comparison, the whole hash.  Slower per window than the unrolled hot path, but run one candidate per lane.
template <int K, class Ins> MHX_HD uint32_t process_deferred(const TileSmem &sm, uint32_t code, uint64_t T, Ins &ins)
{
    constexpr int NW = (K + 3) / 4;
    constexpr uint32_t tail_mask = (K % 4) ? (1u << (8 * (K % 4))) - 1u : 0xFFFFFFFFu;
    const uint32_t pos = 8u * (code >> 3) + (code & 7u);
    const uint32_t *b = reinterpret_cast<const uint32_t *>(sm.bytes) + (pos >> 2);
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
    if ((ok_bits & want) != want) return 0u; // mash skips every window that holds anything but A/C/G/T
    wf[NW - 1] &= tail_mask;
#pragma unroll
    for (int d = NW; d < 8; ++d) wf[d] = 0u;
    // reverse complement: the 4*NW bytes reversed and complemented put the window's K bytes behind 4*NW - K bytes of padding
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
    const uint64_t h = K <= 16 ? (uint64_t)tail.low32() : tail.finish();
    if (h > T) return 0u;
    ins(h);
    return 1u;
}

} // namespace mhx
