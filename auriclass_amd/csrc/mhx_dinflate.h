// mhx_dinflate.h -- per-lane logic of the device DEFLATE decoder (mhx_dinflate.hip), written as host+device inline
// functions in the way of mhx_tile.h: the kernels call them one lane per segment or candidate position, and the CPU
// emulator (tests/emul/dinflate_emul.cpp) runs the very same functions, and the very same round driver, lane by lane.
//
// One gzip member on the device (the design of the host's mhx_pinflate.cpp, moved to many more lanes):
//   search     the member is cut at target bit offsets (seg_bits apart); for each target the first later bit position
//              (below the next target) where a dynamic-Huffman block header is valid -- BTYPE 2, HLIT/HDIST in range, a
//              complete code-length code, complete literal/length and distance codes, an end-of-block code -- becomes a
//              segment start.  Lanes test consecutive positions.  Segment 0 starts at the true start.
//   decode     each segment is decoded by one lane into 16-bit symbols: a byte, or kMarker | w = "byte w of the unknown
//              32 KiB in front of the segment".  Blocks are decoded while their header lies before the next segment's
//              start, so a segment ends on a block boundary at or past its successor's start; it records that bit, its
//              symbol count and whether it saw the final block.  The count stays exact when the symbol slab is full.
//   chain      segment j is right if segment j-1 is right and stopped exactly where j started (segment 0 is right:
//              induction).  A broken link is redone from where the predecessor stopped, at most kMaxPasses times.
//   resolve    markers read the output in front of the segment: first the last 32 KiB of every segment, in order (one
//              workgroup walks the chain), then everything else in parallel.
//   crc        CRC-32 per segment on the device; the host joins them (crc32_combine) and checks the trailer.
// Work goes in rounds (search, decode, chain, resolve, CRC each), so device memory stays bounded for any member: a round's
// first segment starts where the previous round verifiably stopped, its markers read the previous round's output.  The
// first round is small and each further one twice as large, up to a bound, so a small member costs one small round.
//
// Robustness: every loop is bounded by input bits or output capacity, reads past the input return zero bits and are
// reported, every table index is masked or checked.  A failure of any kind is reported to the caller, whose rule is
// that the host decoder then has the last word.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#ifndef MHX_HD
#define MHX_HD __host__ __device__ __forceinline__
#endif
#else
#ifndef MHX_HD
#define MHX_HD inline
#endif
#endif

#include <algorithm>
#include <vector>

namespace mhx {
namespace dinf {

constexpr uint32_t kWin = 32768;
constexpr uint16_t kMarker = 0x8000;
constexpr uint64_t kNoBit = ~0ull;         // "no candidate" / "no stop target"
constexpr int kLitBits = 11, kDistBits = 8;
constexpr int kLitCap = (1 << kLitBits) + 288 * 16, kDistCap = (1 << kDistBits) + 32 * 128;
constexpr int kLaneWords = kLitCap + kDistCap + 320 / 4; // per-lane workspace: both tables and the code lengths
constexpr int kMaxPasses = 16;

// segment status
enum : uint32_t { kSegOk = 0, kSegData = 1, kSegEnd = 2 };

// table entries (the layout of the host decoder, mhx_inflate_impl.h): bits 0..7 bits to consume (or index bits of the
// sub-table), 8 literal, 9 end of block, 10 sub-table link, 11 invalid, 12 length/distance base, 13..16 extra bits,
// 17..31 the literal, base or sub-table offset
constexpr uint32_t kLiteral = 0x0100, kEnd = 0x0200, kSub = 0x0400, kInvalid = 0x0800, kBase = 0x1000;
constexpr int kValShift = 17, kExtraShift = 13;

MHX_HD uint32_t len_base(int i)
{
    const uint16_t t[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
    return t[i];
}
MHX_HD uint32_t len_extra(int i) { return i < 8 || i == 28 ? 0u : (uint32_t)((i - 4) >> 2); }
MHX_HD uint32_t dist_base(int i)
{
    const uint16_t t[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577};
    return t[i];
}
MHX_HD uint32_t dist_extra(int i) { return i < 4 ? 0u : (uint32_t)((i - 2) >> 1); }
MHX_HD int clen_order(int i)
{
    const uint8_t t[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    return t[i];
}

// ---- bit input: reads past the n bytes return zero bits; pos() > 8 n tells that it happened ----
struct Bits {
    const uint8_t *p;
    uint64_t n;    // bytes of input
    uint64_t next; // next byte to load
    uint64_t buf;
    int cnt;
    MHX_HD void refill()
    {
        if (next + 8 <= n) {
            uint64_t v;
            memcpy(&v, p + next, 8);
            buf |= v << cnt;
            next += (uint64_t)((63 - cnt) >> 3);
            cnt |= 56;
        } else {
            while (cnt <= 56) {
                const uint64_t b = next < n ? p[next] : 0;
                buf |= b << cnt;
                ++next;
                cnt += 8;
            }
        }
    }
    MHX_HD void seek(uint64_t bit)
    {
        next = bit >> 3;
        buf = 0;
        cnt = 0;
        refill();
        drop((int)(bit & 7));
    }
    MHX_HD uint32_t peek(int k) const { return (uint32_t)(buf & ((1ull << k) - 1)); }
    MHX_HD void drop(int k) { buf >>= k; cnt -= k; }
    MHX_HD uint32_t take(int k)
    {
        if (cnt < k) refill();
        const uint32_t v = peek(k);
        drop(k);
        return v;
    }
    MHX_HD uint64_t pos() const { return next * 8 - (uint64_t)cnt; }
    MHX_HD bool over() const { return pos() > n * 8; }
};

// ---- the code-length code: decoded bit by bit from counts (19 symbols, 7 bits at most) ----
struct ClenCode {
    uint8_t count[8];
    uint8_t sym[19];
};
// false: over-subscribed (complete: Kraft sum exactly 1)
MHX_HD bool clen_build(const uint8_t *lens19, ClenCode &c, bool *complete)
{
    for (int l = 0; l < 8; ++l) c.count[l] = 0;
    for (int i = 0; i < 19; ++i) c.count[lens19[i] & 7]++;
    int left = 1;
    for (int l = 1; l < 8; ++l) {
        left <<= 1;
        left -= c.count[l];
        if (left < 0) return false;
    }
    *complete = left == 0;
    uint8_t offs[8];
    offs[1] = 0;
    for (int l = 1; l < 7; ++l) offs[l + 1] = (uint8_t)(offs[l] + c.count[l]);
    for (int i = 0; i < 19; ++i)
        if (lens19[i]) c.sym[offs[lens19[i] & 7]++] = (uint8_t)i;
    return true;
}
// symbol or -1 (no code of <= 7 bits matches: incomplete code)
MHX_HD int clen_decode(Bits &b, const ClenCode &c)
{
    if (b.cnt < 8) b.refill();
    int code = 0, first = 0, index = 0;
    for (int l = 1; l < 8; ++l) {
        code |= (int)(b.buf & 1);
        b.drop(1);
        const int count = c.count[l];
        if (code - count < first) return c.sym[(index + (code - first)) % 19];
        index += count;
        first += count;
        first <<= 1;
        code <<= 1;
    }
    return -1;
}

// Reads HLIT/HDIST/HCLEN, the code-length code and the code lengths.  lens (320 bytes) receives the literal/length
// lengths at [0, 288) and the distance lengths at [288, 320) when non-null; kraft[0]/[1] receive the Kraft sums (in units of
// 2^-15) of the literal/length and distance codes, eob whether symbol 256 has a code.  Returns false on an invalid header.
MHX_HD bool read_dynamic(Bits &b, uint8_t *lens, bool strict, uint32_t *kraft, bool *eob)
{
    if (b.cnt < 14) b.refill();
    const int nlit = (int)b.take(5) + 257, ndist = (int)b.take(5) + 1, nclen = (int)b.take(4) + 4;
    if (nlit > 286 || ndist > 30) return false;
    uint8_t cl[19];
    for (int i = 0; i < 19; ++i) cl[i] = 0;
    for (int i = 0; i < nclen; ++i) cl[clen_order(i)] = (uint8_t)b.take(3);
    if (b.over()) return false;
    ClenCode cc;
    bool complete = false;
    if (!clen_build(cl, cc, &complete)) return false;
    if (strict && !complete) return false;
    uint32_t k0 = 0, k1 = 0;
    int prev = 0;
    bool has_eob = false;
    int i = 0;
    while (i < nlit + ndist) {
        const int sym = clen_decode(b, cc);
        if (sym < 0) return false;
        int rep = 1, val = sym;
        if (sym == 16) {
            if (i == 0) return false;
            val = prev;
            rep = 3 + (int)b.take(2);
        } else if (sym == 17) { val = 0; rep = 3 + (int)b.take(3); }
        else if (sym == 18) { val = 0; rep = 11 + (int)b.take(7); }
        if (i + rep > nlit + ndist) return false;
        if (b.over()) return false;
        for (int r = 0; r < rep; ++r, ++i) {
            if (i < nlit) {
                if (val) k0 += 1u << (15 - val);
                if (i == 256) has_eob = val != 0;
                if (lens) lens[i] = (uint8_t)val;
            } else {
                if (val) k1 += 1u << (15 - val);
                if (lens) lens[288 + i - nlit] = (uint8_t)val;
            }
        }
        prev = val;
    }
    if (lens) {
        for (int j = nlit; j < 288; ++j) lens[j] = 0;
        for (int j = ndist; j < 32; ++j) lens[288 + j] = 0;
    }
    kraft[0] = k0;
    kraft[1] = k1;
    *eob = has_eob;
    return true;
}

// Search test: is `bit` the start of a dynamic-Huffman block header that a real encoder could have written?
MHX_HD bool header_candidate(const uint8_t *in, uint64_t n, uint64_t bit)
{
    Bits b{in, n, 0, 0, 0};
    b.seek(bit);
    b.drop(1); // BFINAL: either
    if (b.take(2) != 2) return false;
    uint32_t kraft[2];
    bool eob = false;
    if (!read_dynamic(b, nullptr, true, kraft, &eob)) return false;
    if (!eob || kraft[0] != 32768u) return false;
    // distances: complete, or the single one-bit code that encoders write for a block with one distance (or none)
    if (kraft[1] != 32768u && kraft[1] != 16384u) return false;
    return !b.over();
}

// ---- decode tables (the host decoder's construction): false for an over-subscribed code or a table overflow ----
MHX_HD uint32_t payload(int kind, int s)
{
    if (kind == 0) { // literal/length
        if (s < 256) return kLiteral | ((uint32_t)s << kValShift);
        if (s == 256) return kEnd;
        if (s > 285) return kInvalid;
        return kBase | (len_base(s - 257) << kValShift) | (len_extra(s - 257) << kExtraShift);
    }
    if (s > 29) return kInvalid;
    return kBase | (dist_base(s) << kValShift) | (dist_extra(s) << kExtraShift);
}
MHX_HD bool build_table(const uint8_t *lens, int nsym, int first_bits, uint32_t *table, int cap, int kind)
{
    int count[16];
    for (int l = 0; l < 16; ++l) count[l] = 0;
    for (int i = 0; i < nsym; ++i) ++count[lens[i] & 15];
    count[0] = 0;
    int max_len = 15;
    while (max_len > 0 && count[max_len] == 0) --max_len;
    uint32_t next_code[16];
    uint32_t code = 0;
    int left = 1;
    next_code[0] = 0;
    for (int l = 1; l <= 15; ++l) {
        left <<= 1;
        left -= count[l];
        if (left < 0) return false;
        code = (code + (uint32_t)count[l - 1]) << 1;
        next_code[l] = code;
    }
    const int first_size = 1 << first_bits;
    for (int i = 0; i < first_size; ++i) table[i] = kInvalid | 1u;
    int sub_next = first_size;
    const int sub_bits = max_len > first_bits ? max_len - first_bits : 0;
    for (int sym = 0; sym < nsym; ++sym) {
        const int l = lens[sym] & 15;
        if (!l) continue;
        const uint32_t c = next_code[l]++;
        uint32_t r = 0;
        for (int i = 0; i < l; ++i) r |= ((c >> i) & 1u) << (l - 1 - i);
        if (l <= first_bits) {
            const uint32_t e = payload(kind, sym) | (uint32_t)l;
            for (uint32_t i = r; i < (uint32_t)first_size; i += 1u << l) table[i] = e;
        } else {
            const uint32_t lo = r & (uint32_t)(first_size - 1);
            uint32_t head = table[lo];
            if (!(head & kSub)) {
                if (sub_next + (1 << sub_bits) > cap) return false;
                head = kSub | (uint32_t)sub_bits | ((uint32_t)sub_next << kValShift);
                table[lo] = head;
                for (int i = 0; i < (1 << sub_bits); ++i) table[sub_next + i] = kInvalid | 1u;
                sub_next += 1 << sub_bits;
            }
            const uint32_t base = head >> kValShift;
            const uint32_t e = payload(kind, sym) | (uint32_t)(l - first_bits);
            for (uint32_t i = r >> first_bits; i < (1u << sub_bits); i += 1u << (l - first_bits)) table[base + i] = e;
        }
    }
    return true;
}
MHX_HD void fixed_lens(uint8_t *lens)
{
    for (int i = 0; i < 288; ++i) lens[i] = (uint8_t)(i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : 8);
    for (int i = 0; i < 32; ++i) lens[288 + i] = 5;
}

// ---- one segment, symbolically ----
struct SegResult {
    uint64_t stop_bit; // bit after the last block decoded
    uint64_t n_sym;    // symbols produced (exact even when more than the slab holds)
    uint32_t status;   // kSeg*
    uint32_t final_block;
};

// Decodes blocks from start_bit while their header lies before stop_target (kNoBit: until the final block).  Symbols go to
// sym[0, cap); window: a match may reach up to 32 KiB in front of the segment (markers), else that is an error (the start
// of a member).  ws: kLaneWords words of workspace.
MHX_HD void decode_segment(const uint8_t *in, uint64_t n, uint64_t start_bit, uint64_t stop_target, bool window,
                           uint16_t *sym, uint64_t cap, uint32_t *ws, SegResult *res)
{
    uint32_t *lit = ws, *dist = ws + kLitCap;
    uint8_t *lens = (uint8_t *)(ws + kLitCap + kDistCap);
    Bits b{in, n, 0, 0, 0};
    b.seek(start_bit);
    uint64_t o = 0;
    uint32_t status = kSegOk, final_block = 0;
    const uint64_t hist = window ? kWin : 0;
    while (!final_block && b.pos() < stop_target) {
        if (b.over()) { status = kSegEnd; break; }
        if (b.cnt < 3) b.refill();
        final_block = b.take(1);
        const uint32_t type = b.take(2);
        if (type == 0) {
            b.drop(b.cnt & 7);
            if (b.cnt < 32) b.refill();
            const uint32_t len = b.take(16), nlen = b.take(16);
            if (b.over()) { status = kSegEnd; break; }
            if ((len ^ nlen) != 0xFFFFu) { status = kSegData; break; }
            if (b.pos() / 8 + len > n) { status = kSegEnd; break; }
            for (uint32_t i = 0; i < len; ++i) {
                const uint32_t v = b.take(8);
                if (o < cap) sym[o] = (uint16_t)v;
                ++o;
            }
            continue;
        }
        if (type == 3) { status = kSegData; break; }
        if (type == 1) fixed_lens(lens);
        else {
            uint32_t kraft[2];
            bool eob = false;
            if (!read_dynamic(b, lens, false, kraft, &eob) || !eob) { status = b.over() ? kSegEnd : kSegData; break; }
        }
        if (!build_table(lens, 288, kLitBits, lit, kLitCap, 0) || !build_table(lens + 288, 32, kDistBits, dist, kDistCap, 1)) {
            status = kSegData;
            break;
        }
        // the symbol loop of one block; each pass consumes at least one bit, so it ends within the input
        for (;;) {
            if (b.cnt < 48) b.refill();
            if (b.over()) { status = kSegEnd; break; }
            uint32_t e = lit[b.buf & ((1u << kLitBits) - 1)];
            if (e & kSub) {
                b.drop(kLitBits);
                e = lit[((e >> kValShift) + (uint32_t)(b.buf & ((1ull << (e & 0xFF)) - 1))) % kLitCap];
            }
            if (e & kInvalid) { status = kSegData; break; }
            b.drop((int)(e & 0xFF));
            if (e & kLiteral) {
                if (o < cap) sym[o] = (uint16_t)(e >> kValShift);
                ++o;
                continue;
            }
            if (e & kEnd) break;
            const int le = (int)((e >> kExtraShift) & 15u);
            const uint32_t len = (e >> kValShift) + (uint32_t)(b.buf & ((1ull << le) - 1));
            b.drop(le);
            if (b.cnt < 32) b.refill();
            uint32_t d = dist[b.buf & ((1u << kDistBits) - 1)];
            if (d & kSub) {
                b.drop(kDistBits);
                d = dist[((d >> kValShift) + (uint32_t)(b.buf & ((1ull << (d & 0xFF)) - 1))) % kDistCap];
            }
            if (!(d & kBase)) { status = kSegData; break; }
            b.drop((int)(d & 0xFF));
            const int de = (int)((d >> kExtraShift) & 15u);
            const uint32_t distance = (d >> kValShift) + (uint32_t)(b.buf & ((1ull << de) - 1));
            b.drop(de);
            if ((uint64_t)distance > o + hist) { status = kSegData; break; }
            for (uint32_t i = 0; i < len; ++i, ++o) {
                if (o >= cap) { o += len - i; break; }
                sym[o] = o >= distance ? sym[o - distance] : (uint16_t)(kMarker | (uint32_t)(kWin + o - distance));
            }
        }
        if (status != kSegOk) break;
    }
    if (status == kSegOk && b.over()) status = kSegEnd;
    res->stop_bit = b.pos();
    res->n_sym = o;
    res->status = status;
    res->final_block = final_block;
}

// ---- resolution: symbol -> byte; markers read the output in front of the segment (never before `floor`) ----
MHX_HD bool resolve_symbol(uint16_t s, const uint8_t *out, uint64_t seg_out, uint64_t floor, uint8_t *dst)
{
    if (!(s & kMarker)) { *dst = (uint8_t)s; return true; }
    const uint64_t w = s & 0x7FFFu;
    if (seg_out + w < floor + kWin) return false; // would read in front of the member
    *dst = out[seg_out + w - kWin];
    return true;
}

// ---- CRC-32 (gzip polynomial), table driven ----
MHX_HD void crc_table(uint32_t *t)
{
    for (uint32_t i = 0; i < 256; ++i) {
        uint32_t c = i;
        for (int k = 0; k < 8; ++k) c = c & 1 ? 0xEDB88320u ^ (c >> 1) : c >> 1;
        t[i] = c;
    }
}
MHX_HD uint32_t crc_update(const uint32_t *t, uint32_t crc, const uint8_t *p, uint64_t n)
{
    uint32_t c = ~crc;
    for (uint64_t i = 0; i < n; ++i) c = t[(c ^ p[i]) & 0xFF] ^ (c >> 8);
    return ~c;
}

// ---- host side: the gzip member header and the round driver, shared by the HIP host code and the emulator ----

// Offset of the DEFLATE data of the member at in[0], 0 when there is no member there (fewer than 18 bytes or no gzip magic:
// the host decoder ends there too), -1 for a member header the host decoder refuses.
inline int64_t member_data_offset(const uint8_t *in, size_t n)
{
    if (n < 18 || in[0] != 0x1f || in[1] != 0x8b) return 0;
    if (in[2] != 8) return -1;
    const uint8_t flg = in[3];
    size_t p = 10;
    if (flg & 4) {
        if (n - p < 2) return -1;
        const size_t xlen = in[p] | (in[p + 1] << 8);
        p += 2;
        if (n - p < xlen) return -1;
        p += xlen;
    }
    for (int bit = 8; bit <= 16; bit <<= 1) {
        if (!(flg & bit)) continue;
        const void *z = memchr(in + p, 0, n - p);
        if (!z) return -1;
        p = (size_t)((const uint8_t *)z - in) + 1;
    }
    if (flg & 2) { if (n - p < 2) return -1; p += 2; }
    return (int64_t)p;
}

// Is the member at in[0] a BGZF block (bgzip: FEXTRA with a 'BC' subfield announcing the block size)?
inline bool member_is_bgzf(const uint8_t *in, size_t n)
{
    if (n < 18 || in[0] != 0x1f || in[1] != 0x8b || in[2] != 8 || !(in[3] & 4)) return false;
    const size_t xlen = in[10] | (in[11] << 8);
    if (n < 12 + xlen) return false;
    for (size_t p = 12; p + 4 <= 12 + xlen;) {
        const size_t slen = in[p + 2] | (in[p + 3] << 8);
        if (in[p] == 'B' && in[p + 1] == 'C' && slen == 2) return true;
        p += 4 + slen;
    }
    return false;
}

// What the driver asks of a backend (the kernels, or the emulator):
//   search(targets, ntargets, limit_bit, cands)   cands[i] = first candidate in [targets[i], targets[i+1] or limit_bit),
//                                                  kNoBit if none
//   slabs(nseg, cap)                               room for nseg symbol slabs of cap symbols (contents may be lost)
//   decode(idx, nidx, starts, stops, window, res)  decodes slab slots idx[..] (slot j: starts[j], stops[j], window[j])
//   out_room(n)                                    the output holds n bytes from its start (contents kept); false: no room
//   resolve(nseg, n_sym, out_off, floor)           slot j -> out[out_off[j], + n_sym[j]); false: a marker in front of floor
//   crc(nseg, n_sym, out_off, crcs)                CRC-32 of every slot's output
struct MemberStats {
    uint64_t segments = 0, redone = 0, hops = 0, out_bytes = 0;
};
enum MemberStatus { kMemberOk = 0, kMemberFail = 1 };
struct MemberOut {
    uint64_t end_bit = 0; // bit after the final block
    uint64_t out_n = 0;
    uint32_t crc = 0;
};
using CrcCombine = uint32_t (*)(uint32_t, uint32_t, long);

// Rounds: the first covers first_segs targets, every further one twice as many, up to max_segs -- the search and the
// decode of a round reach no further than its own targets, so a small member costs one small round, not a walk over
// everything behind it in the buffer.
template <class Backend>
int inflate_member(Backend &be, uint64_t n_bytes, uint64_t start_bit, uint64_t seg_bits, uint32_t first_segs, uint32_t max_segs,
                   uint64_t out_base, CrcCombine combine, MemberOut *mo, MemberStats *st)
{
    const uint64_t limit = n_bytes * 8;
    uint64_t cap = std::max<uint64_t>(seg_bits / 8 * 8, 1u << 16); // symbols per slab: 8x the target size to start with
    uint64_t cur = start_bit, out_pos = out_base;
    uint32_t crc = 0;
    bool first_round = true;
    uint64_t round_n = std::max<uint32_t>(1, std::min(first_segs, max_segs));
    std::vector<uint64_t> targets, cands, s, stop;
    std::vector<uint8_t> win;
    std::vector<SegResult> res;
    std::vector<uint32_t> idx;
    for (;;) {
        // this round's targets: cur + k seg_bits, k = 1 .. round_n - 1; its last segment stops at the first block boundary
        // at or past round_end (or runs to the final block when the input ends before that)
        const uint64_t round_end = round_n * seg_bits < limit - std::min(limit, cur) ? cur + round_n * seg_bits : kNoBit;
        targets.clear();
        for (uint64_t k = 1; k < round_n && cur + k * seg_bits < limit; ++k) targets.push_back(cur + k * seg_bits);
        cands.assign(targets.size(), kNoBit);
        if (!targets.empty() && !be.search(targets.data(), targets.size(), std::min(round_end, limit), cands.data())) return kMemberFail;
        s.assign(1, cur);
        for (uint64_t c : cands)
            if (c != kNoBit && c > s.back()) s.push_back(c);
        const size_t m = s.size();
        stop.resize(m);
        win.resize(m);
        for (size_t j = 0; j < m; ++j) {
            stop[j] = j + 1 < m ? s[j + 1] : round_end;
            win[j] = !(first_round && j == 0);
        }
        if (!be.slabs(m, cap)) return kMemberFail;
        res.assign(m, SegResult{0, 0, 0, 0});
        idx.resize(m);
        for (size_t j = 0; j < m; ++j) idx[j] = (uint32_t)j;
        st->segments += m;
        size_t last = m; // index of the final segment of the round (m: the round ends without a final block)
        for (int pass = 0;; ++pass) {
            if (pass > kMaxPasses) return kMemberFail;
            if (!idx.empty() && !be.decode(idx.data(), idx.size(), s.data(), stop.data(), win.data(), res.data())) return kMemberFail;
            // the verified prefix
            size_t v = 0;
            uint64_t need_cap = 0;
            last = m;
            for (; v < m; ++v) {
                if (v > 0 && res[v - 1].stop_bit != s[v]) break;
                if (res[v].status != kSegOk) break;
                if (res[v].n_sym > cap) need_cap = std::max(need_cap, res[v].n_sym);
                if (res[v].final_block) { last = v; break; }
            }
            if (last < m || v == m) {
                if (need_cap) { // a verified segment overflowed its slab: larger slabs, the round again
                    cap = need_cap + need_cap / 8;
                    if (!be.slabs(m, cap)) return kMemberFail;
                    idx.resize(m);
                    for (size_t j = 0; j < m; ++j) idx[j] = (uint32_t)j;
                    continue;
                }
                break;
            }
            if (v == 0 || (res[v - 1].stop_bit == s[v] && res[v].status != kSegOk)) return kMemberFail; // a true error
            // redo every segment whose link is broken, from where its predecessor stopped
            idx.clear();
            for (size_t j = v; j < m; ++j) {
                if (res[j - 1].stop_bit != s[j] || res[j].status != kSegOk) {
                    if (res[j - 1].status != kSegOk && j > v) continue; // its predecessor is redone first
                    s[j] = res[j - 1].stop_bit;
                    idx.push_back((uint32_t)j);
                }
            }
            st->redone += idx.size();
        }
        const size_t used = last < m ? last + 1 : m;
        std::vector<uint64_t> nsym(used), off(used);
        uint64_t total = out_pos;
        for (size_t j = 0; j < used; ++j) { nsym[j] = res[j].n_sym; off[j] = total; total += nsym[j]; }
        if (!be.out_room(total)) return kMemberFail;
        if (!be.resolve(used, nsym.data(), off.data(), out_base)) return kMemberFail;
        st->hops += used;
        std::vector<uint32_t> crcs(used);
        if (!be.crc(used, nsym.data(), off.data(), crcs.data())) return kMemberFail;
        for (size_t j = 0; j < used; ++j) crc = combine(crc, crcs[j], (long)nsym[j]);
        out_pos = total;
        cur = res[used - 1].stop_bit;
        first_round = false;
        if (last < m) break;
        if (round_end == kNoBit || cur < round_end) return kMemberFail; // cannot happen for a verified round: no progress
        round_n = std::min<uint64_t>(round_n * 2, max_segs);
    }
    mo->end_bit = cur;
    mo->out_n = out_pos - out_base;
    mo->crc = crc;
    st->out_bytes += mo->out_n;
    return kMemberOk;
}

} // namespace dinf
} // namespace mhx
