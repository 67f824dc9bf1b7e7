// mhx_deflate.h -- the DEFLATE (RFC 1951) and gzip (RFC 1952) formats, written once for the three decoders of libmhx:
// the sequential GzInflater (mhx_inflate.cpp), the multi-threaded ParallelGunzip / BgzfReader (mhx_pinflate.cpp) and
// the device decoder (mhx_dinflate.h / mhx_dinflate.hip and its CPU emulator).  Here: the decode-table layout, the
// length/distance tables, the two-level Huffman table builder, the fixed code, the dynamic block header, the gzip member
// header, the BGZF block size and the CRC-32 table.  The symbol loops stay with their decoders: the host's runs on padded
// input without index checks, the device's checks every read and index.  Internal to libmhx.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "mhx_hd.h"

namespace mhx {
namespace deflate {

constexpr int kLitBits = 11, kDistBits = 8; // index bits of the first-level tables
constexpr int kLitCap = (1 << kLitBits) + 288 * 16, kDistCap = (1 << kDistBits) + 32 * 128; // entries, sub-tables included
constexpr int kLensBytes = 288 + 32;        // code lengths: literal/length at [0, 288), distance at [288, 320)

// Table entries: bits 0..7 = bits to consume (or index bits of the sub-table), bit 8 literal, bit 9 end of block, bit 10
// sub-table link, bit 11 invalid, bit 12 length / distance base; bits 13..16 = number of extra bits that follow the code;
// bits 17..31 = the literal, the base length, the base distance or the sub-table offset.
constexpr uint32_t kKindLiteral = 0x0100, kKindEnd = 0x0200, kKindSub = 0x0400, kKindInvalid = 0x0800, kKindBase = 0x1000;
constexpr int kValShift = 17, kExtraShift = 13;

struct Tables {
    uint32_t lit[kLitCap];
    uint32_t dist[kDistCap];
};

// RFC 1951 3.2.5 and 3.2.7; the tables live inside the functions, which keeps them out of scratch on the device
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

// ---- decode tables ----
enum TableKind { kLitLenTable = 0, kDistTable = 1 };
MHX_HD uint32_t payload(int kind, int s) // bits 8..31 of the entries of symbol s
{
    if (kind == kLitLenTable) {
        if (s < 256) return kKindLiteral | ((uint32_t)s << kValShift);
        if (s == 256) return kKindEnd;
        if (s > 285) return kKindInvalid;
        return kKindBase | (len_base(s - 257) << kValShift) | (len_extra(s - 257) << kExtraShift);
    }
    if (s > 29) return kKindInvalid;
    return kKindBase | (dist_base(s) << kValShift) | (dist_extra(s) << kExtraShift);
}

// Builds the two-level decode table of a canonical Huffman code (first_bits index bits, sub-tables behind them, cap
// entries in all).  Returns false for an over-subscribed code or a table overflow; incomplete codes are legal (unused
// slots decode as invalid).
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
    for (int i = 0; i < first_size; ++i) table[i] = kKindInvalid | 1u; // consume one bit, report invalid
    int sub_next = first_size;
    const int sub_bits = max_len > first_bits ? max_len - first_bits : 0;
    for (int sym = 0; sym < nsym; ++sym) {
        const int l = lens[sym] & 15;
        if (!l) continue;
        const uint32_t c = next_code[l]++;
        uint32_t r = 0; // the code, bit-reversed: DEFLATE sends Huffman codes most significant bit first
        for (int i = 0; i < l; ++i) r |= ((c >> i) & 1u) << (l - 1 - i);
        if (l <= first_bits) {
            const uint32_t e = payload(kind, sym) | (uint32_t)l;
            for (uint32_t i = r; i < (uint32_t)first_size; i += 1u << l) table[i] = e;
        } else {
            const uint32_t lo = r & (uint32_t)(first_size - 1);
            uint32_t head = table[lo];
            if (!(head & kKindSub)) { // open a sub-table for this prefix
                if (sub_next + (1 << sub_bits) > cap) return false;
                head = kKindSub | (uint32_t)sub_bits | ((uint32_t)sub_next << kValShift);
                table[lo] = head;
                for (int i = 0; i < (1 << sub_bits); ++i) table[sub_next + i] = kKindInvalid | 1u;
                sub_next += 1 << sub_bits;
            }
            const uint32_t base = head >> kValShift;
            const uint32_t e = payload(kind, sym) | (uint32_t)(l - first_bits);
            for (uint32_t i = r >> first_bits; i < (1u << sub_bits); i += 1u << (l - first_bits)) table[base + i] = e;
        }
    }
    return true;
}

MHX_HD void fixed_lens(uint8_t *lens) // the code of a fixed-Huffman block, in the layout of kLensBytes
{
    for (int i = 0; i < 288; ++i) lens[i] = (uint8_t)(i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : 8);
    for (int i = 0; i < 32; ++i) lens[288 + i] = 5;
}

// ---- the dynamic block header ----

// The code-length code (19 symbols, 7 bits at most), decoded bit by bit from the counts per length: it is read once per
// block header, and the counts fit in registers where a table would not.
struct ClenCode {
    uint8_t count[8];
    uint8_t sym[19];
};
// false: over-subscribed; *complete: the Kraft sum is exactly 1
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
// symbol, or -1 when no code of <= 7 bits matches (an incomplete code); needs 7 bits buffered
template <class R>
MHX_HD int clen_decode(R &b, const ClenCode &c)
{
    const uint32_t bits = b.peek(7);
    int code = 0, first = 0, index = 0;
    for (int l = 1; l < 8; ++l) {
        code |= (int)((bits >> (l - 1)) & 1u);
        const int count = c.count[l];
        if (code - count < first) {
            b.drop(l);
            return c.sym[(index + (code - first)) % 19];
        }
        index += count;
        first += count;
        first <<= 1;
        code <<= 1;
    }
    return -1;
}

// read_dynamic's verdicts, in the order its checks come (zlib's order: mhx_inflate_impl.h maps each to zlib's text)
enum HeaderStatus {
    kHeaderOk = 0,
    kHeaderEnd,            // the header runs past the input
    kHeaderTooMany,        // HLIT > 29 or HDIST > 29
    kHeaderClenSet,        // over-subscribed code-length code
    kHeaderClenIncomplete, // incomplete code-length code (strict mode only)
    kHeaderClenCode,       // a code-length code that the code does not hold
    kHeaderRepeat,         // a repeat with nothing to repeat, or past the last length
    kHeaderNoEnd,          // no code for the end-of-block symbol
};

// Reads HLIT/HDIST/HCLEN, the code-length code and the run-length coded code lengths of a dynamic block (the three bits
// in front are read).  lens (kLensBytes) receives the code lengths when non-null; kraft[0] / [1] (when non-null) the Kraft
// sums, in units of 2^-15, of the literal/length and the distance code.  strict: an incomplete code-length code is refused
// as well (every encoder writes a complete one: the block search).  The reader R has peek/drop, overrun() (a bit past the
// input has been consumed) and fill(k): refill when fewer than k bits are buffered; false when the reader may not refill
// any more (the host reader, whose refills read no further than its pad behind the input).  Every read below is of bits
// that a fill() has buffered.
template <class R>
MHX_HD int read_dynamic(R &b, uint8_t *lens, bool strict, uint32_t *kraft)
{
    auto bits = [&b](int k) {
        const uint32_t v = b.peek(k);
        b.drop(k);
        return (int)v;
    };
    if (!b.fill(14)) return kHeaderEnd;
    const int nlit = bits(5) + 257, ndist = bits(5) + 1, nclen = bits(4) + 4;
    if (nlit > 286 || ndist > 30) return kHeaderTooMany;
    uint8_t cl[19];
    for (int i = 0; i < 19; ++i) cl[i] = 0;
    for (int i = 0; i < nclen; ++i) {
        if (!b.fill(3)) return kHeaderEnd;
        cl[clen_order(i)] = (uint8_t)bits(3);
    }
    if (b.overrun()) return kHeaderEnd;
    ClenCode cc;
    bool complete = false;
    if (!clen_build(cl, cc, &complete)) return kHeaderClenSet;
    if (strict && !complete) return kHeaderClenIncomplete;
    uint32_t k0 = 0, k1 = 0;
    int prev = 0;
    bool has_eob = false;
    int i = 0;
    while (i < nlit + ndist) {
        if (!b.fill(14) || b.overrun()) return kHeaderEnd; // a code and its repeat bits: 14 bits at most
        const int sym = clen_decode(b, cc);
        if (sym < 0) return kHeaderClenCode;
        int rep = 1, val = sym;
        if (sym == 16) {
            if (i == 0) return kHeaderRepeat;
            val = prev;
            rep = 3 + bits(2);
        } else if (sym == 17) { val = 0; rep = 3 + bits(3); }
        else if (sym == 18) { val = 0; rep = 11 + bits(7); }
        if (i + rep > nlit + ndist) return kHeaderRepeat;
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
    if (kraft) {
        kraft[0] = k0;
        kraft[1] = k1;
    }
    return has_eob ? kHeaderOk : kHeaderNoEnd;
}

// ---- gzip and BGZF framing (host only) ----

// What the bytes in[0, n) start with: kGzNone -- no member (fewer than 18 bytes, or no gzip magic: the decoders stop
// there and ignore the rest, as gzread does), kGzMethod -- a compression method other than DEFLATE, kGzTruncated --
// FEXTRA, FNAME, FCOMMENT or FHCRC runs past the input; otherwise the offset of the member's DEFLATE data (10..n).
enum : int64_t { kGzNone = 0, kGzMethod = -1, kGzTruncated = -2 };
inline int64_t gzip_member(const uint8_t *in, size_t n)
{
    if (n < 18 || in[0] != 0x1f || in[1] != 0x8b) return kGzNone;
    if (in[2] != 8) return kGzMethod;
    const uint8_t flg = in[3];
    size_t p = 10;
    if (flg & 4) { // FEXTRA
        if (n - p < 2) return kGzTruncated;
        const size_t xlen = in[p] | (in[p + 1] << 8);
        p += 2;
        if (n - p < xlen) return kGzTruncated;
        p += xlen;
    }
    for (int bit = 8; bit <= 16; bit <<= 1) { // FNAME, FCOMMENT: zero-terminated
        if (!(flg & bit)) continue;
        const void *z = memchr(in + p, 0, n - p);
        if (!z) return kGzTruncated;
        p = (size_t)((const uint8_t *)z - in) + 1;
    }
    if (flg & 2) { // FHCRC
        if (n - p < 2) return kGzTruncated;
        p += 2;
    }
    return (int64_t)p;
}

// Size of the BGZF block at in[0, n) -- a gzip member whose FEXTRA holds the subfield 'B','C' with the block's size less
// one (bgzip) -- or 0 when there is none, or its size does not fit the header and the input.
inline uint32_t bgzf_block_size(const uint8_t *in, size_t n)
{
    if (n < 28 || in[0] != 0x1f || in[1] != 0x8b || in[2] != 8 || !(in[3] & 4)) return 0;
    const uint32_t xlen = in[10] | (in[11] << 8);
    if (n < 12 + (size_t)xlen) return 0;
    for (uint32_t p = 0; p + 4 <= xlen;) {
        const uint8_t *f = in + 12 + p;
        const uint32_t slen = f[2] | (f[3] << 8);
        if (f[0] == 'B' && f[1] == 'C' && slen == 2 && p + 6 <= xlen) {
            const uint32_t total = (uint32_t)(f[4] | (f[5] << 8)) + 1u;
            return total >= 12 + xlen + 8 && total <= n ? total : 0;
        }
        p += 4 + slen;
    }
    return 0;
}

// ---- CRC-32 of gzip (the bit-reflected IEEE 802.3 polynomial) ----
MHX_HD uint32_t crc_entry(uint32_t i) // entry i of the byte-at-a-time table
{
    uint32_t c = i;
    for (int k = 0; k < 8; ++k) c = c & 1 ? 0xEDB88320u ^ (c >> 1) : c >> 1;
    return c;
}

} // namespace deflate
} // namespace mhx
