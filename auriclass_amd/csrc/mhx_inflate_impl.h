// mhx_inflate_impl.h -- pieces of the host DEFLATE decoder shared by the sequential inflater (mhx_inflate.cpp) and the
// parallel one (mhx_pinflate.cpp): bit reader, block header parsing (on the format core of mhx_deflate.h) and the symbol
// loop.  Internal to libmhx.
#pragma once
#include <stdint.h>
#include <string.h>

#include "mhx_deflate.h"

namespace mhx {
namespace deflate {

// Over-read discipline: the true read position is P = in - (bitcnt >> 3); a refill loads 8 bytes at
// `in` <= P + 7, i.e. touches bytes up to P + 14.  Every refill is preceded (at a distance of at most 2
// consumed bytes) by an overrun() test that pins P <= in_end, so no load reaches past in_end + 17 -- inside
// the GzInflater::kInputPad (64) zero bytes the caller guarantees behind the input.
struct BitReader {
    const uint8_t *in = nullptr, *in_end = nullptr; // in_end excludes the readable pad bytes
    uint64_t bitbuf = 0;
    int bitcnt = 0;
    void refill()
    { // branch-free: valid while 8 bytes at `in` are readable (the buffer is padded)
        uint64_t v;
        memcpy(&v, in, 8);
        bitbuf |= v << bitcnt;
        in += (63 - bitcnt) >> 3;
        bitcnt |= 56;
    }
    uint32_t peek(int n) const { return (uint32_t)(bitbuf & ((1ull << n) - 1)); }
    void drop(int n) { bitbuf >>= n; bitcnt -= n; }
    uint32_t take(int n) { const uint32_t v = peek(n); drop(n); return v; }
    bool overrun() const { return (in - (bitcnt >> 3)) > in_end; }
    bool fill(int n) // read_dynamic's refill: tested first
    {
        if (bitcnt >= n) return true;
        if (overrun()) return false;
        refill();
        return true;
    }
    void byte_align() { drop(bitcnt & 7); }
    // give back whole unread bytes: `in` is then the true position (only meaningful on a byte boundary)
    void unread() { in -= bitcnt >> 3; bitbuf = 0; bitcnt = 0; }
    // absolute bit position of the next unread bit, relative to `base`
    uint64_t bitpos(const uint8_t *base) const { return (uint64_t)(in - base) * 8 - (uint64_t)bitcnt; }
    void seek(const uint8_t *base, uint64_t bit)
    {
        in = base + (bit >> 3);
        bitbuf = 0;
        bitcnt = 0;
        refill();
        drop((int)(bit & 7));
    }
};

// zlib's text for a status of read_dynamic
inline const char *header_error(int status)
{
    switch (status) {
    case kHeaderEnd: return "unexpected end of deflate stream";
    case kHeaderTooMany: return "too many length or distance symbols";
    case kHeaderClenSet:
    case kHeaderClenIncomplete: return "invalid code lengths set";
    case kHeaderClenCode: return "invalid code length code";
    case kHeaderRepeat: return "invalid bit length repeat";
    default: return "invalid code -- missing end-of-block";
    }
}

// Parses one block header at the reader's position.  type 0: stored block, *stored_len bytes follow (the reader is left
// byte-aligned, bits buffered); types 1/2: the tables are built.  Returns nullptr or the error text (zlib's wording).
inline const char *read_block_header(BitReader &r, Tables &t, bool *last_block, uint32_t *stored_len, uint32_t *type_out)
{
    r.refill();
    *last_block = r.take(1) != 0;
    const uint32_t type = r.take(2);
    *type_out = type;
    if (type == 0) {
        r.byte_align();
        if (r.overrun()) return "unexpected end of deflate stream";
        r.refill();
        const uint32_t len = r.take(16), nlen = r.take(16);
        // LEN/NLEN must lie inside the input: read from the zero pad they would pass the check as 0xFFFF/0x0000
        if (r.overrun()) return "unexpected end of deflate stream";
        if ((len ^ nlen) != 0xFFFFu) return "stored block length check failed";
        *stored_len = len;
        return nullptr;
    }
    uint8_t lens[kLensBytes];
    if (type == 1) fixed_lens(lens);
    else if (type == 2) {
        const int status = read_dynamic(r, lens, false, nullptr);
        if (status != kHeaderOk) return header_error(status);
    } else {
        return "invalid block type";
    }
    if (!build_table(lens, 288, kLitBits, t.lit, kLitCap, kLitLenTable)) return "invalid literal/lengths set";
    if (!build_table(lens + 288, 32, kDistBits, t.dist, kDistCap, kDistTable)) return "invalid distances set";
    return nullptr;
}

// The symbol loop of a Huffman block, on output elements of type T: uint8_t for the plain decoder, uint16_t for the
// parallel decoder's symbolic pass (bytes, or markers >= 0x8000 that stand for bytes of the not yet known 32 KiB in front
// of a segment).  Decodes until `o_limit` is reached (may overshoot by < 320 elements), the block ends or an error occurs.
// [window_start, o) is the output so far (a match may reach back 32 KiB into it).
enum BlockStatus { kBlockEnd, kBlockLimit, kBlockError };
template <class T>
inline BlockStatus huffman_block(BitReader &r, const Tables &t, T *&o_ref, T *const o_limit, const T *window_start, const char **err_out)
{
    // the decoder state lives in locals inside the loop: stores through `o` may alias
    // anything reachable through the reader, which would force a reload after every literal
    const uint32_t *const lit = t.lit, *const dist = t.dist;
    const uint8_t *in = r.in;
    const uint8_t *const in_end = r.in_end;
    uint64_t bitbuf = r.bitbuf;
    int bitcnt = r.bitcnt;
    T *o = o_ref;
    const char *err = nullptr;
    bool end_of_block = false;
#define MHX_REFILL()                                                                         \
    do {                                                                                     \
        uint64_t v_;                                                                         \
        memcpy(&v_, in, 8);                                                                  \
        bitbuf |= v_ << bitcnt;                                                              \
        in += (63 - bitcnt) >> 3;                                                            \
        bitcnt |= 56;                                                                        \
    } while (0)
#define MHX_DROP(n) do { const int n_ = (int)(n); bitbuf >>= n_; bitcnt -= n_; } while (0)
    while (o < o_limit) {
        MHX_REFILL();
        if (in - (bitcnt >> 3) > in_end) { err = "unexpected end of deflate stream"; break; }
        uint32_t e = lit[bitbuf & ((1u << kLitBits) - 1)];
        if (e & kKindSub) {
            MHX_DROP(kLitBits);
            e = lit[(e >> kValShift) + (uint32_t)(bitbuf & ((1ull << (e & 0xFF)) - 1))];
        }
        MHX_DROP(e & 0xFF);
        if (e & kKindLiteral) {
            *o++ = (T)(e >> kValShift);
            // a second and third literal usually fit the bits already buffered
            e = lit[bitbuf & ((1u << kLitBits) - 1)];
            if ((e & (kKindLiteral | kKindSub)) == kKindLiteral) {
                MHX_DROP(e & 0xFF);
                *o++ = (T)(e >> kValShift);
                e = lit[bitbuf & ((1u << kLitBits) - 1)];
                if ((e & (kKindLiteral | kKindSub)) == kKindLiteral) {
                    MHX_DROP(e & 0xFF);
                    *o++ = (T)(e >> kValShift);
                }
            }
            continue;
        }
        if (e & kKindBase) {
            const int le = (int)((e >> kExtraShift) & 15u);
            const uint32_t len = (e >> kValShift) + (uint32_t)(bitbuf & ((1ull << le) - 1));
            MHX_DROP(le);
            if (bitcnt < 32) MHX_REFILL();
            uint32_t d = dist[bitbuf & ((1u << kDistBits) - 1)];
            if (d & kKindSub) {
                MHX_DROP(kDistBits);
                d = dist[(d >> kValShift) + (uint32_t)(bitbuf & ((1ull << (d & 0xFF)) - 1))];
            }
            if (!(d & kKindBase)) { err = "invalid distance code"; break; }
            MHX_DROP(d & 0xFF);
            const int de = (int)((d >> kExtraShift) & 15u);
            const uint32_t distance = (d >> kValShift) + (uint32_t)(bitbuf & ((1ull << de) - 1));
            MHX_DROP(de);
            if ((size_t)(o - window_start) < distance) { err = "invalid distance too far back"; break; }
            const T *src = o - distance;
            T *const end = o + len;
            if (distance * sizeof(T) >= 8) {
                do { memcpy(o, src, 8); o += 8 / sizeof(T); src += 8 / sizeof(T); } while (o < end);
            } else if (distance == 1) {
                const T v = *src;
                for (T *p = o; p < end; ++p) *p = v;
            } else {
                while (o < end) *o++ = *src++;
            }
            o = end;
            continue;
        }
        if (e & kKindEnd) { end_of_block = true; break; }
        err = "invalid literal/length code";
        break;
    }
#undef MHX_REFILL
#undef MHX_DROP
    r.in = in;
    r.bitbuf = bitbuf;
    r.bitcnt = bitcnt;
    o_ref = o;
    if (err) { *err_out = err; return kBlockError; }
    return end_of_block ? kBlockEnd : kBlockLimit;
}

} // namespace deflate
} // namespace mhx
