// mhx_fasta.h -- the arithmetic of the device FASTA parser as host+device inline functions: mhx_fasta.hip strings them
// together with the wave shuffles, the barriers and the launches; the CPU emulator (tests/emul/fasta_emul.cpp) runs the
// very same functions thread by thread, so that the bit logic, the chunk and tile edges and the partition of the offsets
// pass are checked without a GPU (the rule they must meet is stated line by line in tests/fasta_rule.py).
//
// One thread owns a chunk of 64 bytes and holds what it knows about them as 64-bit masks (ChunkMasks); 256 chunks make a
// tile of 16 KiB.  A chunk cannot know whether its first bytes belong to a header or to a sequence line when no line
// starts in front of them inside the tile, so every count is kept for either state (kSeq / kHdr) until the offsets pass
// has walked the tiles' end states in order.
#pragma once
#include <stdint.h>
#include <string.h>

#include "mhx_hd.h"
#include "mhx_tile.h"

namespace mhx {

constexpr int kFaThreads = 256;
constexpr int kFaBytesPerThread = 64;
constexpr int kFaTile = kFaThreads * kFaBytesPerThread; // 16 KiB
constexpr int kFaOffsetThreads = 1024;                  // the one workgroup of the offsets pass

// state of the line that is open at some point of the stream
enum : uint32_t { kPass = 0, kSeq = 1, kHdr = 2 };
MHX_HD uint32_t combine(uint32_t a, uint32_t b) { return b != kPass ? b : a; }

struct ChunkMasks {
    uint64_t in;    // bytes inside the file
    uint64_t nl;    // newline bytes
    uint64_t keepc; // bytes a sequence line keeps (> ' ' and not DEL)
    uint64_t ls;    // line starts: the previous byte is a newline (or the file begins here)
    uint64_t gt;    // '>' bytes
    uint64_t fq;    // '@' or '+' bytes
};

MHX_HD uint64_t byte_eq_mask64(const uint32_t (&d)[16], uint32_t pattern)
{
    uint64_t m = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) m |= (uint64_t)flags_to_nibble(zero_byte_flags(d[i] ^ pattern)) << (4 * i);
    return m;
}

// masks of the 64 bytes at file offset `off` (the caller guarantees 16-byte alignment of base; readable are the 16-byte
// pieces of [0, n rounded up to 16))
MHX_HD ChunkMasks load_chunk(const uint8_t *base, uint64_t off, uint64_t n, uint32_t (&d)[16])
{
    ChunkMasks c;
    const uint64_t lim = (n + 15) & ~(uint64_t)15;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        uint4 v = {0, 0, 0, 0};
#if defined(__HIP_DEVICE_COMPILE__)
        if (off + 16u * j < lim) v = *reinterpret_cast<const uint4 *>(base + off + 16u * j);
#else
        if (off + 16u * j < lim) memcpy(&v, base + off + 16u * j, 16);
#endif
        d[4 * j] = v.x; d[4 * j + 1] = v.y; d[4 * j + 2] = v.z; d[4 * j + 3] = v.w;
    }
    c.in = off >= n ? 0ull : (n - off >= 64 ? ~0ull : ((1ull << (n - off)) - 1ull));
    c.nl = byte_eq_mask64(d, 0x0A0A0A0Au) & c.in;
    c.gt = byte_eq_mask64(d, 0x3E3E3E3Eu) & c.in;
    c.fq = (byte_eq_mask64(d, 0x40404040u) | byte_eq_mask64(d, 0x2B2B2B2Bu)) & c.in;
    // kept by a sequence line: byte > 0x20 and != 0x7F.  byte > 0x20  <=>  (byte & 0xE0) != 0 and byte != 0x20
    uint64_t low = 0, del = 0, sp = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        low |= (uint64_t)flags_to_nibble(zero_byte_flags(d[i] & 0xE0E0E0E0u)) << (4 * i); // byte < 0x20
        sp |= (uint64_t)flags_to_nibble(zero_byte_flags(d[i] ^ 0x20202020u)) << (4 * i);
        del |= (uint64_t)flags_to_nibble(zero_byte_flags(d[i] ^ 0x7F7F7F7Fu)) << (4 * i);
    }
    c.keepc = ~(low | sp | del) & c.in;
    const bool prev_nl = off == 0 ? true : (off <= n && base[off - 1] == '\n');
    c.ls = ((c.nl << 1) | (prev_nl ? 1ull : 0ull)) & c.in;
    return c;
}

// header-line bytes of a chunk whose first byte belongs to a line in state `in_state` (kSeq / kHdr)
MHX_HD uint64_t header_mask(const ChunkMasks &c, uint32_t in_state)
{
    uint64_t hdr = 0, rest = c.ls;
    uint64_t from = 0; // start of the current segment (bit index)
    bool cur = in_state == kHdr;
    while (rest) {
        const int q = __builtin_ctzll(rest);
        if (cur && q > (int)from) hdr |= ((q >= 64 ? 0ull : (1ull << q)) - 1ull) & ~((1ull << from) - 1ull);
        cur = (c.gt >> q) & 1ull;
        from = (uint64_t)q;
        rest &= rest - 1ull;
    }
    if (cur) hdr |= ~((1ull << from) - 1ull);
    return hdr & c.in;
}

// state of the line open at the end of the chunk, kPass if no line starts inside it
MHX_HD uint32_t chunk_state(const ChunkMasks &c)
{
    if (!c.ls) return kPass;
    const int q = 63 - __builtin_clzll(c.ls);
    return ((c.gt >> q) & 1ull) ? kHdr : kSeq;
}

// bytes of the chunk that go to the output for a given start state: the sequence-line bytes that are not blank, and the
// newline that ends a header line
MHX_HD uint64_t kept_mask(const ChunkMasks &c, uint32_t in_state)
{
    const uint64_t hdr = header_mask(c, in_state);
    return (~hdr & c.keepc) | (hdr & c.nl);
}

// ---- the offsets pass: thread t of kFaOffsetThreads owns the tiles [lo, hi) --------------------------------------
// summary[3 i ..]: tile i's end state (kPass: no line starts inside), its kept bytes if it starts inside a sequence line,
// its kept bytes if it starts inside a header line.
struct FaSpan { uint32_t lo, hi; };
MHX_HD uint32_t fa_min(uint32_t a, uint32_t b) { return a < b ? a : b; }
MHX_HD FaSpan fa_span(uint32_t t, uint32_t ntiles)
{
    const uint32_t per = (ntiles + kFaOffsetThreads - 1) / kFaOffsetThreads;
    FaSpan sp;
    sp.lo = fa_min(t * per, ntiles);
    sp.hi = fa_min(sp.lo + per, ntiles);
    return sp;
}
// the state a thread's tiles leave behind them (kPass: none of them holds a line start)
MHX_HD uint32_t fa_span_state(const uint32_t *summary, FaSpan sp)
{
    uint32_t s = kPass;
    for (uint32_t i = sp.lo; i < sp.hi; ++i) s = combine(s, summary[3 * i]);
    return s;
}
// The state in front of thread t's first tile, from the threads' partials st[0, t).  The file starts with a header line
// ('>' checked by the host), so the stream state in front of tile 0 is irrelevant: tile 0 has a line start at byte 0.
// Serial combine over up to 1024 partials by every thread (1024 LDS reads, cheap enough).
MHX_HD uint32_t fa_state_before(const uint32_t *st, uint32_t t)
{
    uint32_t in = kSeq;
    for (uint32_t i = 0; i < t; ++i) in = combine(in, st[i]);
    return in;
}
MHX_HD uint32_t fa_tile_kept(const uint32_t *summary, uint32_t i, uint32_t state) { return state == kHdr ? summary[3 * i + 2] : summary[3 * i + 1]; }
// first walk over a thread's tiles: the state every tile starts in; returns the bytes they keep
MHX_HD unsigned long long fa_walk_states(const uint32_t *summary, FaSpan sp, uint32_t in, uint32_t *tile_in)
{
    unsigned long long sum = 0;
    uint32_t cur = in;
    for (uint32_t i = sp.lo; i < sp.hi; ++i) {
        tile_in[i] = cur;
        sum += fa_tile_kept(summary, i, cur);
        cur = combine(cur, summary[3 * i]);
    }
    return sum;
}
// second walk: every tile's first output byte, `before` being the bytes kept in front of the thread's first tile; returns
// the bytes kept in front of the tile behind its last one
MHX_HD unsigned long long fa_walk_offsets(const uint32_t *summary, FaSpan sp, uint32_t in, unsigned long long before, uint64_t *tile_off)
{
    uint32_t cur = in;
    for (uint32_t i = sp.lo; i < sp.hi; ++i) {
        tile_off[i] = before;
        before += fa_tile_kept(summary, i, cur);
        cur = combine(cur, summary[3 * i]);
    }
    return before;
}

} // namespace mhx
