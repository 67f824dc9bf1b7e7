// mhx_fqcheck.h -- record check of a 4-line FASTQ span against the kseq-style reader (oracle/mashcore.c
// mo_sketch_add_fastx, mirrored by parse_fastx), as host+device inline functions: mhx_fqcheck.hip strings them
// together, the CPU emulator (tests/emul/fqcheck_emul.cpp) runs the very same functions thread by thread.
//
// The sketch kernel checks only that record lines start with '@' and '+'.  A span whose records pass that layout
// check is read by the kseq reader exactly as the device parser reads it when every record is clean:
//   (a) its sequence line holds no byte <= 0x20 and no 0x7F, except one '\r' right before the newline (or the end
//       of the span);
//   (b) its sequence line does not begin with '>', '@' or '+';
//   (c) its quality line holds exactly as many bytes > 0x20 and != 0x7F as the sequence line holds bases.
// A span with a record that is not clean raises kFlagBadFastq; the file-level call then hands the file to the
// record parser, whose verdict is final.  The check may flag more than strictly needed (a span that ends inside a
// record, for one), never less.
//
// How (c) is checked without per-record storage: S(i) = non-blank bytes of sequence lines minus non-blank bytes of
// quality lines in front of byte i.  Every record is balanced iff S is 0 at every record end (the newline that ends a
// quality line) and at the end of the span.  Everything depends on the line index of a byte only mod 4, and a span
// starts at a record start (line 0), so a piece of the span is summarised for each of the four line phases its first
// byte may have: newlines (mod 4), its share of S, whether it holds a record end and the share of S in front of the
// first one, and whether a rule failed inside it.  Summaries compose in order (fq_combine); the span's verdict is the
// phase-0 entry of the summary of all its pieces.  The bytes are read once.
#pragma once
#include <stdint.h>

#include "mhx_hd.h"

namespace mhx {

constexpr int kFqBlock = 256;                       // threads per workgroup
constexpr int kFqBytesPerThread = 128;              // four 32-byte words, contiguous
constexpr int kFqTileBytes = kFqBlock * kFqBytesPerThread; // 32 KiB staged per step
constexpr int kFqTilesPerBlock = 8;                 // steps per workgroup: one summary per 256 KiB
constexpr uint64_t kFqBlockBytes = (uint64_t)kFqTileBytes * kFqTilesPerBlock;

// Summary of a piece of the span, for each phase q (line index mod 4 of the piece's first byte).
template <class I> struct FqSum {
    uint32_t nl;     // newlines in the piece (mod 4)
    uint32_t flags;  // bit q: the piece holds a record end; bit 4 + q: a rule failed inside the piece
    I t[4];          // share of S
    I v[4];          // share of S in front of the first record end (bit q of flags)
};

template <class I> MHX_HD FqSum<I> fq_identity()
{
    FqSum<I> s;
    s.nl = 0; s.flags = 0;
    for (int q = 0; q < 4; ++q) { s.t[q] = 0; s.v[q] = 0; }
    return s;
}

// x[i] by selects: an array in registers indexed at run time would go to scratch memory
template <class J> MHX_HD J fq_pick(const J (&x)[4], int i) { return i == 0 ? x[0] : i == 1 ? x[1] : i == 2 ? x[2] : x[3]; }

// a then b.  All record ends of a piece must see the same S (0 once the prefix is added); b's first one is
// compared with a's.
template <class I, class J> MHX_HD FqSum<I> fq_combine(const FqSum<I> &a, const FqSum<J> &b)
{
    FqSum<I> r;
    r.nl = (a.nl + b.nl) & 3u;
    r.flags = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int q2 = (q + (int)a.nl) & 3;
        const I bt = (I)fq_pick(b.t, q2), bv = (I)fq_pick(b.v, q2);
        const bool ea = (a.flags >> q) & 1u, eb = (b.flags >> q2) & 1u;
        const bool bad = ((a.flags >> (4 + q)) & 1u) || ((b.flags >> (4 + q2)) & 1u) || (ea && eb && a.t[q] + bv != a.v[q]);
        r.t[q] = a.t[q] + bt;
        r.v[q] = ea ? a.v[q] : a.t[q] + bv;
        r.flags |= ((ea || eb) ? 1u : 0u) << q;
        r.flags |= (bad ? 1u : 0u) << (4 + q);
    }
    return r;
}

// the span's verdict: its summary starts at line 0
template <class I> MHX_HD bool fq_span_bad(const FqSum<I> &s)
{
    return ((s.flags >> 4) & 1u) || s.t[0] != 0 || ((s.flags & 1u) && s.v[0] != 0);
}

// ---- bytes -> bit masks (exact per byte: no borrow crosses a byte) -----------------------
MHX_HD uint32_t fq_eq(uint32_t v, uint32_t pattern) // 0x80 in every byte equal to the pattern's
{
    const uint32_t y = v ^ pattern;
    return ~(((y & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | y) & 0x80808080u;
}
// bytes the kseq reader counts: > 0x20 and != 0x7F (unsigned)
MHX_HD uint32_t fq_nonblank(uint32_t v)
{
    const uint32_t ge21 = ((v | 0x80808080u) - 0x21212121u) & 0x80808080u; // low seven bits >= 0x21
    return (v & 0x80808080u) | (ge21 & ~fq_eq(v, 0x7F7F7F7Fu));
}
// the 0x80 flags of two dwords (bytes 0..3, 4..7) -> 8 bits in byte order
MHX_HD uint32_t fq_pack(uint32_t f_lo, uint32_t f_hi) { return (((f_lo >> 4) | f_hi) * 0x00204081u) >> 24; }

MHX_HD uint32_t fq_prefix_xor_excl(uint32_t x)
{
    x ^= x << 1; x ^= x << 2; x ^= x << 4; x ^= x << 8; x ^= x << 16;
    return x << 1;
}

// ---- LDS of one step ---------------------------------------------------------------------
// Chunk c (16 B; c in [0, kFqChunks)) holds the absolute bytes tile_off - 16 + 16 c: the tile with one chunk in front of
// it and one behind it.  Lane t reads chunks 8 t + 1 .. 8 t + 8 (its 128 bytes) with 16-byte reads; one slot of padding
// behind every eight chunks puts the lanes of a 16-lane group on 16 different 16-byte bank groups (a stride of 144 bytes
// instead of 128, which would put them on two).
constexpr int kFqChunks = kFqTileBytes / 16 + 2;
MHX_HD constexpr int fq_slot(int c) { return c + ((c + 7) >> 3); }
constexpr int kFqSlots = fq_slot(kFqChunks - 1) + 1;
struct FqSmem {
    uint4 bytes[kFqSlots];
    FqSum<int32_t> red[kFqBlock];
};
// byte x of the tile (-16 <= x < kFqTileBytes + 16)
MHX_HD uint8_t fq_byte(const FqSmem &sm, int x)
{
    return reinterpret_cast<const uint8_t *>(sm.bytes)[16 * fq_slot((x + 16) >> 4) + ((x + 16) & 15)];
}

// Stage lane tid's chunks of the step at tile_off.  Readable are the 16-byte chunks of [0, lim), lim = end rounded up
// to 16 (as for the sketch kernel); chunks outside are zero.
MHX_HD bool fq_chunk_readable(uint64_t tile_off, int c, uint64_t lim)
{
    const uint64_t at = tile_off + 16u * (uint64_t)c; // + 16: offset of the chunk's end
    return at >= 16u && at - 16u < lim;
}
MHX_HD void fq_stage(FqSmem &sm, int tid, const uint8_t *base, uint64_t tile_off, uint64_t lim)
{
    const uint4 *src = reinterpret_cast<const uint4 *>(base + tile_off - 16u); // (chunk 0; used when readable)
    constexpr int kPer = (kFqChunks - 2) / kFqBlock;
    if (tile_off >= 16u && tile_off + kFqTileBytes + 16u <= lim) { // every chunk readable: all loads before the first LDS write
        uint4 v[kPer];
#pragma unroll
        for (int j = 0; j < kPer; ++j) v[j] = src[j * kFqBlock + tid];
        uint4 h = {0, 0, 0, 0};
        if (tid < 2) h = src[kFqChunks - 2 + tid];
#pragma unroll
        for (int j = 0; j < kPer; ++j) sm.bytes[fq_slot(j * kFqBlock + tid)] = v[j];
        if (tid < 2) sm.bytes[fq_slot(kFqChunks - 2 + tid)] = h;
        return;
    }
    for (int c = tid; c < kFqChunks; c += kFqBlock) {
        uint4 v = {0, 0, 0, 0};
        if (fq_chunk_readable(tile_off, c, lim)) v = src[c];
        sm.bytes[fq_slot(c)] = v;
    }
}

// One 32-byte word at tile byte L: w = its eight dwords, in = bits of its bytes inside the span, prev_start = the byte in
// front of bit 0 is a newline or lies in front of the span, next_end = the byte behind bit 31 is a newline or lies
// behind the span.
MHX_HD FqSum<int32_t> fq_word(const FqSmem &sm, int L, const uint32_t (&w)[8], uint32_t in, bool prev_start, bool next_end)
{
    uint32_t nl = 0, nb = 0;
#pragma unroll
    for (int d = 0; d < 8; d += 2) {
        nl |= fq_pack(fq_eq(w[d], 0x0A0A0A0Au), fq_eq(w[d + 1], 0x0A0A0A0Au)) << (4 * d);
        nb |= fq_pack(fq_nonblank(w[d]), fq_nonblank(w[d + 1])) << (4 * d);
    }
    nl &= in; nb &= in;
    const uint32_t brk = nl | ~in;                                     // a line ends (or the span does) at these bytes
    const uint32_t start = ((brk << 1) | (prev_start ? 1u : 0u)) & in; // first byte of a line
    // the bytes that break rule (a) or (b) if their line is a sequence line.  Blanks are rare, and only line starts
    // can break (b): both are looked at byte by byte.
    uint32_t bad_byte = 0;
    for (uint32_t m = in & ~nb & ~nl; m; m &= m - 1u) { // blanks: only a '\r' that ends its line (or the span) is allowed
        const int b = __builtin_ctz(m);
        const bool line_ends = b == 31 ? next_end : ((brk >> (b + 1)) & 1u) != 0;
        if (!(fq_byte(sm, L + b) == '\r' && line_ends)) bad_byte |= 1u << b;
    }
    for (uint32_t m = start & nb; m; m &= m - 1u) {
        const int b = __builtin_ctz(m);
        const uint8_t c = fq_byte(sm, L + b);
        if (c == '>' || c == '@' || c == '+') bad_byte |= 1u << b;
    }
    // line index (mod 4) of every byte relative to the word's first byte: newlines strictly in front of it
    const uint32_t b0 = fq_prefix_xor_excl(nl);
    const uint32_t b1 = fq_prefix_xor_excl(nl & b0);
    const uint32_t cls[4] = {~b1 & ~b0, ~b1 & b0, b1 & ~b0, b1 & b0};
    FqSum<int32_t> s;
    s.nl = (uint32_t)__builtin_popcount(nl) & 3u;
    s.flags = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const uint32_t seq = cls[(1 - q) & 3], qual = cls[(3 - q) & 3];
        const uint32_t plus = nb & seq, minus = nb & qual;
        s.t[q] = __builtin_popcount(plus) - __builtin_popcount(minus);
        s.v[q] = 0;
        bool bad = (bad_byte & seq) != 0;
        uint32_t ends = nl & qual;
        if (ends) {
            s.flags |= 1u << q;
            const uint32_t below = (ends & (0u - ends)) - 1u;
            s.v[q] = __builtin_popcount(plus & below) - __builtin_popcount(minus & below);
            for (ends &= ends - 1u; ends; ends &= ends - 1u) { // the records that end inside the word behind the first
                const uint32_t bl = (ends & (0u - ends)) - 1u;
                bad = bad || (__builtin_popcount(plus & bl) - __builtin_popcount(minus & bl)) != s.v[q];
            }
        }
        s.flags |= (bad ? 1u : 0u) << (4 + q);
    }
    return s;
}

// bits of the 32-byte word at absolute offset A (from base) that lie inside [begin, end)
MHX_HD uint32_t fq_inrange(uint64_t A, uint64_t begin, uint64_t end)
{
    uint32_t m = 0xFFFFFFFFu;
    if (begin > A) { const uint64_t lo = begin - A; m = lo >= 32 ? 0u : (m << lo); }
    if (end < A + 32) { const uint64_t hi = end > A ? end - A : 0; m &= hi >= 32 ? 0xFFFFFFFFu : ((1u << hi) - 1u); }
    return m;
}

// One lane's 128 bytes of the staged step (read as 16-byte pieces: see FqSmem).
MHX_HD FqSum<int32_t> fq_thread(const FqSmem &sm, int tid, uint64_t tile_off, uint64_t begin, uint64_t end)
{
    const uint4 *mine = sm.bytes + fq_slot(8 * tid + 1);
    FqSum<int32_t> acc = fq_identity<int32_t>();
#pragma unroll
    for (int j = 0; j < kFqBytesPerThread / 32; ++j) {
        const int L = tid * kFqBytesPerThread + 32 * j; // tile byte of the word
        const uint64_t A = tile_off + (uint64_t)L;
        const uint4 lo = mine[2 * j], hi = mine[2 * j + 1];
        const uint32_t w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
        const uint32_t in = fq_inrange(A, begin, end);
        if (!in) continue;
        const bool prev_start = A <= begin || fq_byte(sm, L - 1) == '\n';
        const bool next_end = A + 32 >= end || fq_byte(sm, L + 32) == '\n';
        acc = fq_combine(acc, fq_word(sm, L, w, in, prev_start, next_end));
    }
    return acc;
}

} // namespace mhx
