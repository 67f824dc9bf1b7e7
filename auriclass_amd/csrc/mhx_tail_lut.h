// mhx_tail_lut.h -- Murmur's tail block as a table look-up.
//
// The last, partial 8-byte word of the key goes through two 64x64 multiplications and a rotation before it is xor-ed
// into the state: k1 = rotl31(x * c1) * c2 for the first word of the tail block, k2 = rotl33(x * c2) * c1 for the second.
// When that word holds t = 1..5 bases it is a pure function of 2t bits (4^t <= 1024 entries of 8 bytes, 8 KB at most), and
// the sketch kernel's vector-memory path is idle inside the hash loop: one gather replaces 10 VALU instructions
// (2 x v_mad_u64_u32, 4 x v_mul_lo_u32, 2 x v_add3_u32, 2 x v_alignbit) for the 5 that form the offset.
//
// Index: base j of the word (byte j, little-endian) is digit j, two bits wide, its value bits 1..2 of the ASCII byte:
// A, C, T, G -> 0, 1, 2, 3 -- the case bit (5) is not among them, so upper and lower case index alike.  The entry holds the
// value for the UPPER-case letters (mash upper-cases before hashing).  The offset is formed from those masked bits and
// nothing else (tail_lut_index), so it lies inside the table for all 256 values of every byte: the hot loop hashes windows
// that are no valid start as well (newline, quality or halo bytes in them) and windows that hold an N, and they must load
// from inside the table.  Such a window gets the entry of the four letters its bytes alias to -- NOT Murmur's value of its
// bytes.  That is allowed for the reason the base check is deferred (mhx_tile.h, head comment): it is never a true
// candidate.  The inline form drops it in window_is_acgt (or by its cleared bit of the start mask) after finish(); the
// queue form hands it to process_deferred, which checks the bases first and hashes from the bytes itself, in the
// multiply form.  No statistic counts a window before those checks.
#pragma once
#include <stdint.h>

#include "mhx_hd.h"

namespace mhx {

constexpr uint64_t kMurmurC1 = 0x87c37b91114253d5ull, kMurmurC2 = 0x4cf5ad432745937full;
constexpr uint32_t kTailLutLetters = 0x47544341u; // digit -> 'A', 'C', 'T', 'G'

// the little-endian value of the T upper-case bases that index i stands for
constexpr uint64_t tail_lut_word(int t, uint32_t i)
{
    uint64_t x = 0;
    for (int j = 0; j < t; ++j) x |= (uint64_t)((kTailLutLetters >> (8 * ((i >> (2 * j)) & 3u))) & 0xFFu) << (8 * j);
    return x;
}
constexpr uint64_t tail_lut_rotl(uint64_t x, int r) { return (x << r) | (x >> (64 - r)); }
// SECOND = false: the partial k1 word; true: the partial k2 word
constexpr uint64_t tail_lut_value(bool second, uint64_t x)
{
    return second ? tail_lut_rotl(x * kMurmurC2, 33) * kMurmurC1 : tail_lut_rotl(x * kMurmurC1, 31) * kMurmurC2;
}
template <int T, bool SECOND> struct TailLut {
    static_assert(T >= 1 && T <= 5, "bases in the partial word");
    static constexpr uint32_t kEntries = 1u << (2 * T);
    uint64_t v[kEntries];
    constexpr TailLut() : v{}
    {
        for (uint32_t i = 0; i < kEntries; ++i) v[i] = tail_lut_value(SECOND, tail_lut_word(T, i));
    }
};
// one table per (T, SECOND) that is used, per translation unit: in device memory for the kernels, in host memory
// for the CPU emulators
template <int T, bool SECOND> inline constexpr TailLut<T, SECOND> kTailLutHost{};
#if defined(__HIPCC__)
template <int T, bool SECOND> static __device__ const TailLut<T, SECOND> kTailLutDevice{};
#endif

// Index of the partial word {hi:lo} (T bases, T <= 5: hi holds the fifth).  The four digits of lo: lo & 0x06060606
// keeps bits 1..2 of every byte where they stand (bits 8j + 1, 8j + 2); times 2^23 + 2^17 + 2^11 + 2^5 digit j lands on
// bits 24 + 2j, 25 + 2j, and the stray partial products (digit j times the term of digit i != j, at bit 24 + 8j - 6i) fall
// on distinct bit pairs below 24 or beyond 31 -- nothing overlaps, so nothing carries.  The top byte is the index of
// four bases; the fifth digit is put on top of it.  Bytes beyond T are masked away whatever they hold.
template <int T> MHX_HD uint32_t tail_lut_index(uint32_t lo, uint32_t hi)
{
    static_assert(T >= 1 && T <= 5, "bases in the partial word");
    constexpr uint32_t mask = T >= 4 ? 0x06060606u : (0x06060606u & ((1u << (8 * T)) - 1u));
    if constexpr (T == 1) return (lo & mask) >> 1;
    const uint32_t p = (lo & mask) * 0x00820820u;
    if constexpr (T < 5) return p >> 24;
    const uint32_t fifth = (hi >> 1) & 3u;
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_alignbit(fifth, p, 24); // (fifth << 8) | (p >> 24) as one instruction
#else
    return (fifth << 8) | (p >> 24);
#endif
}

// The digits of NDW = 2 or 3 consecutive dwords (8 or 12 bytes, lowest first) packed into one word: the digit of byte i on
// bits 2i, 2i + 1.  Every dword goes the way of tail_lut_index -- mask, times 0x00820820, its four digits in the top byte --
// and two v_perm_b32 put the top bytes side by side (selector 0x0c: a zero byte).  A window's index is then a 2T-bit field
// of this word, tail_lut_index<T> of the T bytes from byte i on = bits 2i .. 2i + 2T - 1: the sketch kernel packs once per
// group of eight windows what it would otherwise form per window (mhx_tile.h, TailDigits).  Like the index itself the
// word is made of bits 1..2 of the bytes and nothing else, so any field of it lies inside the table for every byte value.
MHX_HD uint32_t tail_lut_perm(uint32_t hi, uint32_t lo, uint32_t sel)
{ // v_perm_b32: out.byte[i] = byte sel.byte[i] of {hi:lo} (0..7), or zero (0x0c)
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_perm(hi, lo, sel);
#else
    const uint64_t both = ((uint64_t)hi << 32) | lo;
    uint32_t o = 0;
    for (int i = 0; i < 4; ++i) {
        const uint32_t s = (sel >> (8 * i)) & 0xFFu;
        if (s < 8u) o |= (uint32_t)((both >> (8 * s)) & 0xFFu) << (8 * i);
    }
    return o;
#endif
}
template <int NDW> MHX_HD uint32_t tail_lut_pack(uint32_t d0, uint32_t d1, uint32_t d2)
{
    static_assert(NDW == 2 || NDW == 3, "dwords packed");
    const uint32_t p0 = (d0 & 0x06060606u) * 0x00820820u, p1 = (d1 & 0x06060606u) * 0x00820820u;
    const uint32_t two = tail_lut_perm(p1, p0, 0x0c0c0703u); // {0, 0, top of p1, top of p0}
    if constexpr (NDW == 2) return two;
    return tail_lut_perm((d2 & 0x06060606u) * 0x00820820u, two, 0x0c070100u);
}

// The table itself.  On the device the address is made opaque in a scalar register pair: left as the constant it is,
// hipcc materialises it anew in every basic block that loads from it (s_getpc_b64, two adds, an s_load_dwordx2 from the
// GOT and an s_waitcnt on it in front of every gather); opaque, that happens once, outside the hash loop.  Behind the
// barrier the compiler no longer knows that the pointer is one into global memory (it falls back to flat_load with a 64-bit
// address sum per gather), so the type says it: the gather is global_load_dwordx2 v, v_offset, s[base].
#if defined(__HIP_DEVICE_COMPILE__)
typedef const __attribute__((address_space(1))) uint64_t *TailLutPtr;
#else
typedef const uint64_t *TailLutPtr;
#endif
// the entry at a byte offset (8 * index)
MHX_HD uint64_t tail_lut_at(TailLutPtr lut, uint32_t byte_offset)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return *(TailLutPtr)((const __attribute__((address_space(1))) char *)lut + byte_offset);
#else
    return *(TailLutPtr)((const char *)lut + byte_offset);
#endif
}
template <int T, bool SECOND> MHX_HD TailLutPtr tail_lut_table()
{
#if defined(__HIP_DEVICE_COMPILE__)
    const uint64_t *p = kTailLutDevice<T, SECOND>.v;
    asm("" : "+s"(p));
    return (TailLutPtr)p;
#else
    return kTailLutHost<T, SECOND>.v;
#endif
}

} // namespace mhx
