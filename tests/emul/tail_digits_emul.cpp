// tests/emul/tail_digits_emul.cpp -- the tail table's offset taken from the digits a group packs once (TailDigits<K>,
// auriclass_amd/csrc/mhx_tile.h) on the CPU, against tail_lut_index of the partial word itself, and the hot loop's window
// in that form (window_partial_hash<K, J, ND, true, TailDigits<K>>) against the multiply form.  The functions are the very
// ones the kernel runs.  Not part of the product; built by tests/test_tail_digits.py with g++.
#include <cstdint>
#include <cstring>
#include "../../auriclass_amd/csrc/mhx_tile.h"

using namespace mhx;

// per chunk six values: the packed route's byte offset with the forward and with the reverse strand forced, 8 x
// tail_lut_index of either strand's own partial word, the strand canonical_words (multiply form) takes, and 8 x
// tail_lut_index of the partial word it yields
template <int K, int J> static void offsets(const uint32_t *chunks, uint64_t n, uint32_t *out)
{
    constexpr int ND = GroupGeom<K>::ND, T = K & 7, P = 2 * (K / 8);
    constexpr int OF = J, OR = ND * 4 - K - J;
    for (uint64_t c = 0; c < n; ++c) {
        uint32_t src[ND], U[ND + 1], R[ND + 1], Wr[ND + 1], Cc[ND + 1], wf[8], wr[8], w[8];
        memcpy(src, chunks + c * ND, sizeof(src));
        strand_views<ND>(src, U, R, Wr, Cc);
        const TailDigits<K> digits(U, R);
        extract_words<K, OF>(U, wf);
        extract_words<K, OR>(R, wr);
        const bool rc = canonical_words<K, J, ND>(U, R, Wr, Cc, w);
        uint32_t *o = out + 6 * c;
        o[0] = digits.template byte_offset<J>(false);
        o[1] = digits.template byte_offset<J>(true);
        o[2] = 8u * tail_lut_index<T>(wf[P], wf[(P + 1) & 7]);
        o[3] = 8u * tail_lut_index<T>(wr[P], wr[(P + 1) & 7]);
        o[4] = rc ? 1u : 0u;
        o[5] = 8u * tail_lut_index<T>(w[P], w[(P + 1) & 7]);
    }
}

// per chunk: the hash of window J from the packed route (body words only, entry at the packed offset) and from the
// multiply form
template <int K, int J> static void hashes(const uint32_t *chunks, uint64_t n, uint64_t *packed, uint64_t *mul)
{
    constexpr int ND = GroupGeom<K>::ND;
    for (uint64_t c = 0; c < n; ++c) {
        uint32_t src[ND], U[ND + 1], R[ND + 1], Wr[ND + 1], Cc[ND + 1], w[8];
        memcpy(src, chunks + c * ND, sizeof(src));
        strand_views<ND>(src, U, R, Wr, Cc);
        const TailDigits<K> digits(U, R);
        packed[c] = window_partial_hash<K, J, ND, true>(U, R, Wr, Cc, digits, tail_lut_of<K>()).finish();
        canonical_words<K, J, ND>(U, R, Wr, Cc, w);
        mul[c] = murmur3_h1<K>(w);
    }
}

#define FOR_J(F, ...)                                                                                                  \
    switch (j) {                                                                                                       \
    case 0: F<K, 0>(__VA_ARGS__); return 0;                                                                            \
    case 1: F<K, 1>(__VA_ARGS__); return 0;                                                                            \
    case 2: F<K, 2>(__VA_ARGS__); return 0;                                                                            \
    case 3: F<K, 3>(__VA_ARGS__); return 0;                                                                            \
    case 4: F<K, 4>(__VA_ARGS__); return 0;                                                                            \
    case 5: F<K, 5>(__VA_ARGS__); return 0;                                                                            \
    case 6: F<K, 6>(__VA_ARGS__); return 0;                                                                            \
    case 7: F<K, 7>(__VA_ARGS__); return 0;                                                                            \
    default: return -1;                                                                                                \
    }
template <int K> static int offsets_k(int j, const uint32_t *chunks, uint64_t n, uint32_t *out) { FOR_J(offsets, chunks, n, out) }
template <int K> static int hashes_k(int j, const uint32_t *chunks, uint64_t n, uint64_t *packed, uint64_t *mul) { FOR_J(hashes, chunks, n, packed, mul) }

#define FOR_K(X) X(17) X(18) X(19) X(20) X(21) X(25) X(26) X(27) X(28) X(29)

// 1 when the device's hot loop takes this k's offset from packed digits, 0 when not, -1 for a k outside 1..32
extern "C" int emul_tail_digits_apply(int k)
{
    switch (k) {
#define X(KK) case KK: return tail_lut_applies<KK>() && tail_digits_apply<KK>() ? 1 : 0;
        X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10) X(11) X(12) X(13) X(14) X(15) X(16) X(17) X(18) X(19) X(20) X(21)
        X(22) X(23) X(24) X(25) X(26) X(27) X(28) X(29) X(30) X(31) X(32)
#undef X
    default: return -1;
    }
}

// n chunks of (8 + k - 1 bytes, rounded up to dwords) -> six values per chunk (offsets<K, J>); -1 for a k without a table
extern "C" int emul_tail_digit_offsets(int k, int j, const uint32_t *chunks, uint64_t n, uint32_t *out)
{
    switch (k) {
#define X(KK) case KK: return offsets_k<KK>(j, chunks, n, out);
        FOR_K(X)
#undef X
    default: return -1;
    }
}

extern "C" int emul_tail_digit_hashes(int k, int j, const uint32_t *chunks, uint64_t n, uint64_t *packed, uint64_t *mul)
{
    switch (k) {
#define X(KK) case KK: return hashes_k<KK>(j, chunks, n, packed, mul);
        FOR_K(X)
#undef X
    default: return -1;
    }
}
