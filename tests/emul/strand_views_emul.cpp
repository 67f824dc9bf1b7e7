// tests/emul/strand_views_emul.cpp -- the strand decision of the sketch kernel's hash loop from the two views the hash
// reads (auriclass_amd/csrc/mhx_tile.h: strand_views<ND>(src, U, R), canonical_strand<K, J, ND>(U, R)), and everything that
// takes those two views: canonical_words<K, J, ND> in both forms, PairWords' route, the table routes of the tail block.
// Next to them the four-view overloads the older emulators call, on views made by the four-view strand_views.
// For every K in 8..32 and every window 0..7 of a group, on chunks handed in by the test.  The functions are the very
// ones the kernel runs.  Not part of the product; built by tests/test_strand_views.py with g++.
#include <cstdint>
#include <cstring>
#include "../../auriclass_amd/csrc/mhx_tile.h"

using namespace mhx;

constexpr int kOut = 64; // dwords per chunk, see run
constexpr uint32_t kNone = 0xFFFFFFFFu;

// per chunk, out:
//   [0..8)   canonical_words<K, W, ND>(U, R, w)                [8..16)  the four-view overload's, on the four views
//   [16..24) its BODY_ONLY form (K > 16 with a partial word)    [24..32) the four-view overload's
//   [32..40) PairWords<K, W % 4, ND, false>'s words (K > 16)    [40..48) PairWords<K, W % 4, ND, true>'s (as [16..24))
//   [48] canonical_strand(U, R)   [49] the strand canonical_words(U, R, w) returns   [50] / [51] the same two by the four-view
//   overloads   [52] window_is_acgt<K, W, ND>(U)   [53] 8 x tail_lut_index of the partial word in [0..8) (kNone: no table for K)
//   [54] TailDigits<K>'s byte offset on the strand [48] (kNone: no table)   [55] bytes of the table (0: none)
// hashes, three per chunk: murmur3_h1<K> of [0..8); window_partial_hash by the table and the packed digits; window_pair_hash by
// the same route (both the first value where K has no table)
template <int K, int W> static void run(const uint32_t *chunks, uint64_t n, uint32_t *out, uint64_t *hashes)
{
    constexpr int ND = GroupGeom<K>::ND, J = W % 4;
    constexpr bool SECOND = W >= 4;
    for (uint64_t c = 0; c < n; ++c) {
        uint32_t src[ND], U[ND + 1], R[ND + 1], U4[ND + 1], R4[ND + 1], Wr[ND + 1], Cc[ND + 1];
        uint32_t *o = out + c * kOut;
        uint64_t *h = hashes + 3 * c;
        memcpy(src, chunks + c * ND, sizeof(src));
        strand_views<ND>(src, U, R);
        strand_views<ND>(src, U4, R4, Wr, Cc);
        uint32_t w2[8], w4[8], b2[8] = {}, b4[8] = {}, wp[8] = {}, bp[8] = {};
        const bool rc2 = canonical_words<K, W, ND>(U, R, w2);
        const bool rc4 = canonical_words<K, W, ND>(U4, R4, Wr, Cc, w4);
        bool rs2 = rc2, rs4 = rc4; // K < 8 has no decision apart from its words
        if constexpr (K >= 8) {
            rs2 = canonical_strand<K, W, ND>(U, R);
            rs4 = canonical_strand<K, W, ND>(U4, R4, Wr, Cc);
        }
        o[53] = o[54] = kNone;
        o[55] = 0;
        h[0] = h[1] = h[2] = murmur3_h1<K>(w2);
        if constexpr (K > 16) {
            const PairWords<K, J, ND, false> pair(U, R);
            pair.template words<SECOND>(rs2, wp);
            if constexpr (K % 8 != 0) {
                canonical_words<K, W, ND, true>(U, R, b2);
                canonical_words<K, W, ND, true>(U4, R4, Wr, Cc, b4);
                const PairWords<K, J, ND, true> body(U, R);
                body.template words<SECOND>(rs2, bp);
            }
            if constexpr (tail_lut_applies<K>()) {
                constexpr int T = K & 7, P = 2 * (K / 8);
                const TailDigits<K> digits(U, R);
                o[53] = 8u * tail_lut_index<T>(w2[P], w2[(P + 1) & 7]);
                o[54] = digits.template byte_offset<W>(rs2);
                o[55] = 8u << (2 * T);
                if (o[53] < o[55] && o[54] < o[55]) { // (the test asserts the range; no read outside the table here)
                    h[1] = window_partial_hash<K, W, ND, true>(U, R, digits, tail_lut_of<K>()).finish();
                    const PairWords<K, J, ND, true> body(U, R);
                    h[2] = window_pair_hash<K, J, ND, SECOND, true>(body, U, R, digits, tail_lut_of<K>()).finish();
                }
            }
        }
        memcpy(o, w2, 32); memcpy(o + 8, w4, 32); memcpy(o + 16, b2, 32); memcpy(o + 24, b4, 32); memcpy(o + 32, wp, 32); memcpy(o + 40, bp, 32);
        o[48] = rs2; o[49] = rc2; o[50] = rs4; o[51] = rc4;
        o[52] = window_is_acgt<K, W, ND>(U) ? 1u : 0u;
        for (int i = 56; i < kOut; ++i) o[i] = 0;
    }
}

template <int K> static int run_k(int w, const uint32_t *chunks, uint64_t n, uint32_t *out, uint64_t *hashes)
{
    switch (w) {
#define X(WW) case WW: run<K, WW>(chunks, n, out, hashes); return 0;
        X(0) X(1) X(2) X(3) X(4) X(5) X(6) X(7)
#undef X
    default: return -1;
    }
}

#define MHX_EMUL_KS(X) X(8) X(9) X(10) X(11) X(12) X(13) X(14) X(15) X(16) X(17) X(18) X(19) X(20) X(21) X(22) X(23) X(24) X(25) \
    X(26) X(27) X(28) X(29) X(30) X(31) X(32)

// dwords of one chunk for this k, 0 for a k outside 8..32
extern "C" int emul_chunk_dwords(int k)
{
    switch (k) {
#define X(KK) case KK: return GroupGeom<KK>::ND;
        MHX_EMUL_KS(X)
#undef X
    default: return 0;
    }
}

extern "C" int emul_out_dwords() { return kOut; }

// n chunks of emul_chunk_dwords(k) dwords each -> kOut dwords and three hashes per chunk (see run), for window w
extern "C" int emul_strand_views(int k, int w, const uint32_t *chunks, uint64_t n, uint32_t *out, uint64_t *hashes)
{
    switch (k) {
#define X(KK) case KK: return run_k<KK>(w, chunks, n, out, hashes);
        MHX_EMUL_KS(X)
#undef X
    default: return -1;
    }
}
