// tests/emul/pair_words_emul.cpp -- PairWords<K, J, ND, BODY_ONLY> (auriclass_amd/csrc/mhx_tile.h: the words of windows J
// and J + 4 of a group from one funnel shift per strand) next to canonical_words<K, J, ND, BODY_ONLY>, the per-window
// route it stands in for, for every K in 17..32 and every window 0..7 of a group, on chunks handed in by the test.
// Both forms of either: all the window's dwords, and the full 8-byte words in front of the partial word alone (the K
// that have a partial word).  Also the switch: which K and kernel forms take the pair route.
// Not part of the product; built by tests/test_pair_words.py with g++.
#include <cstdint>
#include <cstring>
#include "../../auriclass_amd/csrc/mhx_tile.h"

using namespace mhx;

// per chunk: out[0..8) the pair's words, out[8..16) canonical_words', out[16..24) the pair's body-only words, out[24..32)
// canonical_words' (zero where K has no partial word), out[32] / out[33] the strand either route decided; hashes: murmur3_h1
// of the pair's words
template <int K, int W> static void run(const uint32_t *chunks, uint64_t n, uint32_t *out, uint64_t *hashes)
{
    constexpr int ND = GroupGeom<K>::ND, J = W % 4;
    constexpr bool SECOND = W >= 4;
    for (uint64_t c = 0; c < n; ++c) {
        uint32_t src[ND], U[ND + 1], R[ND + 1], Wr[ND + 1], Cc[ND + 1];
        uint32_t *o = out + c * 34;
        memcpy(src, chunks + c * ND, sizeof(src));
        strand_views<ND>(src, U, R, Wr, Cc);
        uint32_t wp[8], wc[8], bp[8] = {}, bc[8] = {};
        const bool rc_pair = canonical_strand<K, W, ND>(U, R, Wr, Cc);
        const PairWords<K, J, ND, false> pair(U, R);
        pair.template words<SECOND>(rc_pair, wp);
        const bool rc = canonical_words<K, W, ND>(U, R, Wr, Cc, wc);
        if constexpr (K % 8 != 0) {
            const PairWords<K, J, ND, true> body(U, R);
            body.template words<SECOND>(rc_pair, bp);
            canonical_words<K, W, ND, true>(U, R, Wr, Cc, bc);
        }
        memcpy(o, wp, 32); memcpy(o + 8, wc, 32); memcpy(o + 16, bp, 32); memcpy(o + 24, bc, 32);
        o[32] = rc_pair; o[33] = rc;
        hashes[c] = murmur3_h1<K>(wp);
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

#define MHX_EMUL_KS(X) X(17) X(18) X(19) X(20) X(21) X(22) X(23) X(24) X(25) X(26) X(27) X(28) X(29) X(30) X(31) X(32)

// dwords of one chunk for this k, 0 for a k outside 17..32
extern "C" int emul_chunk_dwords(int k)
{
    switch (k) {
#define X(KK) case KK: return GroupGeom<KK>::ND;
        MHX_EMUL_KS(X)
#undef X
    default: return 0;
    }
}

// n chunks of emul_chunk_dwords(k) dwords each -> 34 dwords (see run) and one hash per chunk, for window w
extern "C" int emul_pair_words(int k, int w, const uint32_t *chunks, uint64_t n, uint32_t *out, uint64_t *hashes)
{
    switch (k) {
#define X(KK) case KK: return run_k<KK>(w, chunks, n, out, hashes);
        MHX_EMUL_KS(X)
#undef X
    default: return -1;
    }
}

// the switch: does the kernel form (fmt, queue) of this k take the pair route?  (k outside 1..32: -1)
extern "C" int emul_pair_words_form(int k, int fmt, int queue)
{
    switch (k) {
#define X(KK) case KK: return pair_words_form<KK>(fmt, queue != 0) ? 1 : 0;
        X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10) X(11) X(12) X(13) X(14) X(15) X(16) MHX_EMUL_KS(X)
#undef X
    default: return -1;
    }
}
