// tests/emul/canonical_words_emul.cpp -- canonical_words<K, J, ND> and murmur3_h1<K> (auriclass_amd/csrc/mhx_tile.h, the
// very functions the hash loop of sketch_tile_kernel runs) for every K in 8..32 and every window J in 0..7 of a group,
// on chunks handed in by the test: the K bytes of the canonical strand as the hash reads them, and their hash.
// Not part of the product; built by tests/test_canonical_words.py with g++.
#include <cstdint>
#include <cstring>
#include "../../auriclass_amd/csrc/mhx_tile.h"

using namespace mhx;

template <int K, int J> static void run(const uint32_t *chunks, uint64_t n, uint32_t *words, uint64_t *hashes)
{
    constexpr int ND = GroupGeom<K>::ND;
    for (uint64_t c = 0; c < n; ++c) {
        uint32_t src[ND], U[ND + 1], R[ND + 1], Wr[ND + 1], Cc[ND + 1], w[8];
        memcpy(src, chunks + c * ND, sizeof(src));
        strand_views<ND>(src, U, R, Wr, Cc);
        canonical_words<K, J, ND>(U, R, Wr, Cc, w);
        memcpy(words + c * 8, w, sizeof(w));
        hashes[c] = murmur3_h1<K>(w);
    }
}

template <int K> static int run_k(int j, const uint32_t *chunks, uint64_t n, uint32_t *words, uint64_t *hashes)
{
    switch (j) {
#define X(JJ) case JJ: run<K, JJ>(chunks, n, words, hashes); return 0;
        X(0) X(1) X(2) X(3) X(4) X(5) X(6) X(7)
#undef X
    default: return -1;
    }
}

// dwords of one chunk for this k (the group's 8 + k - 1 bytes, rounded up), 0 for a k outside 8..32
extern "C" int emul_chunk_dwords(int k)
{
    switch (k) {
#define X(KK) case KK: return GroupGeom<KK>::ND;
        X(8) X(9) X(10) X(11) X(12) X(13) X(14) X(15) X(16) X(17) X(18) X(19) X(20)
        X(21) X(22) X(23) X(24) X(25) X(26) X(27) X(28) X(29) X(30) X(31) X(32)
#undef X
    default: return 0;
    }
}

// n chunks of emul_chunk_dwords(k) dwords each -> 8 words and one hash per chunk, for window j
extern "C" int emul_canonical_words(int k, int j, const uint32_t *chunks, uint64_t n, uint32_t *words, uint64_t *hashes)
{
    switch (k) {
#define X(KK) case KK: return run_k<KK>(j, chunks, n, words, hashes);
        X(8) X(9) X(10) X(11) X(12) X(13) X(14) X(15) X(16) X(17) X(18) X(19) X(20)
        X(21) X(22) X(23) X(24) X(25) X(26) X(27) X(28) X(29) X(30) X(31) X(32)
#undef X
    default: return -1;
    }
}
