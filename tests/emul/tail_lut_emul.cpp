// tests/emul/tail_lut_emul.cpp -- the tail tables of the hash (auriclass_amd/csrc/mhx_tail_lut.h) and murmur3_core<K> in
// both forms (mhx_tile.h: the partial word of the tail block multiplied, or taken from the table as the device's hot loop
// takes it) on the CPU: the host arrays hold what the device arrays hold (one constexpr generator), and the index is the
// very function the kernel runs.  Not part of the product; built by tests/test_tail_lut.py with g++.
#include <cstdint>
#include <cstring>
#include "../../auriclass_amd/csrc/mhx_tile.h"

using namespace mhx;

// the entries of table (t, second) into out (room for 1024); their number, or -1
extern "C" int emul_tail_lut_entries(int t, int second, uint64_t *out)
{
#define X(TT)                                                                                                         \
    case TT: {                                                                                                        \
        const uint64_t *p = second ? tail_lut_table<TT, true>() : tail_lut_table<TT, false>();                        \
        memcpy(out, p, sizeof(uint64_t) << (2 * TT));                                                                 \
        return 1 << (2 * TT);                                                                                         \
    }
    switch (t) {
        X(1) X(2) X(3) X(4) X(5)
    default: return -1;
    }
#undef X
}

// index of the partial word {hi:lo} holding t bases, for n words; -1 for a t without a table
extern "C" int emul_tail_lut_index(int t, const uint32_t *lo, const uint32_t *hi, uint64_t n, uint32_t *out)
{
    for (uint64_t i = 0; i < n; ++i) {
        switch (t) {
#define X(TT) case TT: out[i] = tail_lut_index<TT>(lo[i], hi[i]); break;
            X(1) X(2) X(3) X(4) X(5)
#undef X
        default: return -1;
        }
    }
    return 0;
}

// 1 when the hot loop of the device takes this k's partial word from a table
extern "C" int emul_tail_lut_applies(int k)
{
    switch (k) {
#define X(KK) case KK: return tail_lut_applies<KK>() ? 1 : 0;
        X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10) X(11) X(12) X(13) X(14) X(15) X(16) X(17) X(18) X(19) X(20) X(21)
        X(22) X(23) X(24) X(25) X(26) X(27) X(28) X(29) X(30) X(31) X(32)
#undef X
    default: return -1;
    }
}

template <int K, int J> static void run(const uint32_t *chunks, uint64_t n, uint64_t *mul, uint64_t *lut)
{
    constexpr int ND = GroupGeom<K>::ND;
    for (uint64_t c = 0; c < n; ++c) {
        uint32_t src[ND], U[ND + 1], R[ND + 1], Wr[ND + 1], Cc[ND + 1], w[8];
        memcpy(src, chunks + c * ND, sizeof(src));
        strand_views<ND>(src, U, R, Wr, Cc);
        canonical_words<K, J, ND>(U, R, Wr, Cc, w);
        mul[c] = murmur3_h1<K>(w);
        if constexpr (tail_lut_applies<K>()) lut[c] = murmur3_core<K, true>(w, tail_lut_of<K>()).finish();
        else lut[c] = 0;
    }
}

template <int K> static int run_k(int j, const uint32_t *chunks, uint64_t n, uint64_t *mul, uint64_t *lut)
{
    switch (j) {
#define X(JJ) case JJ: run<K, JJ>(chunks, n, mul, lut); return 0;
        X(0) X(1) X(2) X(3) X(4) X(5) X(6) X(7)
#undef X
    default: return -1;
    }
}

// n chunks of (8 + k - 1 bytes, rounded up to dwords) -> the hash of window j's canonical strand, multiplied and (for a k
// with a table; else 0) from the table
extern "C" int emul_tail_hashes(int k, int j, const uint32_t *chunks, uint64_t n, uint64_t *mul, uint64_t *lut)
{
    switch (k) {
#define X(KK) case KK: return run_k<KK>(j, chunks, n, mul, lut);
        X(16) X(17) X(18) X(19) X(20) X(21) X(22) X(24) X(25) X(26) X(27) X(28) X(29) X(32)
#undef X
    default: return -1;
    }
}
