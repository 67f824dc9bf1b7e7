// tests/asan/medoid_fuzz.cpp -- stand-alone program for a host AddressSanitizer / UBSan build (tests/test_medoid_emulation.py): the
// host+device functions of auriclass_amd/csrc/mhx_medoid.h through the emulator of tests/emul/medoid_emul.cpp on heap arrays of
// exact size -- the block predicate next to a brute force, the sum pass next to a plain double loop, the pick, and the pair walk
// next to a walk over std::set -- on seeded random partitions and lists.  Prints "ok" and returns 0, or says what differs.
#include "../emul/medoid_emul.cpp"
#include <cstdio>
#include <random>
#include <algorithm>
#include <set>
int main()
{
    std::mt19937_64 rng(5);
    // predicate and sum pass on random partitions of random sizes, exact-size heap arrays
    for (int round = 0; round < 60; ++round) {
        const uint32_t n = 1 + rng() % 300, clusters = 1 + rng() % 9, qbatch = 1 + rng() % 100;
        std::vector<uint32_t> label(n), first(clusters, 0xFFFFFFFFu);
        for (uint32_t i = 0; i < n; ++i) { const uint32_t c = rng() % clusters; if (first[c] == 0xFFFFFFFFu) first[c] = i; label[i] = first[c]; }
        if (medoid_first_bad_label(label.data(), n) != n) return 1;
        std::vector<uint8_t> runs(100000), brute(100000);
        const uint32_t nb = emul_medoid_blocks(label.data(), n, qbatch, runs.data(), brute.data(), 100000);
        for (uint32_t b = 0; b < nb; ++b) if (runs[b] != brute[b]) { printf("predicate differs\n"); return 2; }
        const size_t pairs = (size_t)n * (n - 1) / 2;
        std::vector<uint32_t> common(pairs), denom(pairs);
        for (size_t p = 0; p < pairs; ++p) { denom[p] = 1 + rng() % 1000; common[p] = rng() % (denom[p] + 1); }
        std::vector<uint64_t> sum(n, 0), want(n, 0);
        uint64_t adds; uint32_t most;
        emul_medoid_sums(common.data(), denom.data(), n, 21, qbatch, label.data(), sum.data(), &adds, &most);
        for (uint32_t i = 0; i < n; ++i) for (uint32_t j = 0; j < i; ++j) if (label[i] == label[j]) { const uint64_t q = linkage_fixed_distance(common[tri_index(i, j)], denom[tri_index(i, j)], 21); want[i] += q; want[j] += q; }
        if (sum != want || most > 34) { printf("sums differ\n"); return 3; }
        std::vector<uint32_t> med(n);
        emul_medoid_pick(label.data(), sum.data(), n, med.data());
    }
    // the pair walk on exact-size lists
    for (int round = 0; round < 400; ++round) {
        const uint32_t nA = rng() % 60, nB = rng() % 60, s = 1 + rng() % 80;
        std::set<uint64_t> a, b;
        while (a.size() < nA) a.insert(rng() % 100);
        while (b.size() < nB) b.insert(rng() % 100);
        std::vector<uint64_t> A(a.begin(), a.end()), B(b.begin(), b.end());
        std::set<uint64_t> uni(a); uni.insert(b.begin(), b.end());
        uint32_t u = 0, c = 0;
        for (uint64_t v : uni) { if (++u > s) break; if (a.count(v) && b.count(v)) ++c; }
        const uint32_t d = std::min<uint32_t>(s, uni.size());
        for (uint32_t shares : {1u, 3u, 16u, 256u, 1024u}) {
            uint32_t gc, gd;
            emul_medoid_pair(A.data(), nA, B.data(), nB, shares, s, &gc, &gd);
            if (gc != c || gd != d) { printf("pair differs %u %u: %u/%u want %u/%u\n", nA, nB, gc, gd, c, d); return 4; }
        }
    }
    printf("ok\n");
    return 0;
}
