// tests/emul/contain_search_emul.cpp -- CPU emulator of the containment search's take-out (mhx_contain_search.hip, test tool).
// Runs the host+device functions of auriclass_amd/csrc/mhx_contain_search.h -- contain_better, contain_insert, contain_keep
// and the host's contain_need_build -- and the schedule of mhx_search.h in the engine's order, one work item after the
// other: per block of the schedule the three counts of its pairs go into block-local [queries][32] arrays (where the finish
// pass or the pair kernel leaves them; the counts themselves are the caller's: tests/emul/contain_emul.cpp emulates how they come
// about), then the take-out feeds the candidates that pass the hit test, lowest lane first, through contain_insert.  A
// flagged block is delivered behind its group of blocks, as the engine redoes it.
// Not part of the product; built by tests/test_contain_search_emulation.py with g++.
#include <cstdint>
#include <cstring>
#include <vector>
#include "../../auriclass_amd/csrc/mhx_contain_search.h"

using namespace mhx;

extern "C" int emul_contain_better(uint32_t ar, uint32_t as, uint32_t an, uint32_t br, uint32_t bs, uint32_t bn)
{
    return contain_better(ContainHit{ar, as, an, 0}, ContainHit{br, bs, bn, 0}) ? 1 : 0;
}

// candidates order[0 .. n) of (ref, shared, n_ref)[...] one after the other through contain_insert; returns the list's length
extern "C" uint32_t emul_contain_insert_many(const uint32_t *ref, const uint32_t *shared, const uint32_t *n_ref, const uint32_t *order, uint32_t n,
                                             uint32_t top, uint32_t *out_ref, uint32_t *out_shared, uint32_t *out_n_ref)
{
    std::vector<ContainHit> list(top);
    uint32_t m = 0;
    for (uint32_t i = 0; i < n; ++i) m = contain_insert(list.data(), m, top, ContainHit{ref[order[i]], shared[order[i]], n_ref[order[i]], 0});
    for (uint32_t i = 0; i < m; ++i) { out_ref[i] = list[i].ref; out_shared[i] = list[i].shared; out_n_ref[i] = list[i].n_ref; }
    return m;
}

extern "C" void emul_contain_need(uint32_t limit, int k, double min_identity, uint32_t min_shared, uint32_t *need)
{
    contain_need_build(limit, k, min_identity, min_shared, need);
}

extern "C" int emul_contain_keep(uint32_t shared, uint32_t n_ref, const uint32_t *need, uint32_t limit) { return contain_keep(shared, n_ref, need, limit) ? 1 : 0; }

// The whole call over the counts shared / n_qry / n_ref [nq][nr] of its pairs.  qbatch: queries per block (0: all); reverse
// != 0: the blocks of a group run last to first; flagged (may be null): [blocks], non-zero = the block's finish and take-out
// do nothing and the block is delivered behind its group; group: blocks per group (0: 4096, the engine's).  need_limit: the
// table covers n_ref = 0 .. need_limit.  Outputs as the host form of mhx_dist_contain_search: [nq][top] best first, zero
// behind n_hits[q].  Returns the number of blocks, -2 for bad arguments.
extern "C" int64_t emul_contain_search(const uint32_t *shared, const uint32_t *n_qry, const uint32_t *n_ref, uint32_t nq, uint32_t nr, uint32_t qbatch,
                                       int reverse, const uint8_t *flagged, uint32_t group, int k, double min_identity, uint32_t min_shared,
                                       uint32_t need_limit, uint32_t top, uint32_t *hit_ref, uint32_t *hit_shared, uint32_t *hit_n_ref, uint32_t *hit_n_qry,
                                       uint32_t *n_hits)
{
    if (nq == 0 || nr == 0 || top < 1 || top > kSearchMaxTop || min_shared == 0) return -2;
    if (qbatch == 0 || qbatch > nq) qbatch = nq;
    if (group == 0) group = 4096;
    std::vector<uint32_t> need((size_t)need_limit + 1);
    contain_need_build(need_limit, k, min_identity, min_shared, need.data());
    std::vector<ContainHit> lists((size_t)nq * top);
    std::vector<uint32_t> n(nq, 0); // zeroed at the start of the call
    std::vector<uint32_t> loc_s((size_t)qbatch * kTriSlice), loc_q((size_t)qbatch * kTriSlice), loc_r((size_t)qbatch * kTriSlice);
    const uint64_t nblocks = search_blocks(nq, nr, qbatch);
    auto deliver = [&](uint64_t bi) {
        const SearchBlock b = search_block(nq, nr, qbatch, bi);
        // contain_finish_kernel / contain_pairs_kernel: cell (q, r) at q * 32 + r - (q0 * 32 + r0)
        std::fill(loc_s.begin(), loc_s.end(), 0xFFFFFFFFu);
        std::fill(loc_r.begin(), loc_r.end(), 0u);
        std::fill(loc_q.begin(), loc_q.end(), 0xFFFFFFFFu);
        const uint64_t base = (uint64_t)b.q0 * kTriSlice + b.r0;
        for (uint32_t ql = 0; ql < b.nq; ++ql)
            for (uint32_t rl = 0; rl < b.nr; ++rl) {
                const uint64_t in = (uint64_t)(b.q0 + ql) * nr + b.r0 + rl, out = (uint64_t)(b.q0 + ql) * kTriSlice + b.r0 + rl - base;
                loc_s[out] = shared[in]; loc_q[out] = n_qry[in]; loc_r[out] = n_ref[in];
            }
        // contain_take_kernel: one wave per query; the candidates that pass the hit test, lowest lane first
        for (uint32_t ql = 0; ql < b.nq; ++ql)
            for (uint32_t lane = 0; lane < b.nr; ++lane) {
                const ContainHit c{b.r0 + lane, loc_s[(size_t)ql * kTriSlice + lane], loc_r[(size_t)ql * kTriSlice + lane], loc_q[(size_t)ql * kTriSlice + lane]};
                if (!contain_keep(c.shared, c.n_ref, need.data(), need_limit)) continue;
                const uint32_t gq = b.q0 + ql;
                n[gq] = contain_insert(&lists[(size_t)gq * top], n[gq], top, c);
            }
    };
    for (uint64_t b0 = 0; b0 < nblocks; b0 += group) {
        const uint64_t b1 = b0 + group < nblocks ? b0 + group : nblocks;
        for (uint64_t i = b0; i < b1; ++i) {
            const uint64_t bi = reverse ? b1 - 1 - (i - b0) : i;
            if (!(flagged && flagged[bi])) deliver(bi);
        }
        for (uint64_t bi = b0; bi < b1; ++bi)
            if (flagged && flagged[bi]) deliver(bi);
    }
    for (uint32_t i = 0; i < nq; ++i) {
        for (uint32_t t = 0; t < top; ++t) {
            const size_t at = (size_t)i * top + t;
            const ContainHit h = t < n[i] ? lists[at] : ContainHit{0, 0, 0, 0};
            hit_ref[at] = h.ref; hit_shared[at] = h.shared; hit_n_ref[at] = h.n_ref; hit_n_qry[at] = h.n_qry;
        }
        n_hits[i] = n[i];
    }
    return (int64_t)nblocks;
}

#ifdef CONTAIN_SEARCH_EMUL_MAIN
// stand-alone run for a host sanitizer build: the header's functions on a made-up count table through every order of
// delivery, batch size and top; all orders must give the same lists, and the lists must be sorted and complete
#include <cstdio>
int main()
{
    const uint32_t nq = 11, nr = 150, limit = 300;
    std::vector<uint32_t> shared((size_t)nq * nr), n_qry((size_t)nq * nr), n_ref((size_t)nq * nr);
    uint64_t x = 88172645463325252ull;
    for (size_t i = 0; i < shared.size(); ++i) {
        x ^= x << 13; x ^= x >> 7; x ^= x << 17;
        n_ref[i] = (uint32_t)(x % 7 == 0 ? 0 : (x >> 8) % (limit + 1));
        shared[i] = n_ref[i] == 0 ? 0 : (uint32_t)((x >> 20) % 4 == 0 ? n_ref[i] : (x >> 24) % (n_ref[i] + 1)); // many ties at 1/1
        n_qry[i] = shared[i] + (uint32_t)((x >> 40) % 50);
    }
    int bad = 0;
    for (uint32_t top : {1u, 5u, 64u})
        for (double min_identity : {0.0, 0.9, 1.0, 1.5})
            for (uint32_t min_shared : {1u, 20u}) {
                const size_t cells = (size_t)nq * top;
                std::vector<uint32_t> r0(cells), s0(cells), a0(cells), b0(cells), h0(nq), r(cells), s(cells), a(cells), b(cells), h(nq);
                std::vector<uint8_t> flagged(512, 0);
                for (size_t i = 0; i < flagged.size(); ++i) flagged[i] = i % 3 == 1;
                const uint32_t forms[][3] = {{0, 0, 0}, {4, 0, 0}, {4, 1, 0}, {3, 0, 1}, {1, 1, 1}, {0, 1, 1}};
                for (size_t f = 0; f < sizeof forms / sizeof forms[0]; ++f) {
                    const int64_t rc = emul_contain_search(shared.data(), n_qry.data(), n_ref.data(), nq, nr, forms[f][0], (int)forms[f][1], forms[f][2] ? flagged.data() : nullptr,
                                                           7, 21, min_identity, min_shared, limit, top, f ? r.data() : r0.data(), f ? s.data() : s0.data(),
                                                           f ? a.data() : a0.data(), f ? b.data() : b0.data(), f ? h.data() : h0.data());
                    if (rc <= 0 || rc > (int64_t)flagged.size()) { printf("form %zu: rc %lld\n", f, (long long)rc); bad = 1; }
                    if (f && (r != r0 || s != s0 || a != a0 || b != b0 || h != h0)) { printf("top %u: form %zu differs from form 0\n", top, f); bad = 1; }
                }
                for (uint32_t q = 0; q < nq; ++q) {
                    uint32_t hits = 0;
                    for (uint32_t j = 0; j < nr; ++j)
                        hits += contain_is_hit(shared[(size_t)q * nr + j], n_ref[(size_t)q * nr + j], 21, min_identity, min_shared) ? 1u : 0u;
                    if (h0[q] != (hits < top ? hits : top)) { printf("query %u: %u hits in the list, %u by the predicate\n", q, h0[q], hits); bad = 1; }
                    for (uint32_t t = 0; t + 1 < h0[q]; ++t) {
                        const size_t at = (size_t)q * top + t;
                        if (!contain_better(ContainHit{r0[at], s0[at], a0[at], b0[at]}, ContainHit{r0[at + 1], s0[at + 1], a0[at + 1], b0[at + 1]})) { printf("query %u: entry %u out of order\n", q, t); bad = 1; }
                    }
                }
            }
    printf(bad ? "FAILED\n" : "ok\n");
    return bad;
}
#endif
