// tests/emul/contain_within_emul.cpp -- CPU emulator of the unbounded containment call (mhx_contain_within.hip and the host
// loop of mhx_engine_contain_within.cpp, test tool).  Runs the host+device functions of auriclass_amd/csrc/mhx_contain_within.h,
// mhx_within.h, mhx_contain_search.h and mhx_search.h one work item after the other over the three matrices of the pairs (the
// passes that compute a block's pairs have an emulator of their own: contain_emul.cpp): the need table of the bound,
// super-batches of queries, the blocks of each in a permuted order with some taken out only after all others -- the late
// fallback --, the waves of a take-out drawing their places in the arrival list in a shuffled order, then the scan into
// row_off and the gather.
// Not part of the product; built by tests/emul_build.py with g++.
#include <cstdint>
#include <cstring>
#include <vector>
#include "../../auriclass_amd/csrc/mhx_contain_within.h"

using namespace mhx;

static uint64_t next_random(uint64_t &x)
{
    x ^= x << 13; x ^= x >> 7; x ^= x << 17;
    return x;
}
template <class T> static void shuffle(std::vector<T> &v, uint64_t &x)
{
    for (size_t i = v.size(); i > 1; --i) std::swap(v[i - 1], v[next_random(x) % i]);
}

// The whole call over the pairs shared / n_qry / n_ref [nq][nr].  limit: of the need table (no n_ref exceeds it); qbatch:
// queries per block; cells: the limit of a super-batch; seed: the permutation of the blocks and of the waves' arrivals (0: the
// schedule's own order); late: every late-th block of the permuted order is held back and taken out behind all others of its
// super-batch (0: none).  cap: room of the hit arrays, hit_ref null with cap 0 the counting form.  Returns the number of hits;
// row_off [nq + 1] is always complete.
// stats (may be null): [0] super-batches, [1] blocks, [2] blocks taken out late, [3] hits counted beyond the arrival room,
// [4] additions to the arrival counter.
extern "C" uint64_t emul_contain_within(const uint32_t *shared, const uint32_t *n_qry, const uint32_t *n_ref, uint32_t nq, uint32_t nr, uint32_t limit, int k,
                                        double min_identity, uint32_t min_shared, uint32_t qbatch, uint64_t cells, uint64_t seed, uint32_t late,
                                        uint64_t *row_off, uint32_t *hit_ref, uint32_t *hit_shared, uint32_t *hit_n_ref, uint32_t *hit_n_qry, uint64_t cap,
                                        uint64_t *stats)
{
    std::vector<uint32_t> need((size_t)limit + 1);
    contain_need_build(limit, k, min_identity, min_shared, need.data());
    const uint32_t nslices = within_slices(nr), super = within_super_queries(nq, nr, cells ? cells : kWithinCells);
    if (qbatch == 0 || qbatch > super) qbatch = super;
    const bool store = hit_ref != nullptr && cap != 0;
    const uint64_t room64 = store ? ((uint64_t)super * nr < cap ? (uint64_t)super * nr : cap) : 0;
    const uint32_t room = (uint32_t)room64;
    std::vector<uint32_t> mask((size_t)super * nslices), base(store ? (size_t)super * nslices : 0), arr_s(room), arr_r(room), arr_q(room);
    uint64_t x = seed ? seed : 1, n_super = 0, n_blocks = 0, n_late = 0, n_beyond = 0, n_atomics = 0;
    row_off[0] = 0;
    for (uint32_t s0 = 0; s0 < nq; s0 += super, ++n_super) {
        const uint32_t snq = nq - s0 < super ? nq - s0 : super;
        std::fill(mask.begin(), mask.end(), 0xDEADBEEFu); // every cell must be written by its block
        uint32_t count = 0;
        const uint64_t nblocks = search_blocks(snq, nr, qbatch);
        std::vector<uint64_t> order, held;
        for (uint64_t b = 0; b < nblocks; ++b) order.push_back(b);
        if (seed) shuffle(order, x);
        if (late) { // the flagged blocks of a group: skipped by their take-out, redone behind the others
            std::vector<uint64_t> now;
            for (size_t i = 0; i < order.size(); ++i) (i % late == late - 1 ? held : now).push_back(order[i]);
            order = now;
            order.insert(order.end(), held.begin(), held.end());
        }
        n_blocks += nblocks;
        n_late += held.size();
        for (const uint64_t b : order) {
            const SearchBlock blk = search_block(snq, nr, qbatch, b);
            // block-local results [queries of the block][32], as the finish pass or the pair kernel leaves them: the query
            // of the CALL is s0 + blk.q0 + ql, the cell counts from the super-batch's first
            std::vector<uint32_t> loc_s((size_t)blk.nq * kTriSlice, 0xFFFFFFFFu), loc_q(loc_s), loc_r(loc_s);
            for (uint32_t ql = 0; ql < blk.nq; ++ql)
                for (uint32_t rl = 0; rl < blk.nr; ++rl) {
                    const size_t from = (size_t)(s0 + blk.q0 + ql) * nr + blk.r0 + rl, to = (size_t)ql * kTriSlice + rl;
                    loc_s[to] = shared[from]; loc_q[to] = n_qry[from]; loc_r[to] = n_ref[from];
                }
            // contain_within_take_kernel: a wave holds two cells; the waves reach the arrival counter in any order
            std::vector<uint32_t> waves;
            for (uint32_t w = 0; w < (blk.nq + 1) / 2; ++w) waves.push_back(w);
            if (seed) shuffle(waves, x);
            for (const uint32_t w : waves) {
                uint32_t word[2] = {0, 0};
                for (uint32_t h = 0; h < 2; ++h)
                    if (2 * w + h < blk.nq)
                        word[h] = contain_within_ballot(&loc_s[(size_t)(2 * w + h) * kTriSlice], &loc_r[(size_t)(2 * w + h) * kTriSlice], blk.nr, need.data(), limit);
                uint32_t first = 0;
                if (store && (word[0] | word[1])) { first = count; count += within_popc(word[0]) + within_popc(word[1]); ++n_atomics; }
                for (uint32_t h = 0; h < 2; ++h) {
                    const uint32_t ql = 2 * w + h;
                    if (ql >= blk.nq) continue;
                    const uint32_t start = first + (h ? within_popc(word[0]) : 0u);
                    if (store)
                        for (uint32_t rl = 0; rl < blk.nr; ++rl)
                            if ((word[h] >> rl) & 1u) {
                                const uint32_t at = start + within_rank(word[h], rl);
                                const size_t from = (size_t)ql * kTriSlice + rl;
                                if (at < room) { arr_s[at] = loc_s[from]; arr_r[at] = loc_r[from]; arr_q[at] = loc_q[from]; }
                                else ++n_beyond;
                            }
                    within_cell_record(mask.data(), store ? base.data() : nullptr, within_cell(blk.q0 + ql, blk.r0, nslices), word[h], start);
                }
            }
        }
        // within_count_kernel and within_offsets_kernel
        for (uint32_t q = 0; q < snq; ++q) row_off[s0 + q + 1] = row_off[s0 + q] + within_row_count(&mask[(size_t)q * nslices], nslices);
        // contain_within_gather_kernel
        if (store)
            for (uint32_t q = 0; q < snq; ++q) {
                uint64_t before = 0;
                for (uint32_t sl = 0; sl < nslices; ++sl) {
                    const uint64_t cell = (uint64_t)q * nslices + sl;
                    const uint32_t n = within_popc(mask[cell]);
                    for (uint32_t rank = 0; rank < n; ++rank) {
                        const uint64_t to = within_dest(row_off[s0 + q], before, rank);
                        const uint32_t from = base[cell] + rank;
                        if (to >= cap || from >= room) continue;
                        hit_ref[to] = sl * kTriSlice + within_nth_bit(mask[cell], rank);
                        hit_shared[to] = arr_s[from];
                        hit_n_ref[to] = arr_r[from];
                        hit_n_qry[to] = arr_q[from];
                    }
                    before += n;
                }
            }
    }
    if (stats) { stats[0] = n_super; stats[1] = n_blocks; stats[2] = n_late; stats[3] = n_beyond; stats[4] = n_atomics; }
    return row_off[nq];
}

#ifdef CONTAIN_WITHIN_EMUL_MAIN
// stand-alone run for a host sanitizer build: a small matrix through several batch sizes, permutations and capacities
#include <cstdio>
int main()
{
    const uint32_t nq = 23, nr = 70, limit = 64;
    std::vector<uint32_t> c((size_t)nq * nr), a((size_t)nq * nr), b((size_t)nq * nr);
    uint64_t x = 88172645463325252ull;
    for (size_t i = 0; i < c.size(); ++i) {
        b[i] = i % 7 == 3 ? (uint32_t)(next_random(x) % (limit + 1)) : limit;
        c[i] = (uint32_t)(next_random(x) % (b[i] + 1));
        if (i % 5 == 0) c[i] = b[i];
        a[i] = c[i] + (uint32_t)(next_random(x) % 60);
    }
    auto run = [&](uint32_t qbatch, uint64_t cells, uint64_t seed, uint32_t late, uint64_t *off, uint32_t *r, uint32_t *s, uint32_t *nr_, uint32_t *nq_, uint64_t cap,
                   uint64_t *stats) {
        return emul_contain_within(c.data(), a.data(), b.data(), nq, nr, limit, 21, 0.95, 2, qbatch, cells, seed, late, off, r, s, nr_, nq_, cap, stats);
    };
    std::vector<uint64_t> off0(nq + 1), off(nq + 1);
    uint64_t stats[5];
    const uint64_t n0 = run(0, 0, 0, 0, off0.data(), nullptr, nullptr, nullptr, nullptr, 0, stats);
    int bad = stats[4] != 0; // the counting form does no atomic
    std::vector<uint32_t> r0(n0), s0(n0), f0(n0), q0(n0), r1(n0), s1(n0), f1(n0), q1(n0);
    bad |= run(0, 0, 0, 0, off.data(), r0.data(), s0.data(), f0.data(), q0.data(), n0, nullptr) != n0 || off != off0;
    const uint64_t forms[][4] = {{1, 0, 7, 3}, {5, 20, 11, 2}, {23, 3, 13, 0}, {4, 9, 5, 1}};
    for (const auto &f : forms) {
        const uint64_t n = run((uint32_t)f[0], f[1], f[2], (uint32_t)f[3], off.data(), r1.data(), s1.data(), f1.data(), q1.data(), n0, stats);
        if (n != n0 || off != off0 || r1 != r0 || s1 != s0 || f1 != f0 || q1 != q0 || stats[3]) { printf("form %llu differs\n", (unsigned long long)f[0]); bad = 1; }
        if (n0 && (run((uint32_t)f[0], f[1], f[2], (uint32_t)f[3], off.data(), r1.data(), s1.data(), f1.data(), q1.data(), n0 - 1, stats) != n0 || off != off0)) {
            printf("form %llu: row_off incomplete beside a short list\n", (unsigned long long)f[0]);
            bad = 1;
        }
    }
    if (bad || n0 == 0) printf("FAILED\n");
    else printf("ok (%llu hits)\n", (unsigned long long)n0);
    return bad || n0 == 0;
}
#endif
