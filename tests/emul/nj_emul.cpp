// tests/emul/nj_emul.cpp -- CPU emulator of neighbour joining (mhx_nj.hip, test tool).  Runs the host+device functions of
// auriclass_amd/csrc/mhx_nj.h themselves over whole calls: the init pass and the three launches of every join -- scan (the
// workgroups' spans of words, and the words of a span, in any order), join (the workgroups' candidates reduced in any order)
// and update (one work item per position of the active list, in any order: no work item reads what another one of the same
// launch writes, and the shares of r[b] are an integer sum).  seed 0 takes the kernels' order, another seed shuffles every
// launch.  The distances come from the packed common / denom of a triangle or, common == null, as raw words in `denom`'s
// place.  Not part of the product; built by tests/test_nj_emulation.py with g++.
#include <algorithm>
#include <cstdint>
#include <numeric>
#include <vector>
#include "../../auriclass_amd/csrc/mhx_nj.h"

using namespace mhx;

namespace {

struct Rng {
    uint64_t x;
    explicit Rng(uint64_t seed) : x(seed * 0x9E3779B97F4A7C15ull + 88172645463325252ull) {}
    uint64_t draw(uint64_t bound) { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return (x >> 11) % bound; }
    template <class T> void shuffle(std::vector<T> &v) { for (size_t i = v.size(); i > 1; --i) std::swap(v[i - 1], v[draw(i)]); }
};

std::vector<uint32_t> order_of(uint32_t count, Rng &rng, bool shuffled)
{
    std::vector<uint32_t> o(count);
    std::iota(o.begin(), o.end(), 0u);
    if (shuffled) rng.shuffle(o);
    return o;
}

} // namespace

extern "C" int64_t emul_nj_q(uint32_t m, uint64_t d, uint64_t ri, uint64_t rj) { return nj_q(m, d, ri, rj); }
extern "C" int emul_nj_precedes(int64_t qa, uint32_t la, uint32_t ha, int64_t qb, uint32_t lb, uint32_t hb)
{
    return nj_cand_precedes(NjCand{qa, la, ha}, NjCand{qb, lb, hb}) ? 1 : 0;
}
extern "C" uint64_t emul_nj_join_word(uint64_t dac, uint64_t dbc, uint64_t dab, int *clamped)
{
    const NjWord w = nj_join_word(dac, dbc, dab);
    *clamped = w.clamped ? 1 : 0;
    return w.d;
}
extern "C" void emul_nj_lengths(uint64_t d, uint32_t m, uint64_t r_a, uint64_t r_b, double *len_a, double *len_b)
{
    nj_lengths(NjRecord{1, 0, d, r_a, r_b}, m, *len_a, *len_b);
}
extern "C" uint32_t emul_nj_scan_blocks(uint32_t n, uint32_t m) { return nj_scan_blocks(n, m); }

// A whole call over n nodes: the packed common / denom of the triangle, or (common == null) `raw`, the packed distance words.
// Outputs [n - 1] each; *clamps: the updates the clamp changed.  `blocks` > 0 overrides the number of workgroups of every
// scan (the spans then cut the rows elsewhere).  Returns the number of records, or -1 - t when join t goes wrong.
extern "C" int64_t emul_nj_call(const uint32_t *common, const uint32_t *denom, const uint64_t *raw, uint32_t n, int k, uint64_t seed, uint32_t blocks,
                                uint32_t *join_a, uint32_t *join_b, uint64_t *d, uint64_t *r_a, uint64_t *r_b, double *len_a, double *len_b, uint64_t *clamps)
{
    *clamps = 0;
    if (n < 2) return 0;
    Rng rng(seed);
    const bool shuffled = seed != 0;
    const uint64_t pairs = (uint64_t)n * (n - 1) / 2;
    std::vector<uint64_t> words(pairs), r(n, 0), pre[2];
    std::vector<uint32_t> act[2];
    const NjState s{words.data(), r.data(), n};
    // init: the words, the list of all ids with its running sums, the first r
    for (uint64_t p = 0; p < pairs; ++p) words[p] = common ? linkage_fixed_distance(common[p], denom[p], k) : raw[p];
    for (int x = 0; x < 2; ++x) { act[x].assign(n, kNjNone); pre[x].assign((size_t)n + 1, ~0ull); }
    for (uint32_t p = 0; p <= n; ++p) { if (p < n) act[0][p] = p; pre[0][p] = p ? (uint64_t)p * (p - 1) / 2 : 0; }
    for (const uint32_t i : order_of(n, rng, shuffled)) {
        uint64_t sum = 0;
        for (uint32_t j = 0; j < i; ++j) sum += words[tri_index(i, j)];
        for (uint32_t c = i + 1; c < n; ++c) sum += words[tri_index(c, i)];
        r[i] = sum;
    }
    for (uint32_t t = 0; t + 1 < n; ++t) {
        const uint32_t m = n - t, from = t & 1u, to = from ^ 1u;
        NjRecord rec;
        if (m > 2) {
            // scan: every workgroup its span, every word of the span once
            const uint32_t grid = blocks ? blocks : nj_scan_blocks(n, m);
            std::vector<NjCand> cand(grid, nj_no_cand());
            for (const uint32_t b : order_of(grid, rng, shuffled)) {
                uint64_t w0, w1;
                nj_span(pre[from][m], grid, b, w0, w1);
                if (w0 >= w1) continue;
                struct Item { uint32_t i, j; };
                std::vector<Item> items;
                for (uint32_t p = nj_first_row(pre[from].data(), m, w0); p < m && pre[from][p] < w1; ++p) {
                    uint32_t c0, c1;
                    nj_row_part(pre[from].data(), p, act[from][p], w0, w1, c0, c1);
                    for (uint32_t j = c0; j < c1; ++j) items.push_back(Item{act[from][p], j});
                }
                if (items.size() != w1 - w0) return -1 - (int64_t)t; // the spans cover the words exactly
                if (shuffled) rng.shuffle(items);
                for (const Item &it : items) cand[b] = nj_cand_better(cand[b], nj_scan_candidate(s, m, it.i, r[it.i], it.j));
            }
            // join
            NjCand mine = nj_no_cand();
            for (const uint32_t b : order_of(grid, rng, shuffled)) mine = nj_cand_better(mine, cand[b]);
            NjPick pick;
            if (!nj_join(s, act[from].data(), m, mine, rec, pick)) return -1 - (int64_t)t;
            // update
            uint64_t r_u = 0;
            for (const uint32_t p : order_of(m + 1, rng, shuffled)) {
                uint32_t q;
                uint64_t sum;
                if (!nj_compact(pick, pre[from].data(), p, q, sum)) continue;
                pre[to][q] = sum;
                if (p == m) continue;
                const uint32_t c = act[from][p];
                act[to][q] = c;
                if (c == pick.b) continue;
                const NjWord w = nj_update(s, pick, c);
                r_u += w.d;
                *clamps += w.clamped ? 1 : 0;
            }
            r[pick.b] += r_u;
        } else rec = nj_last_record(s, act[from].data());
        join_a[t] = rec.a; join_b[t] = rec.b; d[t] = rec.d; r_a[t] = rec.r_a; r_b[t] = rec.r_b;
        nj_lengths(rec, m, len_a[t], len_b[t]);
    }
    return (int64_t)n - 1;
}
