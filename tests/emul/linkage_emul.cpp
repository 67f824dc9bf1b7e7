// tests/emul/linkage_emul.cpp -- CPU emulator of complete and average linkage (mhx_linkage.hip, test tool).  Runs the
// host+device functions of auriclass_amd/csrc/mhx_linkage.h themselves over whole calls: the init pass, the first scan of every
// row, and the three launches of every step -- pick (the rows' candidates reduced in any order), update (one work item per
// cluster, in any order: no work item reads what another one of the same launch writes, so the order must not matter) and
// rescan (the rows of the work list, their partners in any order).  seed 0 takes the kernels' order, another seed shuffles
// every launch.  Not part of the product; built by tests/test_linkage_emulation.py with g++.
#include <algorithm>
#include <cstdint>
#include <numeric>
#include <vector>
#include "../../auriclass_amd/csrc/mhx_linkage.h"

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

void rescan(const LinkState &s, const std::vector<uint32_t> &list, Rng &rng, bool shuffled)
{
    for (const uint32_t i : list) {
        LinkCand mine = link_no_cand();
        for (const uint32_t j : order_of(i, rng, shuffled)) mine = link_cand_better(s.linkage, mine, link_scan_candidate(s, i, j));
        s.nn[i] = mine.hi == kLinkNone ? kLinkNone : mine.lo;
    }
}

} // namespace

extern "C" uint64_t emul_linkage_fixed_distance(uint32_t common, uint32_t denom, int k) { return linkage_fixed_distance(common, denom, k); }
extern "C" int emul_linkage_cmp(int linkage, uint64_t wa, uint64_t da, uint64_t wb, uint64_t db) { return link_cmp(linkage, LinkVal{wa, da}, LinkVal{wb, db}); }
extern "C" uint64_t emul_linkage_combine(int linkage, uint64_t wa, uint64_t wb) { return link_combine(linkage, wa, wb); }
extern "C" uint32_t emul_linkage_labels(const uint32_t *ma, const uint32_t *mb, const double *dist, uint32_t n, double max_dist, uint32_t *label)
{
    return linkage_labels(ma, mb, dist, n, max_dist, label);
}

// A whole call over the packed common / denom of n lists.  Outputs [n - 1] each; nn_trace (may be null) [n - 1][n]: nn of every
// row behind every step, kLinkNone for a row that is no cluster; *rescans: the rows scanned again by the steps.  Returns the
// number of merges, or -1 - t when step t finds no pair.
extern "C" int64_t emul_linkage_call(const uint32_t *common, const uint32_t *denom, uint32_t n, int k, int linkage, uint64_t seed, uint32_t *merge_a,
                                     uint32_t *merge_b, uint32_t *size_out, uint64_t *num, uint64_t *den, double *dist, uint32_t *nn_trace, uint64_t *rescans)
{
    *rescans = 0;
    if (n < 2) return 0;
    Rng rng(seed);
    const bool shuffled = seed != 0;
    const uint64_t pairs = (uint64_t)n * (n - 1) / 2;
    std::vector<uint64_t> words(pairs);
    std::vector<uint32_t> size(n, 1u), nn(n, kLinkNone), list;
    const LinkState s{words.data(), size.data(), nn.data(), n, linkage};
    for (uint64_t p = 0; p < pairs; ++p) words[p] = link_init_word(linkage, common[p], denom[p], k);
    for (uint32_t i = 1; i < n; ++i) list.push_back(i);
    rescan(s, list, rng, shuffled);
    for (uint32_t t = 0; t + 1 < n; ++t) {
        LinkCand mine = link_no_cand();
        for (const uint32_t i : order_of(n, rng, shuffled)) mine = link_cand_better(linkage, mine, link_row_candidate(s, i));
        if (mine.hi >= n || mine.lo >= mine.hi) return -1 - (int64_t)t;
        const LinkPick p{mine.hi, mine.lo, size[mine.hi], size[mine.lo]};
        link_record(linkage, mine, num[t], den[t]);
        merge_a[t] = p.a; merge_b[t] = p.b; size_out[t] = p.size_a + p.size_b;
        dist[t] = link_height(linkage, num[t], den[t], k);
        list.clear();
        for (const uint32_t c : order_of(n, rng, shuffled))
            if (link_update(s, p, c)) list.push_back(c);
        *rescans += list.size();
        rescan(s, list, rng, shuffled);
        if (nn_trace)
            for (uint32_t i = 0; i < n; ++i) nn_trace[(size_t)t * n + i] = size[i] ? nn[i] : kLinkNone;
    }
    return (int64_t)n - 1;
}
