// tests/emul/cluster_emul.cpp -- CPU emulator of the single-linkage clustering (mhx_cluster.hip, test tool).  Runs the
// host+device functions of auriclass_amd/csrc/mhx_cluster.h themselves: the builder of the cmin table, the integer edge rule
// over the cells of the triangle's blocks in the kernels' order, the union one pair after the other, and the union of many
// pairs at once -- V virtual threads, each executing cluster_union_step, ONE access to `parent` per step, in an order a
// seeded schedule chooses --, followed by the flatten pass.  Not part of the product; built by
// tests/test_cluster_emulation.py with g++.
#include <cstdint>
#include <vector>
#include "../../auriclass_amd/csrc/mhx_cluster.h"

using namespace mhx;

extern "C" void emul_cluster_cmin(uint32_t s, int k, double max_dist, uint32_t *cmin) { cluster_cmin_build(s, k, max_dist, cmin); }

// tri_cluster_kernel's choice over a whole call: the blocks of the schedule in order, the cells of a block in order, a cell
// that counts and passes cluster_keep is an edge.  common / denom: the packed triangle (what the block-local arrays hold
// for these pairs).  Returns the number of edges; the first `cap` go to (out_i, out_j).
extern "C" uint64_t emul_cluster_edges(const uint32_t *common, const uint32_t *denom, uint32_t n, uint32_t qbatch, const uint32_t *cmin, uint32_t s,
                                       uint32_t *out_i, uint32_t *out_j, uint64_t cap)
{
    uint64_t m = 0;
    TriBlock b;
    for (bool more = tri_first_block(n, qbatch, b); more; more = tri_next_block(n, qbatch, b))
        for (uint32_t id = 0; id < b.nq * kTriSlice; ++id) {
            const uint32_t ql = id / kTriSlice, rl = id % kTriSlice;
            if (!tri_pair_counts(b, ql, rl)) continue;
            const uint64_t at = tri_index(b.q0 + ql, b.r0 + rl);
            if (!cluster_keep(common[at], denom[at], cmin, s)) continue;
            if (m < cap) { out_i[m] = b.q0 + ql; out_j[m] = b.r0 + rl; }
            ++m;
        }
    return m;
}

static uint32_t flatten_all(uint32_t *parent, uint32_t n)
{
    uint32_t roots = 0;
    for (uint32_t i = 0; i < n; ++i) roots += cluster_flatten(parent, i) ? 1u : 0u;
    return roots;
}

// one union after the other, a flatten pass every `flatten_every` pairs (0: never) and behind the last; returns the roots
extern "C" uint32_t emul_cluster_sequential(uint32_t n, const uint32_t *ei, const uint32_t *ej, uint64_t m, uint64_t flatten_every, uint32_t *parent)
{
    for (uint32_t i = 0; i < n; ++i) parent[i] = i;
    for (uint64_t e = 0; e < m; ++e) {
        cluster_union(parent, ei[e], ej[e]);
        if (flatten_every && (e + 1) % flatten_every == 0) flatten_all(parent, n);
    }
    return flatten_all(parent, n);
}

// V virtual threads, each with one pending pair (the next of the list when it is done); every turn ONE thread executes ONE
// step -- one load or one compare-and-swap.  adversarial == 0: the thread of a turn is drawn at random.  adversarial != 0:
// a thread that still walks is always preferred, so that every thread of a round has found both roots before the first
// compare-and-swap of that round happens -- as many of them as can be then fail.  Returns the roots, -1 when parent[x] > x
// was ever seen (a hook under a larger index); *max_retries: the most failed compare-and-swaps of any one union.
extern "C" int64_t emul_cluster_interleaved(uint32_t n, const uint32_t *ei, const uint32_t *ej, uint64_t m, uint32_t V, uint64_t seed, int adversarial,
                                            uint32_t *parent, uint32_t *max_retries)
{
    for (uint32_t i = 0; i < n; ++i) parent[i] = i;
    uint64_t x = seed * 0x9E3779B97F4A7C15ull + 88172645463325252ull;
    auto draw = [&](uint64_t bound) { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return (x >> 11) % bound; };
    std::vector<ClusterUnion> live;
    uint64_t next = 0;
    uint32_t worst = 0;
    for (;;) {
        while (live.size() < V && next < m) { live.push_back(cluster_union_begin(ei[next], ej[next])); ++next; }
        if (live.empty()) break;
        size_t t = (size_t)draw(live.size());
        if (adversarial) { // the first thread at or behind t that still walks, if any
            for (size_t o = 0; o < live.size(); ++o) {
                const size_t c = (t + o) % live.size();
                if (live[c].phase < 2) { t = c; break; }
            }
        }
        const bool done = cluster_union_step(parent, live[t]);
        worst = live[t].retries > worst ? live[t].retries : worst;
        if (done) { live[t] = live.back(); live.pop_back(); }
    }
    for (uint32_t i = 0; i < n; ++i) if (parent[i] > i) return -1;
    *max_retries = worst;
    return (int64_t)flatten_all(parent, n);
}

#ifdef CLUSTER_EMUL_MAIN
// stand-alone run for a host sanitizer build: a ring of chains through both schedules, and a table
#include <cstdio>
int main()
{
    const uint32_t n = 300;
    std::vector<uint32_t> ei, ej, parent(n), ref(n);
    for (uint32_t i = 1; i < n; ++i) if (i % 50) { ei.push_back((i * 7) % n > ((i - 1) * 7) % n ? (i * 7) % n : ((i - 1) * 7) % n); ej.push_back((i * 7) % n > ((i - 1) * 7) % n ? ((i - 1) * 7) % n : (i * 7) % n); }
    const uint32_t roots = emul_cluster_sequential(n, ei.data(), ej.data(), ei.size(), 0, ref.data());
    int bad = 0;
    for (uint64_t seed = 0; seed < 8; ++seed) {
        uint32_t retries = 0;
        const int64_t got = emul_cluster_interleaved(n, ei.data(), ej.data(), ei.size(), 64, seed, (int)(seed & 1), parent.data(), &retries);
        if (got != (int64_t)roots || parent != ref || retries > n) { printf("seed %llu differs\n", (unsigned long long)seed); bad = 1; }
    }
    std::vector<uint32_t> cmin(100001);
    cluster_cmin_build(100000, 21, 0.05, cmin.data());
    for (uint32_t d = 1; d <= 100000; d += 997)
        if (cmin[d] > d || !cluster_is_edge(cmin[d], d, 21, 0.05) || (cmin[d] && cluster_is_edge(cmin[d] - 1, d, 21, 0.05))) { printf("cmin[%u] wrong\n", d); bad = 1; }
    printf(bad ? "FAILED\n" : "ok (%u clusters)\n", roots);
    return bad;
}
#endif
