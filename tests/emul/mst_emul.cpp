// tests/emul/mst_emul.cpp -- CPU emulator of the single-linkage tree (mhx_mst.hip, test tool).  Runs the host+device functions
// of auriclass_amd/csrc/mhx_mst.h themselves over whole calls: the five steps of every Boruvka round -- reset, propose (from
// the packed triangle row by row, the stored source, or cell by cell over the triangle's blocks with the reduction among the
// 32 cells that share a query, the recomputed source), choose, hook and flatten -- until one component is left.  Proposals,
// choices and the unions of the hooks run one after the other (in the kernels' order or shuffled) or as V virtual threads,
// each executing ONE access to the shared word per step, in an order a seeded schedule chooses.  Not part of the product;
// built by tests/test_mst_emulation.py with g++.
#include <algorithm>
#include <cstdint>
#include <vector>
#include "../../auriclass_amd/csrc/mhx_mst.h"

using namespace mhx;

namespace {

struct Rng {
    uint64_t x;
    explicit Rng(uint64_t seed) : x(seed * 0x9E3779B97F4A7C15ull + 88172645463325252ull) {}
    uint64_t draw(uint64_t bound) { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return (x >> 11) % bound; }
    template <class T> void shuffle(std::vector<T> &v) { for (size_t i = v.size(); i > 1; --i) std::swap(v[i - 1], v[draw(i)]); }
};

// V virtual threads over a list of step machines: every turn ONE thread executes ONE step.  adversarial: a thread that has
// not finished its loads yet (phase < swap_phase) is always preferred, so that every thread has loaded before anyone swaps --
// as many swaps as can be then fail (cluster_emul.cpp's schedule).  step(t) returns true when thread t is done.
template <class M, class Step>
uint32_t interleave(std::vector<M> &todo, uint32_t V, Rng &rng, bool adversarial, uint32_t swap_phase, Step step)
{
    std::vector<M> live;
    size_t next = 0;
    uint32_t worst = 0;
    for (;;) {
        while (live.size() < V && next < todo.size()) live.push_back(todo[next++]);
        if (live.empty()) break;
        size_t t = (size_t)rng.draw(live.size());
        if (adversarial)
            for (size_t o = 0; o < live.size(); ++o) {
                const size_t c = (t + o) % live.size();
                if (live[c].phase < swap_phase) { t = c; break; }
            }
        const bool done = step(live[t]);
        worst = std::max(worst, live[t].retries);
        if (done) { live[t] = live.back(); live.pop_back(); }
    }
    return worst;
}

} // namespace

extern "C" int emul_mst_precedes(uint32_t ac, uint32_t ad, uint32_t ai, uint32_t aj, uint32_t bc, uint32_t bd, uint32_t bi, uint32_t bj)
{
    return mst_precedes(mst_edge(ac, ad, ai, aj), mst_edge(bc, bd, bi, bj)) ? 1 : 0;
}

extern "C" uint32_t emul_mst_labels(const uint32_t *ei, const uint32_t *ej, const uint32_t *ec, const uint32_t *ed, uint32_t n, int k, double max_dist,
                                    uint32_t *label)
{
    return mst_labels(ei, ej, ec, ed, n, k, max_dist, label);
}

// A whole call.  common / denom: the packed triangle (what the block-local arrays hold for these pairs).
//   stored != 0: the rows of mst_scan_kernel; else the blocks of the schedule with `qbatch` queries, cell by cell
//   shuffle != 0: the units of a step (rows or blocks; vertices; roots) in a shuffled order
//   V == 0: every proposal, choice and union runs to its end before the next starts
//   V > 0: V virtual threads, interleaved access by access (adversarial as in cluster_emul.cpp)
// Outputs: the edges in the order of arrival (n - 1 of them), rounds[0] the rounds taken, lost[r] / appended[r] the components
// lost and the edges appended in round r (at most 64 rounds are recorded), *max_retries the most failed swaps of one
// proposal, choice or union.  Returns the number of edges, -1 when a round joined nothing or the rounds passed the cap,
// -2 when parent[x] > x was ever seen.
extern "C" int64_t emul_mst_call(const uint32_t *common, const uint32_t *denom, uint32_t n, int stored, uint32_t qbatch, uint64_t shuffle, uint32_t V,
                                 uint64_t seed, int adversarial, uint32_t *out_i, uint32_t *out_j, uint32_t *out_c, uint32_t *out_d, uint32_t *rounds,
                                 uint32_t *lost, uint32_t *appended, uint32_t *max_retries)
{
    Rng rng(seed + 977 * shuffle);
    std::vector<uint64_t> best(n);
    std::vector<uint32_t> winner(n), parent(n), comp(n);
    for (uint32_t i = 0; i < n; ++i) parent[i] = comp[i] = i;
    uint32_t components = n, worst = 0;
    uint64_t m = 0;
    *rounds = 0;
    while (components > 1) {
        if (*rounds == mst_max_rounds(n)) return -1;
        // step 1
        for (uint32_t v = 0; v < n; ++v) { best[v] = 0; winner[v] = kMstNobody; }
        // step 2: the proposals, in the order the kernels make them
        std::vector<MstPropose> props;
        if (stored) {
            std::vector<uint32_t> rows_;
            for (uint32_t i = 1; i < n; ++i) rows_.push_back(i);
            if (shuffle) rng.shuffle(rows_);
            for (uint32_t i : rows_) {
                uint64_t mine[256] = {0};
                for (uint32_t j = 0; j < i; ++j) { // thread j % 256 of the row's workgroup
                    if (comp[j] == comp[i]) continue;
                    const uint64_t at = tri_index(i, j);
                    mine[j % 256] = mst_word_better(mine[j % 256], mst_pack(common[at], denom[at], j));
                    props.push_back(mst_propose_begin(j, mst_pack(common[at], denom[at], i)));
                }
                for (uint32_t wave = 0; wave < 4; ++wave) { // a wave reduces, one lane proposes
                    uint64_t w = 0;
                    for (uint32_t lane = 0; lane < 64; ++lane) w = mst_word_better(w, mine[wave * 64 + lane]);
                    if (mst_valid(w)) props.push_back(mst_propose_begin(i, w));
                }
            }
        } else {
            std::vector<TriBlock> blocks;
            TriBlock b;
            for (bool more = tri_first_block(n, qbatch, b); more; more = tri_next_block(n, qbatch, b)) blocks.push_back(b);
            if (shuffle) rng.shuffle(blocks);
            for (const TriBlock &blk : blocks)
                for (uint32_t ql = 0; ql < blk.nq; ++ql) { // the 32 cells that share query ql
                    uint64_t mine = 0;
                    const uint32_t i = blk.q0 + ql;
                    for (uint32_t rl = 0; rl < kTriSlice; ++rl) {
                        if (!tri_pair_counts(blk, ql, rl)) continue;
                        const uint32_t j = blk.r0 + rl;
                        if (comp[i] == comp[j]) continue;
                        const uint64_t at = tri_index(i, j);
                        mine = mst_word_better(mine, mst_pack(common[at], denom[at], j));
                        props.push_back(mst_propose_begin(j, mst_pack(common[at], denom[at], i)));
                    }
                    if (mst_valid(mine)) props.push_back(mst_propose_begin(i, mine));
                }
        }
        if (shuffle) rng.shuffle(props);
        if (V == 0) for (MstPropose &p : props) { while (!mst_propose_step(best.data(), p)) {} worst = std::max(worst, p.retries); }
        else worst = std::max(worst, interleave(props, V, rng, adversarial != 0, 1u, [&](MstPropose &p) { return mst_propose_step(best.data(), p); }));
        // step 3
        std::vector<MstChoose> choices;
        for (uint32_t v = 0; v < n; ++v) if (mst_valid(best[v])) choices.push_back(mst_choose_begin(v, comp[v]));
        if (shuffle) rng.shuffle(choices);
        if (V == 0) for (MstChoose &x : choices) { while (!mst_choose_step(winner.data(), best.data(), x)) {} worst = std::max(worst, x.retries); }
        else worst = std::max(worst, interleave(choices, V, rng, adversarial != 0, 1u, [&](MstChoose &x) { return mst_choose_step(winner.data(), best.data(), x); }));
        // step 4: the decisions read what no one writes in this step; the unions run against each other
        std::vector<uint32_t> roots_;
        for (uint32_t a = 0; a < n; ++a) roots_.push_back(a);
        if (shuffle) rng.shuffle(roots_);
        std::vector<ClusterUnion> unions;
        const uint64_t before = m;
        for (uint32_t a : roots_) {
            const MstHook h = mst_hook(comp.data(), winner.data(), best.data(), a);
            if (!h.picks) continue;
            if (h.appends) {
                if (m < (uint64_t)n - 1) { out_i[m] = std::max(h.v, h.u); out_j[m] = std::min(h.v, h.u); out_c[m] = h.common; out_d[m] = h.denom; }
                ++m;
            }
            unions.push_back(cluster_union_begin(h.v, h.u));
        }
        if (V == 0) for (ClusterUnion &u : unions) { while (!cluster_union_step(parent.data(), u)) {} worst = std::max(worst, u.retries); }
        else worst = std::max(worst, interleave(unions, V, rng, adversarial != 0, 2u, [&](ClusterUnion &u) { return cluster_union_step(parent.data(), u); }));
        for (uint32_t i = 0; i < n; ++i) if (parent[i] > i) return -2;
        // step 5
        uint32_t now = 0;
        for (uint32_t i = 0; i < n; ++i) now += cluster_flatten(parent.data(), i) ? 1u : 0u;
        comp = parent;
        if (*rounds < 64) { lost[*rounds] = components - now; appended[*rounds] = (uint32_t)(m - before); }
        ++*rounds;
        if (now >= components) return -1;
        components = now;
    }
    *max_retries = worst;
    return (int64_t)m;
}

#ifdef MST_EMUL_MAIN
// stand-alone run for a host sanitizer build: a set of 150 lists with ties at every level, through both pair sources and
// all schedules, against Kruskal by std::sort with mst_precedes
#include <cstdio>
int main()
{
    const uint32_t n = 150;
    const uint64_t pairs = (uint64_t)n * (n - 1) / 2;
    std::vector<uint32_t> common(pairs), denom(pairs);
    Rng rng(5);
    for (uint64_t p = 0; p < pairs; ++p) { denom[p] = 1 + (uint32_t)rng.draw(12); common[p] = (uint32_t)rng.draw(denom[p] + 1); }
    struct E { uint32_t i, j, c, d; };
    std::vector<E> all;
    for (uint32_t i = 1; i < n; ++i) for (uint32_t j = 0; j < i; ++j) all.push_back(E{i, j, common[tri_index(i, j)], denom[tri_index(i, j)]});
    auto before = [](const E &a, const E &b) { return mst_precedes(mst_edge(a.c, a.d, a.i, a.j), mst_edge(b.c, b.d, b.i, b.j)); };
    std::sort(all.begin(), all.end(), before);
    std::vector<uint32_t> label(n);
    std::vector<E> want;
    for (uint32_t i = 0; i < n; ++i) label[i] = i;
    for (const E &e : all) {
        if (cluster_find(label.data(), e.i) == cluster_find(label.data(), e.j)) continue;
        cluster_union(label.data(), e.i, e.j);
        want.push_back(e);
    }
    int bad = 0;
    for (int stored = 0; stored < 2; ++stored)
        for (uint64_t seed = 0; seed < 6; ++seed) {
            std::vector<uint32_t> oi(n), oj(n), oc(n), od(n);
            uint32_t rounds = 0, lost[64], app[64], retries = 0;
            const int64_t m = emul_mst_call(common.data(), denom.data(), n, stored, 48, seed & 1, seed < 2 ? 0 : 64, seed, (int)(seed >> 2), oi.data(), oj.data(),
                                            oc.data(), od.data(), &rounds, lost, app, &retries);
            std::vector<E> got;
            for (int64_t e = 0; e < m; ++e) got.push_back(E{oi[e], oj[e], oc[e], od[e]});
            std::sort(got.begin(), got.end(), before);
            bool same = m == (int64_t)n - 1;
            for (size_t e = 0; same && e < got.size(); ++e) same = got[e].i == want[e].i && got[e].j == want[e].j && got[e].c == want[e].c && got[e].d == want[e].d;
            for (uint32_t r = 0; r < rounds; ++r) same = same && lost[r] == app[r];
            if (!same) { printf("stored %d seed %llu differs\n", stored, (unsigned long long)seed); bad = 1; }
        }
    printf(bad ? "FAILED\n" : "ok\n");
    return bad;
}
#endif
