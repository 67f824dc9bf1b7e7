// tests/emul/contain_winner_emul.cpp -- CPU emulator of the winner-take-all containment kernels (mhx_contain_winner.hip, test
// tool).  Runs the host+device functions of auriclass_amd/csrc/mhx_contain_winner.h themselves: the plain counts of every pair
// (contain_emul.cpp's pair walk), then contain_claim_kernel pair by pair in the ORDER THE CALLER GIVES -- a word must end at
// the best-ranked proposer whatever the order of arrival --, each pair as a workgroup of `shares` threads in descending
// order, then contain_tally_kernel word by word.  Stand-alone too: compiled with -DCONTAIN_WINNER_EMUL_MAIN it has a main()
// that runs a crafted set in three orders against a brute force, for a sanitizer run.
// Not part of the product; built by tests/test_contain_winner_emulation.py with g++.
#include "contain_emul.cpp"
#include "../../auriclass_amd/csrc/mhx_contain_winner.h"

extern "C" uint32_t emul_contain_claim_threads() { return kContainClaimThreads; }

// the comparator alone, over one query's row of counts
extern "C" int emul_contain_ranks_before(const uint32_t *shared, const uint32_t *n_ref, const uint64_t *ref_length, uint32_t a, uint32_t b)
{
    return contain_ranks_before(ContainRanks{shared, n_ref, ref_length}, a, b) ? 1 : 0;
}

// The whole call over rows `stride` apart.  order[nq * nr]: the pairs (q * nr + r) in the order in which their workgroups run;
// every pair must appear once.  won / shared / n_qry / n_ref [nq][nr].  Returns the pairs the claim pass walked, or ~0 when
// `order` is not a permutation or a word index leaves the query's list.
extern "C" uint64_t emul_contain_winner(const uint64_t *q, const uint32_t *q_len, uint32_t nq, uint32_t s_q, const uint64_t *r, const uint32_t *r_len, uint32_t nr,
                                        uint32_t s_r, uint32_t stride, const uint64_t *ref_length, const uint32_t *order, uint32_t shares, uint32_t *won,
                                        uint32_t *shared, uint32_t *n_qry, uint32_t *n_ref)
{
    std::vector<uint32_t> q_eff(nq), r_eff(nr);
    std::vector<uint64_t> q_bound(nq), r_bound(nr);
    emul_contain_bounds(q, q_len, nq, stride, s_q, q_eff.data(), q_bound.data());
    emul_contain_bounds(r, r_len, nr, stride, s_r, r_eff.data(), r_bound.data());
    for (uint32_t qi = 0; qi < nq; ++qi)
        for (uint32_t ri = 0; ri < nr; ++ri) {
            const size_t at = (size_t)qi * nr + ri;
            emul_contain_pair(r + (uint64_t)ri * stride, r_eff[ri], r_bound[ri], q + (uint64_t)qi * stride, q_eff[qi], q_bound[qi], 3, &shared[at], &n_qry[at], &n_ref[at]);
        }
    const uint32_t width = stride < s_q ? stride : s_q; // the engine's: every effective query length fits
    std::vector<uint32_t> words((size_t)nq * width, 0);
    std::vector<uint8_t> seen((size_t)nq * nr, 0);
    uint64_t walked = 0;
    for (size_t t = 0; t < (size_t)nq * nr; ++t) { // contain_claim_kernel, one workgroup after the other
        const uint32_t pair = order[t];
        if (pair >= nq * nr || seen[pair]) return ~0ull;
        seen[pair] = 1;
        const uint32_t qi = pair / nr, ri = pair % nr;
        const size_t row = (size_t)qi * nr;
        if (shared[row + ri] == 0) continue;
        if (n_qry[row + ri] > width) return ~0ull;
        const ContainRanks k{shared + row, n_ref + row, ref_length};
        uint32_t proposed = 0;
        for (uint32_t share = shares; share-- > 0;)
            proposed += contain_claim_walk(r + (uint64_t)ri * stride, n_ref[row + ri], q + (uint64_t)qi * stride, n_qry[row + ri], shares, share,
                                           &words[(size_t)qi * width], k, ri);
        if (proposed != shared[row + ri]) return ~0ull; // a pair proposes every value it found, once
        ++walked;
    }
    for (size_t i = 0; i < (size_t)nq * nr; ++i) won[i] = 0;
    for (size_t id = words.size(); id-- > 0;) contain_tally(words[id], won + (size_t)(id / width) * nr); // contain_tally_kernel
    return walked;
}

#ifdef CONTAIN_WINNER_EMUL_MAIN
#include <cstdio>
#include <map>
// a crafted set in forward, reverse and a shuffled order against a brute force of the rule: what a sanitizer build runs
int main()
{
    const uint32_t stride = 32, s_q = 24, s_r = 12, nq = 4, nr = 6;
    std::vector<uint64_t> q((size_t)nq * stride, ~0ull), r((size_t)nr * stride, 0);
    std::vector<uint32_t> ql(nq), rl(nr);
    uint64_t x = 88172645463325252ull;
    auto next = [&]() { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; };
    for (uint32_t i = 0; i < nq; ++i) {
        ql[i] = i == 2 ? 0 : (i == 3 ? 9 : s_q);
        std::vector<uint64_t> v(ql[i]);
        for (auto &e : v) e = next() | 1;
        std::sort(v.begin(), v.end());
        if (i == 1 && !v.empty()) v.back() = ~0ull;
        for (uint32_t j = 0; j < ql[i]; ++j) q[(size_t)i * stride + j] = v[j];
    }
    for (uint32_t i = 0; i < nr; ++i) { // subsets of the queries' lists: references 0 and 1 are copies, 5 ends in 2^64 - 1
        const uint32_t src = i == 5 ? 1 : (i == 4 ? 3 : 0), step = i < 2 || i == 5 ? 1 : i, from = i == 5 ? s_q - 5 : 0;
        uint32_t n = 0;
        for (uint32_t j = from; j < ql[src] && n < (i == 3 ? 5u : s_r); j += step) r[(size_t)i * stride + n++] = q[(size_t)src * stride + j];
        rl[i] = n;
    }
    const uint64_t lengths[nr] = {7, 9, 7, 7, 7, 7};
    int bad = 0;
    for (int mode = 0; mode < 3; ++mode) {
        std::vector<uint32_t> order(nq * nr);
        for (uint32_t t = 0; t < nq * nr; ++t) order[t] = mode == 0 ? t : (mode == 1 ? nq * nr - 1 - t : (t * 7 + 5) % (nq * nr));
        std::vector<uint32_t> won(nq * nr), sh(nq * nr), a(nq * nr), b(nq * nr);
        const uint64_t walked = emul_contain_winner(q.data(), ql.data(), nq, s_q, r.data(), rl.data(), nr, s_r, stride, mode == 2 ? lengths : nullptr, order.data(),
                                                    mode == 0 ? 256 : 3, won.data(), sh.data(), a.data(), b.data());
        if (walked == ~0ull) { ++bad; continue; }
        for (uint32_t qi = 0; qi < nq; ++qi) { // the rule by brute force
            std::map<uint64_t, uint32_t> best;
            const ContainRanks k{&sh[qi * nr], &b[qi * nr], mode == 2 ? lengths : nullptr};
            for (uint32_t ri = 0; ri < nr; ++ri)
                for (uint32_t i = 0; i < b[qi * nr + ri]; ++i)
                    for (uint32_t j = 0; j < a[qi * nr + ri]; ++j)
                        if (r[(size_t)ri * stride + i] == q[(size_t)qi * stride + j]) {
                            auto it = best.find(q[(size_t)qi * stride + j]);
                            if (it == best.end()) best[q[(size_t)qi * stride + j]] = ri;
                            else if (it->second != ri && contain_ranks_before(k, ri, it->second)) it->second = ri;
                        }
            std::vector<uint32_t> want(nr, 0);
            for (auto &e : best) ++want[e.second];
            for (uint32_t ri = 0; ri < nr; ++ri) if (want[ri] != won[qi * nr + ri]) ++bad;
        }
    }
    printf("contain_winner_emul: %d mismatches\n", bad);
    return bad != 0;
}
#endif
