// tests/emul/contain_emul.cpp -- CPU emulator of the containment kernels (mhx_contain.hip, test tool).  Runs the host+device
// functions of auriclass_amd/csrc/mhx_contain.h themselves: the bounds list by list, the pair walk share by share as a
// workgroup of `shares` threads runs it, and the finish pass of a (query batch, reference slice) block over range data that
// the emulated split and range passes of dist_emul.cpp's text leave (split_list, the table build and the probe of
// mhx_dist.h) at any number of ranges.  Shares and segments run in descending order: nothing may depend on the order.
// Stand-alone too: compiled with -DCONTAIN_EMUL_MAIN it has a main() that runs a few crafted pairs, for a sanitizer run.
// Not part of the product; built by tests/test_contain_emulation.py with g++.
#include <algorithm>
#include "dist_emul.cpp"
#include "../../auriclass_amd/csrc/mhx_contain.h"

extern "C" uint32_t emul_contain_pair_threads() { return kContainPairThreads; }

// contain_bounds_kernel over one set
extern "C" void emul_contain_bounds(const uint64_t *rows, const uint32_t *len, uint32_t n, uint32_t stride, uint32_t s, uint32_t *eff, uint64_t *bound)
{
    for (uint32_t i = n; i-- > 0;) {
        eff[i] = contain_eff_len(len[i], stride, s);
        bound[i] = contain_bound(rows + (uint64_t)i * stride, eff[i], s);
    }
}

// contain_pairs_kernel for one pair with a workgroup of `shares` threads: A the reference's list, B the query's
extern "C" void emul_contain_pair(const uint64_t *A, uint32_t effA, uint64_t boundA, const uint64_t *B, uint32_t effB, uint64_t boundB, uint32_t shares,
                                  uint32_t *shared, uint32_t *n_qry, uint32_t *n_ref)
{
    const uint64_t tau = contain_tau(boundB, boundA);
    const uint32_t nA = contain_prefix(A, effA, tau), nB = contain_prefix(B, effB, tau);
    uint32_t c = 0;
    for (uint32_t t = shares; t-- > 0;) c += contain_walk_shared(A, nA, B, nB, shares, t);
    *shared = c;
    *n_qry = nB;
    *n_ref = nA;
}

// One (query batch, reference slice) block at R ranges (a power of two, 16 .. kDistRanges), nr <= 32, rows `stride` apart:
// bounds, shift, split, range pass, contain_finish_kernel.  Returns 0 and fills shared / n_qry / n_ref [nq][nr]; 1 when the
// block's flag went up (the pair kernel's case: nothing is written).
extern "C" int emul_contain_block(const uint64_t *q, const uint32_t *q_len, uint32_t nq, uint32_t s_q, const uint64_t *r, const uint32_t *r_len, uint32_t nr,
                                  uint32_t s_r, uint32_t stride, uint32_t R, uint32_t *shared, uint32_t *n_qry, uint32_t *n_ref)
{
    if (nr == 0 || nr > 32 || nq == 0 || R < 16 || R > (uint32_t)kDistRanges || (R & (R - 1))) return -2;
    std::vector<uint32_t> q_eff(nq), r_eff(nr);
    std::vector<uint64_t> q_bound(nq), r_bound(nr);
    emul_contain_bounds(q, q_len, nq, stride, s_q, q_eff.data(), q_bound.data());
    emul_contain_bounds(r, r_len, nr, stride, s_r, r_eff.data(), r_bound.data());
    const uint32_t per = R + 1;
    // dist_shift_kernel over the effective lists
    uint64_t gmax = 0;
    for (uint32_t i = 0; i < nq; ++i) if (q_eff[i]) { const uint64_t v = q[(uint64_t)i * stride + q_eff[i] - 1]; gmax = v > gmax ? v : gmax; }
    for (uint32_t i = 0; i < nr; ++i) if (r_eff[i]) { const uint64_t v = r[(uint64_t)i * stride + r_eff[i] - 1]; gmax = v > gmax ? v : gmax; }
    const uint32_t shift = dist_shift_for(gmax, R);
    // dist_split_kernel
    std::vector<uint32_t> offs_q((size_t)nq * per, 0xDEADBEEFu), offs_r((size_t)nr * per, 0xDEADBEEFu);
    for (uint32_t i = 0; i < nq; ++i) split_list(q + (uint64_t)i * stride, q_eff[i], shift, per, &offs_q[(size_t)i * per]);
    for (uint32_t i = 0; i < nr; ++i) split_list(r + (uint64_t)i * stride, r_eff[i], shift, per, &offs_r[(size_t)i * per]);
    // dist_range_kernel<true> / dist_range_lane_kernel<true>: one workgroup per range, in the grid's order
    const uint32_t nwords = (nr + 3) / 4, cstride = 4 * nwords;
    std::vector<uint32_t> cpart((size_t)nq * R * nwords, 0xA5A5A5A5u);
    std::vector<unsigned long long> keys(kDistTableSlots);
    std::vector<uint32_t> masks(kDistMaskWords);
    uint32_t flag = 0;
    for (uint32_t block = 0; block < R; ++block) {
        const uint32_t p = dist_range_of_block(block, R);
        dist_table_clear(keys.data(), masks.data(), 0, 1);
        uint32_t ndistinct = 0;
        for (uint32_t ri = 0; ri < nr; ++ri) {
            const uint32_t b = offs_r[(size_t)ri * per + p], e = offs_r[(size_t)ri * per + p + 1];
            if (e - b > kDistSliceLimit) { ndistinct += (uint32_t)kDistTableSlots; continue; }
            for (uint32_t i = b; i < e; ++i) ndistinct += dist_table_insert_plain(keys.data(), masks.data(), r[(uint64_t)ri * stride + i], ri);
        }
        if (ndistinct > kDistTableLimit) { flag |= 1u; continue; }
        for (uint32_t qi = 0; qi < nq; ++qi) {
            const uint32_t b = offs_q[(size_t)qi * per + p], e = offs_q[(size_t)qi * per + p + 1];
            if (e - b > kDistSliceLimit) { flag |= 1u; continue; }
            uint32_t acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            for (uint32_t i = b; i < e; ++i) {
                const uint32_t m = dist_table_probe(keys.data(), masks.data(), q[(uint64_t)qi * stride + i]);
                for (int j = 0; j < 8; ++j)
                    if (j < (int)nwords) acc[j] += dist_spread4(m, j);
            }
            for (uint32_t j = 0; j < nwords; ++j) cpart[((size_t)qi * R + p) * nwords + j] = acc[j];
        }
    }
    if (flag) return 1;
    // contain_finish_kernel
    const uint8_t *cbytes = reinterpret_cast<const uint8_t *>(cpart.data());
    const uint32_t rps = R / kDistSegs;
    for (uint32_t qi = nq; qi-- > 0;)
        for (uint32_t ri = nr; ri-- > 0;) {
            const DistPair x{cbytes + (size_t)qi * R * cstride + ri, cstride, &offs_q[(size_t)qi * per], &offs_r[(size_t)ri * per],
                             r + (uint64_t)ri * stride, q + (uint64_t)qi * stride, 0u};
            const uint64_t tau = contain_tau(q_bound[qi], r_bound[ri]);
            const uint32_t p_tau = contain_tau_range(tau, shift, R);
            uint32_t seg_shared[kDistSegs];
            for (uint32_t seg = kDistSegs; seg-- > 0;) seg_shared[seg] = contain_segment_shared(x, seg, rps, p_tau);
            const size_t out = (size_t)qi * nr + ri;
            contain_finish_walk(x, seg_shared, 1, p_tau, tau, shared[out], n_qry[out], n_ref[out]);
        }
    return 0;
}

#ifdef CONTAIN_EMUL_MAIN
#include <cstdio>
// a few crafted pairs through every function, checked against a brute force: what a sanitizer build runs
int main()
{
    const uint32_t stride = 48, s_q = 40, s_r = 24, nq = 5, nr = 3;
    std::vector<uint64_t> q((size_t)nq * stride, ~0ull), r((size_t)nr * stride, 0);
    std::vector<uint32_t> ql(nq), rl(nr);
    uint64_t x = 88172645463325252ull;
    auto next = [&]() { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; };
    for (uint32_t i = 0; i < nq; ++i) {
        ql[i] = i == 2 ? 0 : (i == 3 ? 17 : s_q);
        std::vector<uint64_t> v(ql[i]);
        for (auto &e : v) e = next() | 1;
        std::sort(v.begin(), v.end());
        if (i == 4 && !v.empty()) v.back() = ~0ull;
        for (uint32_t j = 0; j < ql[i]; ++j) q[(size_t)i * stride + j] = v[j];
    }
    for (uint32_t i = 0; i < nr; ++i) {
        rl[i] = i == 1 ? 9 : s_r;
        for (uint32_t j = 0; j < rl[i]; ++j) r[(size_t)i * stride + j] = q[(size_t)(i == 2 ? 4 : 0) * stride + 2 * j / (i + 1)];
        std::sort(r.begin() + (size_t)i * stride, r.begin() + (size_t)i * stride + rl[i]);
        rl[i] = (uint32_t)(std::unique(r.begin() + (size_t)i * stride, r.begin() + (size_t)i * stride + rl[i]) - (r.begin() + (size_t)i * stride));
    }
    int bad = 0;
    for (uint32_t R : {16u, 64u, 1024u}) {
        std::vector<uint32_t> sh((size_t)nq * nr), a(sh.size()), b(sh.size());
        if (emul_contain_block(q.data(), ql.data(), nq, s_q, r.data(), rl.data(), nr, s_r, stride, R, sh.data(), a.data(), b.data()) != 0) { ++bad; continue; }
        std::vector<uint32_t> qe(nq), re(nr);
        std::vector<uint64_t> qb(nq), rb(nr);
        emul_contain_bounds(q.data(), ql.data(), nq, stride, s_q, qe.data(), qb.data());
        emul_contain_bounds(r.data(), rl.data(), nr, stride, s_r, re.data(), rb.data());
        for (uint32_t i = 0; i < nq; ++i)
            for (uint32_t j = 0; j < nr; ++j)
                for (uint32_t shares : {1u, 3u, 64u, 256u}) {
                    uint32_t c, nq_, nr_;
                    emul_contain_pair(&r[(size_t)j * stride], re[j], rb[j], &q[(size_t)i * stride], qe[i], qb[i], shares, &c, &nq_, &nr_);
                    if (c != sh[(size_t)i * nr + j] || nq_ != a[(size_t)i * nr + j] || nr_ != b[(size_t)i * nr + j]) ++bad;
                }
    }
    printf("contain_emul: %d mismatches\n", bad);
    return bad != 0;
}
#endif
