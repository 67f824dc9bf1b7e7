// tests/emul/search_emul.cpp -- CPU emulator of the reference-set search (mhx_search.hip and the passes of mhx_dist.hip
// and mhx_triangle.hip it drives, test tool).  Runs the host+device functions of auriclass_amd/csrc/mhx_search.h,
// mhx_triangle.h and mhx_dist.h in the kernels' order, one work item after the other: ONE shift from the largest value of
// both sets, the split pass over the queries and over the references, then per block of the schedule the range pass and
// the finish pass of the block's geometry into block-local results, and the take-out as repeated search_insert of the
// candidates that pass the prefilter; at the end the host's exact distance rule.
// Not part of the product; built by tests/test_search_emulation.py with g++.
#include <cstdint>
#include <cstring>
#include <vector>
#include "../../auriclass_amd/csrc/mhx_search.h"

using namespace mhx;

extern "C" int emul_search_better(uint32_t ar, uint32_t ac, uint32_t ad, uint32_t br, uint32_t bc, uint32_t bd)
{
    return search_better(SearchHit{ar, ac, ad}, SearchHit{br, bc, bd}) ? 1 : 0;
}

// candidates order[0 .. n) of (ref, common, denom)[...] one after the other through search_insert; returns the list's length
extern "C" uint32_t emul_search_insert_many(const uint32_t *ref, const uint32_t *common, const uint32_t *denom, const uint32_t *order, uint32_t n,
                                            uint32_t top, uint32_t *out_ref, uint32_t *out_common, uint32_t *out_denom)
{
    std::vector<SearchHit> list(top);
    uint32_t m = 0;
    for (uint32_t i = 0; i < n; ++i) m = search_insert(list.data(), m, top, SearchHit{ref[order[i]], common[order[i]], denom[order[i]]});
    for (uint32_t i = 0; i < m; ++i) { out_ref[i] = list[i].ref; out_common[i] = list[i].common; out_denom[i] = list[i].denom; }
    return m;
}

extern "C" void emul_search_blocks(uint32_t nq, uint32_t nr, uint32_t qbatch, uint32_t *out, uint64_t cap, uint64_t *count)
{
    *count = search_blocks(nq, nr, qbatch);
    for (uint64_t b = 0; b < *count && b < cap; ++b) {
        const SearchBlock x = search_block(nq, nr, qbatch, b);
        out[4 * b] = x.r0; out[4 * b + 1] = x.nr; out[4 * b + 2] = x.q0; out[4 * b + 3] = x.nq;
    }
}

static void split_list(const uint64_t *v, uint32_t n, uint32_t shift, uint32_t per, uint32_t *offs)
{
    if (n == 0) { for (uint32_t p = 0; p < per; ++p) offs[p] = 0; return; }
    for (uint32_t i = 0; i < n; i += 2) { // one work item of dist_split_kernel
        const bool two = i + 1 < n;
        const uint32_t r0 = dist_range_of(v[i], shift), r1 = two ? dist_range_of(v[i + 1], shift) : r0;
        const uint32_t from = i == 0 ? 0u : dist_range_of(v[i - 1], shift) + 1u;
        dist_split_offsets(offs, per, i, n, two, from, r0, r1);
    }
}

// one pair of a block through the finish pass of the geometry R
static void finish_pair(const DistPair &x, uint32_t R, const uint32_t *wt, uint32_t cstride, uint32_t s, uint32_t &com, uint32_t &den)
{
    uint32_t uni = 0;
    com = 0;
    if (R < (uint32_t)kDistRanges) { // tri_finish_small_kernel
        uint32_t seg_uni[kDistSegs], seg_com[kDistSegs];
        for (uint32_t seg = 0; seg < (uint32_t)kDistSegs; ++seg) tri_segment_total(x, seg, R / kDistSegs, seg_uni[seg], seg_com[seg]);
        tri_finish_walk(x, seg_uni, seg_com, 1, R / kDistSegs, com, den);
    } else if (R == (uint32_t)kDistRanges) { // dist_finish_kernel
        constexpr uint32_t RPS = kDistRanges / kDistSegs;
        uint32_t seg_uni[kDistSegs], seg_com[kDistSegs];
        for (uint32_t seg = 0; seg < (uint32_t)kDistSegs; ++seg) {
            uint32_t c = 0;
            for (uint32_t p = seg * RPS; p < (seg + 1) * RPS; ++p) c += x.cp[(size_t)p * cstride];
            seg_com[seg] = c;
            seg_uni[seg] = dist_range_union(x, seg * RPS, (seg + 1) * RPS, c);
        }
        const uint32_t sg = dist_scan_totals(seg_uni, seg_com, 1, 0, kDistSegs, s, uni, com);
        if (sg == (uint32_t)kDistSegs) den = uni;
        else {
            const uint32_t p = dist_scan_ranges(x, sg * RPS, (sg + 1) * RPS, uni, com);
            dist_two_pointer(x, p, uni, com);
            den = s;
        }
    } else { // dist_finish_wide_kernel
        constexpr uint32_t kGroupWindows = kDistRanges / kDistWindowRanges;
        const uint32_t ngroups = R / kDistRanges;
        uint32_t grp_uni[kDistMaxWindows], grp_com[kDistMaxWindows];
        for (uint32_t grp = 0; grp < ngroups; ++grp) {
            uint32_t c = 0;
            for (uint32_t t = grp * kGroupWindows; t < (grp + 1) * kGroupWindows; ++t) c += wt[(size_t)t * cstride];
            grp_com[grp] = c;
            grp_uni[grp] = dist_range_union(x, grp * kDistRanges, (grp + 1) * kDistRanges, c);
        }
        const uint32_t cg = dist_scan_totals(grp_uni, grp_com, 1, 0, ngroups, s, uni, com);
        if (cg == ngroups) den = uni;
        else {
            const uint32_t cw = dist_scan_windows(x, wt, cstride, cg * kGroupWindows, (cg + 1) * kGroupWindows, uni, com);
            const uint32_t p = dist_scan_ranges(x, cw * kDistWindowRanges, (cw + 1) * kDistWindowRanges, uni, com);
            dist_two_pointer(x, p, uni, com);
            den = s;
        }
    }
}

// The whole call: nq query lists and nr reference lists, rows `stride` apart.  ranges: R forced (a power of two >= 16), 0 =
// tri_ranges of the longest list; qbatch: queries per block, 0 = tri_max_queries; reverse != 0: the blocks run last to first.
// Outputs as the host form of mhx_dist_search: [nq][top] best first, zero behind n_hits[q].  Returns 0; 1 when a block raised
// the overflow flag (the generic kernel's case: its candidates are missing); -1 without geometry; -2 bad arguments.
// stats (may be null): [0] ranges, [1] blocks, [2] flagged blocks, [3] candidates that passed the prefilter, [4] of those
// dropped by the host's exact rule.
extern "C" int emul_search(const uint64_t *q, const uint32_t *q_len, uint32_t nq, const uint64_t *r, const uint32_t *r_len, uint32_t nr,
                           uint32_t stride, uint32_t s, int k, uint32_t ranges, uint32_t qbatch, int reverse, double max_dist, uint32_t top,
                           uint32_t *hit_ref, uint32_t *hit_common, uint32_t *hit_denom, double *hit_dist, uint32_t *n_hits, uint32_t *stats)
{
    if (nq == 0 || nr == 0 || top < 1 || top > kSearchMaxTop) return -2;
    uint32_t longest = 0;
    for (uint32_t i = 0; i < nq; ++i) longest = q_len[i] > longest ? q_len[i] : longest;
    for (uint32_t i = 0; i < nr; ++i) longest = r_len[i] > longest ? r_len[i] : longest;
    const uint32_t R = ranges ? ranges : tri_ranges(longest), per = R + 1;
    if (R == 0) return -1;
    if (R < kTriMinRanges || (R & (R - 1)) != 0) return -2;
    if (qbatch == 0 || qbatch > tri_max_queries(R)) qbatch = tri_max_queries(R);
    if (qbatch > nq) qbatch = nq;
    // dist_shift_kernel over both sets, dist_split_kernel over each
    uint64_t gmax = 0;
    for (uint32_t i = 0; i < nq; ++i) if (q_len[i]) { const uint64_t v = q[(uint64_t)i * stride + q_len[i] - 1]; gmax = v > gmax ? v : gmax; }
    for (uint32_t i = 0; i < nr; ++i) if (r_len[i]) { const uint64_t v = r[(uint64_t)i * stride + r_len[i] - 1]; gmax = v > gmax ? v : gmax; }
    const uint32_t shift = dist_shift_for(gmax, R);
    std::vector<uint32_t> offq((size_t)nq * per, 0xDEADBEEFu), offr((size_t)nr * per, 0xDEADBEEFu);
    for (uint32_t i = 0; i < nq; ++i) split_list(q + (uint64_t)i * stride, q_len[i], shift, per, &offq[(size_t)i * per]);
    for (uint32_t i = 0; i < nr; ++i) split_list(r + (uint64_t)i * stride, r_len[i], shift, per, &offr[(size_t)i * per]);
    const double jmin = tri_jmin(max_dist, k);
    std::vector<SearchHit> lists((size_t)nq * top);
    std::vector<uint32_t> n(nq, 0);
    std::vector<unsigned long long> keys(kDistTableSlots);
    std::vector<uint32_t> masks(kDistMaskWords);
    const uint64_t nblocks = search_blocks(nq, nr, qbatch);
    uint32_t nflagged = 0, passed = 0, dropped = 0;
    for (uint64_t bi = 0; bi < nblocks; ++bi) {
        const SearchBlock b = search_block(nq, nr, qbatch, reverse ? nblocks - 1 - bi : bi);
        const uint64_t *bq = q + (uint64_t)b.q0 * stride, *br = r + (uint64_t)b.r0 * stride;
        const uint32_t *offs_q = &offq[(size_t)b.q0 * per], *offs_r = &offr[(size_t)b.r0 * per];
        const uint32_t nwords = (b.nr + 3) / 4, cstride = 4 * nwords;
        // dist_range_kernel<true> / dist_range_lane_kernel<true>: one workgroup per range, in the grid's order
        std::vector<uint32_t> cpart((size_t)b.nq * R * nwords, 0xA5A5A5A5u);
        uint32_t flag = 0;
        for (uint32_t block = 0; block < R; ++block) {
            const uint32_t p = dist_range_of_block(block, R);
            dist_table_clear(keys.data(), masks.data(), 0, 1);
            uint32_t ndistinct = 0;
            for (uint32_t ri = 0; ri < b.nr; ++ri) {
                const uint32_t lo = offs_r[(size_t)ri * per + p], hi = offs_r[(size_t)ri * per + p + 1];
                if (hi - lo > kDistSliceLimit) { ndistinct += (uint32_t)kDistTableSlots; continue; }
                for (uint32_t i = lo; i < hi; ++i) ndistinct += dist_table_insert_plain(keys.data(), masks.data(), br[(uint64_t)ri * stride + i], ri);
            }
            if (ndistinct > kDistTableLimit) { flag |= 1u; continue; }
            for (uint32_t qi = 0; qi < b.nq; ++qi) {
                const uint32_t lo = offs_q[(size_t)qi * per + p], hi = offs_q[(size_t)qi * per + p + 1];
                if (hi - lo > kDistSliceLimit) { flag |= 1u; continue; }
                uint32_t acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
                for (uint32_t i = lo; i < hi; ++i) {
                    const uint32_t m = dist_table_probe(keys.data(), masks.data(), bq[(uint64_t)qi * stride + i]);
                    for (int j = 0; j < 8; ++j)
                        if (j < (int)nwords) acc[j] += dist_spread4(m, j);
                }
                for (uint32_t j = 0; j < nwords; ++j) cpart[((size_t)qi * R + p) * nwords + j] = acc[j];
            }
        }
        if (flag) { ++nflagged; continue; } // the finish and the take-out return at once
        const uint8_t *cbytes = reinterpret_cast<const uint8_t *>(cpart.data());
        const uint32_t nwin = R / kDistWindowRanges;
        std::vector<uint32_t> wtot;
        if (R > (uint32_t)kDistRanges) { // dist_window_kernel
            wtot.assign((size_t)b.nq * nwin * cstride, 0);
            for (uint32_t qw = 0; qw < b.nq * nwin; ++qw)
                for (uint32_t j = 0; j < nwords; ++j)
                    dist_window_sum(cpart.data() + (size_t)qw * kDistWindowRanges * nwords + j, nwords, kDistWindowRanges, &wtot[((size_t)qw * nwords + j) * 4]);
        }
        std::vector<uint32_t> loc_c((size_t)b.nq * kTriSlice, 0xFFFFFFFFu), loc_d((size_t)b.nq * kTriSlice, 0xFFFFFFFFu);
        for (uint32_t qi = 0; qi < b.nq; ++qi)
            for (uint32_t ri = 0; ri < b.nr; ++ri) {
                const DistPair x{cbytes + (size_t)qi * R * cstride + ri, cstride, offs_q + (size_t)qi * per, offs_r + (size_t)ri * per,
                                 br + (uint64_t)ri * stride, bq + (uint64_t)qi * stride, s};
                finish_pair(x, R, wtot.empty() ? nullptr : &wtot[(size_t)qi * nwin * cstride + ri], cstride, s, loc_c[(size_t)qi * kTriSlice + ri],
                            loc_d[(size_t)qi * kTriSlice + ri]);
            }
        // search_take_kernel: one wave per query; the candidates that pass the prefilter, lowest lane first
        for (uint32_t ql = 0; ql < b.nq; ++ql)
            for (uint32_t rl = 0; rl < b.nr; ++rl) {
                const uint32_t c = loc_c[(size_t)ql * kTriSlice + rl], d = loc_d[(size_t)ql * kTriSlice + rl];
                if (!tri_keep(c, d, jmin)) continue;
                ++passed;
                const uint32_t gq = b.q0 + ql;
                n[gq] = search_insert(&lists[(size_t)gq * top], n[gq], top, SearchHit{b.r0 + rl, c, d});
            }
    }
    // the host: the exact rule on the lists
    for (uint32_t i = 0; i < nq; ++i) {
        uint32_t m = 0;
        for (uint32_t t = 0; t < top; ++t) {
            const size_t at = (size_t)i * top + t;
            hit_ref[at] = hit_common[at] = hit_denom[at] = 0;
            hit_dist[at] = 0.0;
        }
        for (uint32_t t = 0; t < n[i]; ++t) {
            const SearchHit &h = lists[(size_t)i * top + t];
            const double d = tri_distance(h.common, h.denom, k);
            if (!(d <= max_dist)) { ++dropped; continue; }
            const size_t at = (size_t)i * top + m++;
            hit_ref[at] = h.ref; hit_common[at] = h.common; hit_denom[at] = h.denom; hit_dist[at] = d;
        }
        n_hits[i] = m;
    }
    if (stats) { stats[0] = R; stats[1] = (uint32_t)nblocks; stats[2] = nflagged; stats[3] = passed; stats[4] = dropped; }
    return nflagged ? 1 : 0;
}

#ifdef SEARCH_EMUL_MAIN
// stand-alone run for a host sanitizer build: a small pair of sets through every finish form, batch size and block order
#include <cstdio>
int main()
{
    const uint32_t nq = 23, nr = 70, stride = 304, s = 300, top = 7;
    std::vector<uint64_t> rows((size_t)(nq + nr) * stride, 0);
    std::vector<uint32_t> len(nq + nr);
    uint64_t x = 88172645463325252ull;
    for (uint32_t i = 0; i < nq + nr; ++i) {
        len[i] = i == 3 || i == 30 ? 0 : (i == 4 ? 17 : s);
        uint64_t v = 0;
        for (uint32_t j = 0; j < len[i]; ++j) {
            x ^= x << 13; x ^= x >> 7; x ^= x << 17;
            v += 1 + (x >> 9) % (0xFFFFFFFFFFFFFFFFull / (s + 1));
            rows[(size_t)i * stride + j] = i % 5 == 1 ? rows[(size_t)(i - 1) * stride + j] : v; // every fifth list repeats its neighbour
        }
        if (i % 5 == 1) len[i] = len[i - 1];
    }
    for (uint32_t j = 0; j < len[nq + 12]; ++j) rows[(size_t)2 * stride + j] = rows[(size_t)(nq + 12) * stride + j]; // query 2 = reference 12, which reference 13 repeats
    len[2] = len[nq + 12];
    const uint64_t *q = rows.data(), *r = rows.data() + (size_t)nq * stride;
    const size_t cells = (size_t)nq * top;
    std::vector<uint32_t> ref0(cells), c0(cells), d0(cells), n0(nq), ref(cells), c(cells), d(cells), n(nq);
    std::vector<double> x0(cells), xx(cells);
    int bad = 0;
    const uint32_t forms[][3] = {{16, 0, 0}, {64, 5, 0}, {64, 5, 1}, {512, 0, 1}, {1024, 9, 0}, {2048, 0, 0}};
    for (size_t f = 0; f < sizeof forms / sizeof forms[0]; ++f) {
        uint32_t stats[5];
        const int rc = f ? emul_search(q, len.data(), nq, r, len.data() + nq, nr, stride, s, 21, forms[f][0], forms[f][1], (int)forms[f][2], 0.3, top, ref.data(), c.data(), d.data(), xx.data(), n.data(), stats)
                         : emul_search(q, len.data(), nq, r, len.data() + nq, nr, stride, s, 21, forms[f][0], forms[f][1], (int)forms[f][2], 0.3, top, ref0.data(), c0.data(), d0.data(), x0.data(), n0.data(), stats);
        if (rc != 0) { printf("R = %u: rc %d\n", forms[f][0], rc); bad = 1; }
        if (f && (ref != ref0 || c != c0 || d != d0 || n != n0 || xx != x0)) { printf("form %zu differs from form 0\n", f); bad = 1; }
    }
    if (n0[2] < 2 || ref0[2 * top] != 12 || ref0[2 * top + 1] != 13) { printf("the duplicate references of query 2 are not its first hits in index order\n"); bad = 1; }
    printf(bad ? "FAILED\n" : "ok\n");
    return bad;
}
#endif
