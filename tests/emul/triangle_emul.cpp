// tests/emul/triangle_emul.cpp -- CPU emulator of the all-pairs path within one sketch set (mhx_triangle.hip and the passes
// of mhx_dist.hip it drives, test tool).  Runs the host+device functions of auriclass_amd/csrc/mhx_triangle.h and
// mhx_dist.h in the kernels' order, one work item after the other: the shift from the largest value, the split pass ONCE
// over all lists into one offsets table, then per block of the schedule the range pass (table build, probe, byte
// counters) and the finish pass -- the short-range walk below 1024 ranges, the base walk at 1024, window totals and the
// wide walk above -- into block-local results, and the scatter of the pairs that count into the packed triangle.
// Not part of the product; built by tests/test_triangle_emulation.py with g++.
#include <cstdint>
#include <cstring>
#include <vector>
#include "../../auriclass_amd/csrc/mhx_triangle.h"

using namespace mhx;

extern "C" uint64_t emul_tri_index(uint32_t i, uint32_t j) { return tri_index(i, j); }
extern "C" uint32_t emul_tri_ranges(uint64_t longest) { return tri_ranges(longest); }
extern "C" uint32_t emul_tri_ranges_dist(uint64_t longest) { return tri_ranges_dist(longest); }
extern "C" uint32_t emul_tri_max_queries(uint32_t ranges) { return tri_max_queries(ranges); }
extern "C" double emul_tri_jmin(double max_dist, int k) { return tri_jmin(max_dist, k); }
extern "C" double emul_tri_distance(uint32_t common, uint32_t denom, int k) { return tri_distance(common, denom, k); }
extern "C" void emul_tri_keep_many(const uint32_t *common, const uint32_t *denom, uint64_t n, double jmin, uint8_t *out)
{
    for (uint64_t i = 0; i < n; ++i) out[i] = tri_keep(common[i], denom[i], jmin) ? 1 : 0;
}

// the blocks of the schedule, four words each (r0, nr, q0, nq); returns their number (only the first `cap` are stored)
extern "C" uint32_t emul_tri_blocks(uint32_t n, uint32_t qbatch, uint32_t *out, uint32_t cap)
{
    uint32_t count = 0;
    TriBlock b;
    for (bool more = tri_first_block(n, qbatch, b); more; more = tri_next_block(n, qbatch, b)) {
        if (count < cap) { out[4 * count] = b.r0; out[4 * count + 1] = b.nr; out[4 * count + 2] = b.q0; out[4 * count + 3] = b.nq; }
        ++count;
    }
    return count;
}
extern "C" int emul_tri_pair_counts(uint32_t r0, uint32_t nr, uint32_t q0, uint32_t nq, uint32_t ql, uint32_t rl)
{
    const TriBlock b{r0, nr, q0, nq};
    return tri_pair_counts(b, ql, rl) ? 1 : 0;
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

// The whole call: n lists, rows `stride` apart.  ranges: R forced (a power of two >= 16), 0 = tri_ranges of the longest list;
// qbatch: queries per block, 0 = tri_max_queries.  common / denom: packed [n (n - 1) / 2].  Returns 0; 1 when a block raised
// the overflow flag (the generic kernel's case; its pairs are left untouched); -1 without geometry; -4 when a packed cell
// was written twice.  stats (may be null): [0] ranges, [1] longest slice of any list, [2] most distinct keys in one range,
// [3] blocks, [4] flagged blocks, [5] pairs computed and thrown away.
extern "C" int emul_triangle(const uint64_t *rows, const uint32_t *len, uint32_t n, uint32_t stride, uint32_t s, uint32_t ranges,
                             uint32_t qbatch, uint32_t *common, uint32_t *denom, uint32_t *stats)
{
    if (n < 2) return -2;
    uint32_t longest = 0;
    for (uint32_t i = 0; i < n; ++i) longest = len[i] > longest ? len[i] : longest;
    const uint32_t R = ranges ? ranges : tri_ranges(longest), per = R + 1;
    if (R == 0) return -1;
    if (R < kTriMinRanges || (R & (R - 1)) != 0) return -2;
    if (qbatch == 0 || qbatch > tri_max_queries(R)) qbatch = tri_max_queries(R);
    // dist_shift_kernel + dist_split_kernel, once over all lists
    uint64_t gmax = 0;
    for (uint32_t i = 0; i < n; ++i) if (len[i]) { const uint64_t v = rows[(uint64_t)i * stride + len[i] - 1]; gmax = v > gmax ? v : gmax; }
    const uint32_t shift = dist_shift_for(gmax, R);
    std::vector<uint32_t> offs((size_t)n * per, 0xDEADBEEFu);
    for (uint32_t i = 0; i < n; ++i) split_list(rows + (uint64_t)i * stride, len[i], shift, per, &offs[(size_t)i * per]);
    const uint64_t npairs = (uint64_t)n * (n - 1) / 2;
    std::vector<uint8_t> written(npairs, 0);
    std::vector<unsigned long long> keys(kDistTableSlots);
    std::vector<uint32_t> masks(kDistMaskWords);
    uint32_t longest_slice = 0, most_keys = 0, nblocks = 0, nflagged = 0, wasted = 0;
    TriBlock b;
    for (bool more = tri_first_block(n, qbatch, b); more; more = tri_next_block(n, qbatch, b)) {
        ++nblocks;
        const uint64_t *q = rows + (uint64_t)b.q0 * stride, *r = rows + (uint64_t)b.r0 * stride;
        const uint32_t *offs_q = &offs[(size_t)b.q0 * per], *offs_r = &offs[(size_t)b.r0 * per];
        const uint32_t nq = b.nq, nr = b.nr, nwords = (nr + 3) / 4, cstride = 4 * nwords;
        // dist_range_kernel<true> / dist_range_lane_kernel<true>: one workgroup per range, in the grid's order
        std::vector<uint32_t> cpart((size_t)nq * R * nwords, 0xA5A5A5A5u);
        uint32_t flag = 0;
        for (uint32_t block = 0; block < R; ++block) {
            const uint32_t p = dist_range_of_block(block, R);
            if (p >= R) return -3;
            dist_table_clear(keys.data(), masks.data(), 0, 1);
            uint32_t ndistinct = 0;
            for (uint32_t ri = 0; ri < nr; ++ri) {
                const uint32_t lo = offs_r[(size_t)ri * per + p], hi = offs_r[(size_t)ri * per + p + 1];
                longest_slice = hi - lo > longest_slice ? hi - lo : longest_slice;
                if (hi - lo > kDistSliceLimit) { ndistinct += (uint32_t)kDistTableSlots; continue; } // not inserted: counts as a table overflow
                for (uint32_t i = lo; i < hi; ++i) ndistinct += dist_table_insert_plain(keys.data(), masks.data(), r[(uint64_t)ri * stride + i], ri);
            }
            most_keys = ndistinct > most_keys ? ndistinct : most_keys;
            if (ndistinct > kDistTableLimit) { flag |= 1u; continue; }
            for (uint32_t qi = 0; qi < nq; ++qi) {
                const uint32_t lo = offs_q[(size_t)qi * per + p], hi = offs_q[(size_t)qi * per + p + 1];
                longest_slice = hi - lo > longest_slice ? hi - lo : longest_slice;
                if (hi - lo > kDistSliceLimit) { flag |= 1u; continue; }
                uint32_t acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
                for (uint32_t i = lo; i < hi; ++i) {
                    const uint32_t m = dist_table_probe(keys.data(), masks.data(), q[(uint64_t)qi * stride + i]);
                    for (int j = 0; j < 8; ++j)
                        if (j < (int)nwords) acc[j] += dist_spread4(m, j);
                }
                for (uint32_t j = 0; j < nwords; ++j) cpart[((size_t)qi * R + p) * nwords + j] = acc[j];
            }
        }
        if (flag) { ++nflagged; continue; } // every finish kernel and the scatter return at once
        const uint8_t *cbytes = reinterpret_cast<const uint8_t *>(cpart.data());
        std::vector<uint32_t> loc_c((size_t)nq * kTriSlice, 0xFFFFFFFFu), loc_d((size_t)nq * kTriSlice, 0xFFFFFFFFu);
        // dist_window_kernel (R >= 2048)
        const uint32_t nwin = R / kDistWindowRanges;
        std::vector<uint32_t> wtot;
        if (R > (uint32_t)kDistRanges) {
            wtot.assign((size_t)nq * nwin * cstride, 0);
            for (uint32_t qw = 0; qw < nq * nwin; ++qw)
                for (uint32_t j = 0; j < nwords; ++j)
                    dist_window_sum(cpart.data() + (size_t)qw * kDistWindowRanges * nwords + j, nwords, kDistWindowRanges, &wtot[((size_t)qw * nwords + j) * 4]);
        }
        for (uint32_t qi = 0; qi < nq; ++qi)
            for (uint32_t ri = 0; ri < nr; ++ri) {
                const DistPair x{cbytes + (size_t)qi * R * cstride + ri, cstride, offs_q + (size_t)qi * per, offs_r + (size_t)ri * per,
                                 r + (uint64_t)ri * stride, q + (uint64_t)qi * stride, s};
                uint32_t uni = 0, com = 0, den;
                if (R < (uint32_t)kDistRanges) { // tri_finish_small_kernel: 16 threads sum a segment each, one walks
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
                    const uint32_t *wt = &wtot[(size_t)qi * nwin * cstride + ri];
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
                loc_c[(size_t)qi * kTriSlice + ri] = com;
                loc_d[(size_t)qi * kTriSlice + ri] = den;
            }
        // tri_scatter_kernel: one work item per cell of the block-local arrays
        for (uint32_t id = 0; id < nq * kTriSlice; ++id) {
            const uint32_t ql = id / kTriSlice, rl = id % kTriSlice;
            if (!tri_pair_counts(b, ql, rl)) { if (rl < nr) ++wasted; continue; }
            const uint64_t at = tri_index(b.q0 + ql, b.r0 + rl);
            if (at >= npairs || written[at]) return -4;
            written[at] = 1;
            common[at] = loc_c[id];
            denom[at] = loc_d[id];
        }
    }
    if (stats) { stats[0] = R; stats[1] = longest_slice; stats[2] = most_keys; stats[3] = nblocks; stats[4] = nflagged; stats[5] = wasted; }
    return nflagged ? 1 : 0;
}

#ifdef TRIANGLE_EMUL_MAIN
// stand-alone run for a host sanitizer build: a small set through every finish form
#include <cstdio>
int main()
{
    const uint32_t n = 40, stride = 304, s = 300;
    std::vector<uint64_t> rows((size_t)n * stride, 0);
    std::vector<uint32_t> len(n);
    uint64_t x = 88172645463325252ull;
    for (uint32_t i = 0; i < n; ++i) {
        len[i] = i == 3 ? 0 : (i == 4 ? 17 : s);
        uint64_t v = 0;
        for (uint32_t j = 0; j < len[i]; ++j) {
            x ^= x << 13; x ^= x >> 7; x ^= x << 17;
            v += 1 + (x >> 9) % (0xFFFFFFFFFFFFFFFFull / (s + 1));
            rows[(size_t)i * stride + j] = i % 5 == 1 ? rows[(size_t)(i - 1) * stride + j] : v; // every fifth list repeats its neighbour
        }
        if (i % 5 == 1) len[i] = len[i - 1];
    }
    const uint64_t pairs = (uint64_t)n * (n - 1) / 2;
    std::vector<uint32_t> ref_c(pairs), ref_d(pairs), c(pairs), d(pairs);
    int bad = 0;
    const uint32_t forms[] = {16, 64, 512, 1024, 2048};
    for (size_t f = 0; f < sizeof forms / sizeof forms[0]; ++f) {
        uint32_t stats[6];
        const int rc = emul_triangle(rows.data(), len.data(), n, stride, s, forms[f], f == 1 ? 7u : 0u, f ? c.data() : ref_c.data(), f ? d.data() : ref_d.data(), stats);
        if (rc != 0) { printf("R = %u: rc %d\n", forms[f], rc); bad = 1; }
        if (f && (c != ref_c || d != ref_d)) { printf("R = %u differs from R = %u\n", forms[f], forms[0]); bad = 1; }
    }
    printf(bad ? "FAILED\n" : "ok\n");
    return bad;
}
#endif
