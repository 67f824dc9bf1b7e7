// tests/emul/dist_emul.cpp -- CPU emulator of the all-vs-refs distance path (mhx_dist.hip: dist_shift / split / range /
// window / finish kernels, test tool).  Runs the host+device functions of auriclass_amd/csrc/mhx_dist.h in the kernels'
// order, one work item after the other: the shift from the largest value, the split pass work item by work item (two
// elements each), the range pass range by range in the workgroups' order (table build, probe, byte counters), the window
// totals and the finish walk of every pair -- in the base form (1024 ranges) and in the windowed form (1024 x W).
// Not part of the product; built by tests/test_dist_emulation.py with g++.
#include <cstdint>
#include <cstring>
#include <vector>
#include "../../auriclass_amd/csrc/mhx_dist.h"

using namespace mhx;

extern "C" uint32_t emul_dist_windows(uint64_t longest) { return dist_windows(longest); }
extern "C" uint32_t emul_dist_wide_max_queries(uint32_t nr, uint32_t ranges) { return dist_wide_max_queries(nr, ranges); }
extern "C" uint32_t emul_dist_max_windows(void) { return kDistMaxWindows; }

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

// One (query batch, reference slice) block: nr <= 32 references, rows `stride` apart.  windows: W of the geometry (a power
// of two), 0 = by the rule from the longest list.  Returns 0 and fills common / denom [nq][nr]; 1 when the overflow flag
// went up (a range with too many distinct keys or a slice too long for byte counters: the generic kernel's case);
// -1 when the lists have no geometry.  stats (may be null): [0] ranges, [1] longest slice of any list, [2] most distinct
// keys in one range, [3] shift.
extern "C" int emul_dist(const uint64_t *q, const uint32_t *q_len, uint32_t nq, const uint64_t *r, const uint32_t *r_len, uint32_t nr,
                         uint32_t stride, uint32_t s, uint32_t windows, uint32_t *common, uint32_t *denom, uint32_t *stats)
{
    if (nr == 0 || nr > 32 || nq == 0) return -2;
    if (windows == 0) {
        uint32_t longest = 0;
        for (uint32_t i = 0; i < nq; ++i) longest = q_len[i] > longest ? q_len[i] : longest;
        for (uint32_t i = 0; i < nr; ++i) longest = r_len[i] > longest ? r_len[i] : longest;
        windows = dist_windows(longest);
        if (windows == 0) return -1;
    }
    const uint32_t R = (uint32_t)kDistRanges * windows, per = R + 1;
    const bool wide = windows > 1;
    // dist_shift_kernel
    uint64_t gmax = 0;
    for (uint32_t i = 0; i < nq; ++i) if (q_len[i]) { const uint64_t v = q[(uint64_t)i * stride + q_len[i] - 1]; gmax = v > gmax ? v : gmax; }
    for (uint32_t i = 0; i < nr; ++i) if (r_len[i]) { const uint64_t v = r[(uint64_t)i * stride + r_len[i] - 1]; gmax = v > gmax ? v : gmax; }
    const uint32_t shift = dist_shift_for(gmax, R);
    // dist_split_kernel
    std::vector<uint32_t> offs_q((size_t)nq * per, 0xDEADBEEFu), offs_r((size_t)nr * per, 0xDEADBEEFu);
    for (uint32_t i = 0; i < nq; ++i) split_list(q + (uint64_t)i * stride, q_len[i], shift, per, &offs_q[(size_t)i * per]);
    for (uint32_t i = 0; i < nr; ++i) split_list(r + (uint64_t)i * stride, r_len[i], shift, per, &offs_r[(size_t)i * per]);
    // dist_range_kernel / dist_range_lane_kernel: one workgroup per range, in the grid's order
    const uint32_t nwords = (nr + 3) / 4, cstride = 4 * nwords;
    std::vector<uint32_t> cpart((size_t)nq * R * nwords, 0xA5A5A5A5u);
    std::vector<unsigned long long> keys(kDistTableSlots);
    std::vector<uint32_t> masks(kDistMaskWords);
    uint32_t flag = 0, longest_slice = 0, most_keys = 0;
    std::vector<uint8_t> seen(R, 0);
    for (uint32_t block = 0; block < R; ++block) {
        const uint32_t p = dist_range_of_block(block, R);
        if (p >= R || seen[p]) return -3; // the order must be a permutation of the ranges
        seen[p] = 1;
        dist_table_clear(keys.data(), masks.data(), 0, 1);
        uint32_t ndistinct = 0;
        for (uint32_t ri = 0; ri < nr; ++ri) {
            const uint32_t b = offs_r[(size_t)ri * per + p], e = offs_r[(size_t)ri * per + p + 1];
            longest_slice = e - b > longest_slice ? e - b : longest_slice;
            if (wide && e - b > kDistSliceLimit) { ndistinct += (uint32_t)kDistTableSlots; continue; } // not inserted: counts as a table overflow
            for (uint32_t i = b; i < e; ++i) ndistinct += dist_table_insert_plain(keys.data(), masks.data(), r[(uint64_t)ri * stride + i], ri);
        }
        most_keys = ndistinct > most_keys ? ndistinct : most_keys;
        if (ndistinct > kDistTableLimit) { flag |= 1u; continue; }
        for (uint32_t qi = 0; qi < nq; ++qi) {
            const uint32_t b = offs_q[(size_t)qi * per + p], e = offs_q[(size_t)qi * per + p + 1];
            longest_slice = e - b > longest_slice ? e - b : longest_slice;
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
    if (stats) { stats[0] = R; stats[1] = longest_slice; stats[2] = most_keys; stats[3] = shift; }
    if (flag) return 1;
    const uint8_t *cbytes = reinterpret_cast<const uint8_t *>(cpart.data());
    // dist_window_kernel (windowed form)
    const uint32_t nwin = R / kDistWindowRanges;
    std::vector<uint32_t> wtot;
    if (wide) {
        wtot.assign((size_t)nq * nwin * cstride, 0);
        for (uint32_t qw = 0; qw < nq * nwin; ++qw)
            for (uint32_t j = 0; j < nwords; ++j)
                dist_window_sum(cpart.data() + (size_t)qw * kDistWindowRanges * nwords + j, nwords, kDistWindowRanges, &wtot[((size_t)qw * nwords + j) * 4]);
    }
    // dist_finish_kernel / dist_finish_wide_kernel
    for (uint32_t qi = 0; qi < nq; ++qi)
        for (uint32_t ri = 0; ri < nr; ++ri) {
            const DistPair x{cbytes + (size_t)qi * R * cstride + ri, cstride, &offs_q[(size_t)qi * per], &offs_r[(size_t)ri * per],
                             r + (uint64_t)ri * stride, q + (uint64_t)qi * stride, s};
            uint32_t uni = 0, com = 0, den;
            if (!wide) {
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
            } else {
                constexpr uint32_t kGroupWindows = kDistRanges / kDistWindowRanges;
                const uint32_t ngroups = windows;
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
            common[(size_t)qi * nr + ri] = com;
            denom[(size_t)qi * nr + ri] = den;
        }
    return 0;
}
