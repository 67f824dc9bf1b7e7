// tests/emul/merge_emul.cpp -- CPU emulator of the sharded path's merge (mhx_merge.hip, test tool).  Runs the host+device
// functions of auriclass_amd/csrc/mhx_merge.h themselves over a whole call: the scatter, bin and compact phases in turn, the
// workgroups of a phase and the virtual threads between two barriers in an order a seeded shuffle chooses (the atomics'
// order shows in the scatter positions and must not show in the result); and the table path's insert over a small table.
// Checked explicitly (-2): the bin index of every entry taken against nbins, the scatter arrays' and the result block's
// bounds in the compaction, and -- by canaries behind a region-sized buffer -- that the rank write stays inside the bin's
// region.  The LDS images are allocated with the byte counts launch_merge_bins requests (merge_*_lds_bytes) and laid out
// as the kernels lay them out; an access beyond them shows under the host sanitizers alone (the stand-alone main).
// Not part of the product; built by tests/test_merge_emulation.py with g++.
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <numeric>
#include <vector>
#include "../../auriclass_amd/csrc/mhx_merge.h"

using namespace mhx;

namespace {

struct Shuffler {
    uint64_t x;
    explicit Shuffler(uint64_t seed) : x(seed * 0x9E3779B97F4A7C15ull + 88172645463325252ull) {}
    uint64_t draw(uint64_t bound) { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return (x >> 11) % bound; }
    std::vector<uint32_t> order(uint32_t n)
    {
        std::vector<uint32_t> o(n);
        std::iota(o.begin(), o.end(), 0u);
        for (uint32_t i = n; i > 1; --i) std::swap(o[i - 1], o[draw(i)]);
        return o;
    }
};

constexpr uint32_t kScatterThreads = 1024, kScatterBatch = 4, kBinThreads = 256, kCompactThreads = 1024, kChunk = 8192;

} // namespace

extern "C" void emul_merge_consts(uint32_t *out4)
{
    out4[0] = kMaxMergeRanks; out4[1] = kMergeMaxBins; out4[2] = kMergeMaxSlots; out4[3] = kMergeMaxQual;
}

// out7: nbins, shift, region, table_slots, bins_used, dynamic LDS bytes of the scatter pass, of the bin pass; returns 1 for the binned path
extern "C" int emul_merge_geometry(uint64_t total, uint64_t t_min, uint32_t n_ranks, uint64_t *out7)
{
    MergeGeometry g;
    const bool ok = merge_geometry(total, t_min, n_ranks, g);
    out7[0] = g.nbins; out7[1] = g.shift; out7[2] = g.region; out7[3] = g.table_slots; out7[4] = g.bins_used;
    out7[5] = ok ? merge_scatter_lds_bytes(g.nbins) : 0;
    out7[6] = ok ? merge_bin_lds_bytes(g.table_slots) : 0;
    return ok ? 1 : 0;
}

// One call of launch_merge_bins on the gathered buffer `slabs` (nranks slabs of slab_words words: [hdr_words | hashes[cap] |
// counts u32[cap]], n[r] valid entries each).  out: the result block [n, T, flags, 0 | hashes[out_cap] | counts[out_cap]];
// fills[nbins]: entries the scatter pass counted into each bin (beyond `region`: not stored), quals[nbins]: entries of each
// bin that qualify (beyond kMergeMaxQual: not ranked).  Returns the flags word; -1: not the binned path; -2: a bin index,
// a rank write or a compaction access out of range; -3: cursor or flags not zero again at the end.
extern "C" int64_t emul_merge_binned(const uint64_t *slabs, uint64_t slab_words, uint64_t cap, uint32_t hdr_words, const uint64_t *n, uint32_t nranks,
                                     uint32_t min_mult, uint64_t t_min, uint64_t seed, uint32_t out_cap, uint64_t *out, uint32_t *fills, uint32_t *quals)
{
    uint64_t total = 0, max_n = 0;
    for (uint32_t r = 0; r < nranks; ++r) { total += n[r]; max_n = std::max(max_n, n[r]); }
    MergeGeometry g;
    if (!merge_geometry(total, t_min, nranks, g)) return -1;
    const uint32_t nbins = g.nbins, region = g.region, slots = g.table_slots;
    Shuffler sh(seed);
    std::vector<uint32_t> cursor(nbins, 0), qn(nbins, 0);
    uint32_t flags = 0;
    std::vector<uint64_t> sc_keys((size_t)nbins * region, 0xDDDDDDDDDDDDDDDDull);
    std::vector<uint32_t> sc_cnts((size_t)nbins * region, 0xDDDDDDDDu);
    bool bad = false;

    // ---- merge_scatter_kernel: grid (chunks, nranks)
    const uint32_t chunks = (uint32_t)((max_n + kChunk - 1) / kChunk);
    const size_t scatter_words = merge_scatter_lds_bytes(nbins) / sizeof(uint32_t);
    for (uint32_t wg : sh.order(chunks * nranks)) {
        const uint32_t bx = wg % chunks, r = wg / chunks;
        std::vector<uint32_t> smem(scatter_words, 0xCCCCCCCCu);
        uint32_t *cnt = smem.data(), *base = smem.data() + nbins;
        const uint64_t i0 = (uint64_t)bx * kChunk;
        if (i0 >= n[r]) continue;
        const uint64_t i1 = std::min(i0 + kChunk, n[r]);
        const uint64_t *hashes = slabs + (uint64_t)r * slab_words + hdr_words;
        const uint32_t *counts = reinterpret_cast<const uint32_t *>(hashes + cap);
        for (uint32_t b = 0; b < nbins; ++b) cnt[b] = 0;
        constexpr uint64_t kStep = (uint64_t)kScatterThreads * kScatterBatch;
        for (uint32_t tid : sh.order(kScatterThreads))
            for (uint64_t j = i0 + tid; j < i1; j += kStep)
                for (uint32_t u = 0; u < kScatterBatch; ++u) {
                    const uint64_t i = j + (uint64_t)u * kScatterThreads;
                    const uint64_t h = i < i1 ? hashes[i] : kEmptyKey;
                    if (!merge_takes(h, t_min)) continue;
                    const uint32_t b = merge_bin(h, g.shift);
                    if (b >= nbins) { bad = true; continue; }
                    merge_atomic_add(&cnt[b], 1u);
                }
        for (uint32_t tid : sh.order(kScatterThreads))
            for (uint32_t b = tid; b < nbins; b += kScatterThreads) {
                const uint32_t c = cnt[b];
                base[b] = c ? merge_atomic_add(&cursor[b], c) : 0u;
                cnt[b] = 0;
            }
        bool over = false;
        for (uint32_t tid : sh.order(kScatterThreads))
            for (uint64_t j = i0 + tid; j < i1; j += kStep)
                for (uint32_t u = 0; u < kScatterBatch; ++u) {
                    const uint64_t i = j + (uint64_t)u * kScatterThreads;
                    const uint64_t h = i < i1 ? hashes[i] : kEmptyKey;
                    const uint32_t c = i < i1 ? counts[i] : 0u;
                    if (!merge_takes(h, t_min)) continue;
                    const uint32_t b = merge_bin(h, g.shift);
                    if (b >= nbins) { bad = true; continue; }
                    const uint32_t pos = base[b] + merge_atomic_add(&cnt[b], 1u);
                    if (pos < region) {
                        sc_keys[(uint64_t)b * region + pos] = h;
                        sc_cnts[(uint64_t)b * region + pos] = c;
                    } else {
                        over = true;
                    }
                }
        if (over) flags |= kMergeFlagRegion;
    }

    // ---- merge_bin_kernel: one workgroup per bin
    const size_t bin_bytes = merge_bin_lds_bytes(slots);
    for (uint32_t b : sh.order(nbins)) {
        std::vector<unsigned long long> lds((bin_bytes + 7) / 8, 0xCCCCCCCCCCCCCCCCull);
        unsigned long long *keys = lds.data();
        uint32_t *cnts = reinterpret_cast<uint32_t *>(keys + slots);
        unsigned long long *qk = reinterpret_cast<unsigned long long *>(cnts + slots);
        uint32_t *qc = reinterpret_cast<uint32_t *>(qk + kMergeMaxQual);
        uint32_t nq = 0;
        const uint32_t mask = slots - 1;
        const uint32_t filled = cursor[b];
        const uint32_t nb = filled < region ? filled : region;
        fills[b] = filled;
        quals[b] = 0;
        for (uint32_t i = 0; i < slots; ++i) { keys[i] = kEmptyKey; cnts[i] = 0; }
        if (merge_table_guard(nb, slots)) {
            flags |= kMergeFlagTable; qn[b] = 0; cursor[b] = 0;
            continue;
        }
        const uint64_t *rk = sc_keys.data() + (uint64_t)b * region;
        const uint32_t *rc = sc_cnts.data() + (uint64_t)b * region;
        bool wrapped = false;
        for (uint32_t tid : sh.order(kBinThreads))
            for (uint32_t i = tid; i < nb; i += kBinThreads) wrapped |= merge_lds_insert(keys, cnts, mask, rk[i], rc[i]);
        if (wrapped) flags |= kMergeFlagWrap;
        bool over = false;
        for (uint32_t tid : sh.order(kBinThreads))
            for (uint32_t i = tid; i < slots; i += kBinThreads)
                if (merge_qualifies(keys[i], cnts[i], min_mult)) {
                    const uint32_t p = merge_atomic_add(&nq, 1u);
                    if (p < kMergeMaxQual) { qk[p] = keys[i]; qc[p] = cnts[i]; }
                    else over = true;
                }
        if (over) flags |= kMergeFlagQual;
        quals[b] = nq;
        const uint32_t q = nq < kMergeMaxQual ? nq : kMergeMaxQual;
        uint64_t *ok = sc_keys.data() + (uint64_t)b * region;
        uint32_t *oc = sc_cnts.data() + (uint64_t)b * region;
        // into a region-sized buffer with canaries behind it (a rank is < q <= kMergeMaxQual), then to the region's head
        constexpr uint64_t kCanary = 0xABABABABABABABABull;
        std::vector<uint64_t> wk((size_t)region + kMergeMaxQual, kCanary);
        std::vector<uint32_t> wc((size_t)region + kMergeMaxQual, (uint32_t)kCanary);
        std::copy(ok, ok + region, wk.begin());
        std::copy(oc, oc + region, wc.begin());
        for (uint32_t tid : sh.order(kBinThreads))
            for (uint32_t t = tid; t < q; t += kBinThreads) merge_rank_write(qk, qc, q, t, region, wk.data(), wc.data());
        for (size_t i = region; i < wk.size(); ++i) if (wk[i] != kCanary || wc[i] != (uint32_t)kCanary) bad = true;
        std::copy(wk.begin(), wk.begin() + region, ok);
        std::copy(wc.begin(), wc.begin() + region, oc);
        qn[b] = q < region ? q : region;
        cursor[b] = 0;
    }

    // ---- merge_compact_kernel: one workgroup per 256 bins
    uint32_t *out_c = reinterpret_cast<uint32_t *>(out + 4 + out_cap);
    uint32_t flags_out = 0;
    for (uint32_t wg : sh.order(nbins / 256)) {
        const uint32_t first = wg * 256;
        uint32_t block_base = 0, grand_total = 0;
        for (uint32_t b = 0; b < nbins; ++b) { grand_total += qn[b]; if (b < first) block_base += qn[b]; }
        uint32_t s_off[257];
        uint32_t run = block_base;
        for (uint32_t i = 0; i < 256; ++i) { s_off[i] = run; run += first + i < nbins ? qn[first + i] : 0u; }
        s_off[256] = run;
        const uint32_t lo = s_off[0], hi = s_off[256] < out_cap ? s_off[256] : out_cap;
        for (uint32_t tid : sh.order(kCompactThreads))
            for (uint32_t e = lo + tid; e < hi; e += 2 * kCompactThreads) {
                const uint32_t e2 = e + kCompactThreads;
                const bool two = e2 < hi;
                const uint64_t s1 = merge_source(s_off, e, first, region), s2 = two ? merge_source(s_off, e2, first, region) : s1;
                if (s1 >= sc_keys.size() || s2 >= sc_keys.size() || e >= out_cap || (two && e2 >= out_cap)) { bad = true; continue; }
                out[4 + e] = sc_keys[s1];
                out_c[e] = sc_cnts[s1];
                if (two) { out[4 + e2] = sc_keys[s2]; out_c[e2] = sc_cnts[s2]; }
            }
        if (wg == 0) {
            out[0] = grand_total; out[1] = t_min; out[2] = flags; out[3] = 0;
            flags_out = flags;
            flags = 0;
        }
    }
    if (bad) return -2;
    if (flags != 0 || std::any_of(cursor.begin(), cursor.end(), [](uint32_t c) { return c != 0; })) return -3;
    return (int64_t)flags_out;
}

// The table path over a table of `nslots` slots (a power of two; keys at 2^64-1 and counts at 0 where vacant, this rank's
// own entries already in it): slab_insert_kernel's launches as merge_slabs_impl makes them, kMaxMergeRanks ranks each, the
// threads of a launch in shuffled order.  own_rank >= nranks: no slab is skipped.  Returns 1 when an entry found no slot.
extern "C" int emul_merge_table(const uint64_t *slabs, uint64_t slab_words, uint64_t cap, uint32_t hdr_words, const uint64_t *n, uint32_t nranks,
                                uint32_t own_rank, uint64_t t_min, uint64_t seed, uint64_t *keys, uint32_t *cnts, uint64_t nslots)
{
    Shuffler sh(seed);
    uint64_t max_n = 0;
    for (uint32_t r = 0; r < nranks; ++r) if (r != own_rank) max_n = std::max(max_n, n[r]);
    uint64_t blocks = (max_n + 255) / 256;
    blocks = std::min<uint64_t>(std::max<uint64_t>(blocks, 1), 4096);
    const uint64_t stride = blocks * 256;
    int full = 0;
    for (uint32_t r0 = 0; r0 < nranks; r0 += kMaxMergeRanks) {
        const uint32_t launch_ranks = merge_launch_ranks(nranks, r0);
        const uint32_t own = merge_launch_own(own_rank, r0, launch_ranks);
        for (uint32_t v : sh.order((uint32_t)(stride * launch_ranks))) {
            const uint32_t r = (uint32_t)(v / stride);
            if (r == own) continue;
            const uint64_t *hashes = slabs + (uint64_t)(r0 + r) * slab_words + hdr_words;
            const uint32_t *counts = reinterpret_cast<const uint32_t *>(hashes + cap);
            for (uint64_t i = v % stride; i < n[r0 + r]; i += stride) {
                const uint64_t h = hashes[i];
                if (!merge_takes(h, t_min)) continue;
                if (!merge_table_insert(reinterpret_cast<unsigned long long *>(keys), cnts, nslots - 1, h, counts[i])) full = 1;
            }
        }
    }
    return full;
}

#ifdef MERGE_EMUL_MAIN
// stand-alone run for a host sanitizer build: three ranks of random entries through the binned merge under several
// schedules and through the table path, against a sorted merge; and one call with every entry in one bin
#include <cstdio>
#include <map>
int main()
{
    const uint32_t nranks = 3, m = 2, out_cap = 2000;
    const uint64_t cap = 3000, t_min = (1ull << 50) + 17, words = cap + cap / 2;
    std::vector<uint64_t> slabs(nranks * words, 0x0123456789ABCDEFull), n = {2900, 3000, 0};
    Shuffler gen(5);
    std::map<uint64_t, uint64_t> want;
    for (uint32_t r = 0; r < nranks; ++r) {
        uint32_t *c = reinterpret_cast<uint32_t *>(slabs.data() + r * words + cap);
        for (uint64_t i = 0; i < n[r]; ++i) {
            const uint64_t h = gen.draw(4000) * 0x3FFFFFFFFFull + (gen.draw(50) == 0 ? t_min : 0); // (distinct within a slab or not: sums either way)
            slabs[r * words + i] = i == 7 ? ~0ull : h;
            c[i] = 1 + (uint32_t)gen.draw(3);
            if (i != 7 && h <= t_min) want[h] += c[i];
        }
    }
    std::vector<uint64_t> wh;
    std::vector<uint32_t> wc;
    for (auto &kv : want) if (kv.second >= m) { wh.push_back(kv.first); wc.push_back((uint32_t)kv.second); }
    int bad = 0;
    uint64_t geo[7];
    emul_merge_geometry(5900, t_min, nranks, geo);
    std::vector<uint32_t> fills(geo[0]), quals(geo[0]);
    for (uint64_t seed = 0; seed < 4; ++seed) {
        std::vector<uint64_t> out(4 + out_cap + out_cap / 2, 0);
        const int64_t rc = emul_merge_binned(slabs.data(), words, cap, 0, n.data(), nranks, m, t_min, seed, out_cap, out.data(), fills.data(), quals.data());
        const uint32_t *oc = reinterpret_cast<const uint32_t *>(out.data() + 4 + out_cap);
        const size_t k = std::min<size_t>(wh.size(), out_cap);
        if (rc != 0 || out[0] != wh.size() || memcmp(out.data() + 4, wh.data(), k * 8) || memcmp(oc, wc.data(), k * 4)) { printf("seed %llu differs (rc %lld)\n", (unsigned long long)seed, (long long)rc); bad = 1; }
    }
    const uint64_t nslots = 1 << 14;
    std::vector<uint64_t> keys(nslots, ~0ull);
    std::vector<uint32_t> cnts(nslots, 0);
    if (emul_merge_table(slabs.data(), words, cap, 0, n.data(), nranks, 2, t_min, 9, keys.data(), cnts.data(), nslots)) { printf("table full\n"); bad = 1; }
    std::map<uint64_t, uint64_t> got;
    for (uint64_t i = 0; i < nslots; ++i) if (keys[i] != ~0ull) got[keys[i]] = cnts[i];
    if (got != want) { printf("table path differs\n"); bad = 1; }
    // every entry in one bin: flag 1, and nothing written out of range
    for (uint32_t r = 0; r < 2; ++r) for (uint64_t i = 0; i < n[r]; ++i) slabs[r * words + i] = (5ull << 42) + r * 5000 + i;
    std::vector<uint64_t> out(4 + out_cap + out_cap / 2, 0);
    const int64_t rc = emul_merge_binned(slabs.data(), words, cap, 0, n.data(), nranks, 1, t_min, 3, out_cap, out.data(), fills.data(), quals.data());
    if (rc != (int64_t)kMergeFlagRegion) { printf("one bin: rc %lld\n", (long long)rc); bad = 1; }
    printf(bad ? "FAILED\n" : "ok (%zu entries)\n", wh.size());
    return bad;
}
#endif
