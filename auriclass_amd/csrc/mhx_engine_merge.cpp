// mhx_engine_merge.cpp -- the multi-GPU path of the sketcher: a shard's partial result exported as a slab, and the gathered
// slabs of all shards merged into the sketch of the union (binned on the device, in this rank's candidate table, or on the
// host).  The sketcher itself is in mhx_engine.cpp.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "mhx_device.h"
#include "mhx_engine_internal.h"
#include "mhx_internal.h"
#include "mhx_sketcher.h"

using namespace mhx;

// Multi-GPU fast path: the shard's partial result as ONE device-resident slab of int64 words
//   [0] n entries (may exceed cap: then only cap are present)   [1] admission threshold T
//   [2] device flags   [3 .. 3+cap) hashes   [3+cap ..) counts, two u32 per word
// holding every (hash, count) with hash <= T (T read on the device), unsorted.  Everything is enqueued on the engine stream
// and the stream is synchronised once, so the slab can go straight into an all-gather; nothing
// crosses PCIe here.
extern "C" int mhx_sketcher_export_slab(mhx_sketcher *sk, void *d_slab, uint32_t cap)
{
    return entry("mhx_sketcher_export_slab", [&]() -> int {
        if (!sk || !d_slab || cap == 0 || (cap & 1)) return fail(MHX_E_ARG, "export_slab: null argument or odd capacity");
        const int rc = settle(sk);
        if (rc) return rc;
        uint64_t *w = (uint64_t *)d_slab;
        HIPCHK(hipMemsetAsync(w, 0, 3 * sizeof(uint64_t), g.stream));
        // (the extract kernel ORs the device flags and the state bits of the m > 1 phase, MHX_SLAB_*, into word [2])
        HIPCHK(launch_extract(table_args(sk), 0, 1, w + 3, (uint32_t *)(w + 3 + cap), cap, (uint32_t *)w, w + 2, sk->d_thresh, w + 1, nullptr, g.stream));
        HIPCHK(hipStreamSynchronize(g.stream));
        return MHX_OK;
    });
}

// ---- sharded path: sizes first, slabs sized from the data, merge on the device ------------------
// 1. mhx_sketcher_export_begin : every (hash, count) <= T_r of this shard -> the sketcher's own device buffer; the
//                                 header [n_r, T_r, flags, #(2^64-1), occupied slots] comes back (ranks all-gather it)
// 2. mhx_sketcher_export_pack  : the entries as ONE slab [hashes[cap] | counts u32[cap]], cap = max_r n_r, into the
//                                 caller's send buffer (device memory for RCCL, host memory for gloo)
// 3. mhx_sketcher_merge_slabs  : the other ranks' gathered slabs are added to this rank's candidate table
//                                 (slab_insert_kernel), the ordinary extraction with limit T_min = min_r T_r yields the
//                                 union's sketch; same exactness rule as finish() -> MHX_E_CAPACITY, never a short sketch
extern "C" int mhx_sketcher_export_begin(mhx_sketcher *sk, uint64_t *header8)
{
    return entry("mhx_sketcher_export_begin", [&]() -> int {
        if (!sk || !header8) return fail(MHX_E_ARG, "null argument");
        if (sk->merged) return fail(MHX_E_ARG, "this sketcher holds a merged table: mhx_sketcher_reset() first");
        const int rc = settle(sk);
        if (rc) return rc;
        uint64_t *d = sk->d_exp_hdr;
        for (int attempt = 0; attempt < 2; ++attempt) {
            // one kernel: entries to d_out_keys / d_out_cnts, the five header words accumulated on the device and stored
            // into the pinned mirror (and cleared for the next call) by the workgroup that finishes last
            HIPCHK(launch_extract(table_args(sk), 0, 1, sk->d_out_keys, sk->d_out_cnts, sk->out_cap(), (uint32_t *)d, d + 2, sk->d_thresh, d + 1, d + 3,
                                  g.stream, nullptr, 0, d, sk->h_exp_hdr, sk->d_done, d + 4, 5));
            HIPCHK(hipStreamSynchronize(g.stream));
            const uint64_t n = sk->h_exp_hdr[0];
            if (n > sk->out_cap()) { // grow (with room for the next, similar shard) and repeat once
                if (n + n / 4 + 1024 > 0xFFFFFFF0ull) return fail(MHX_E_CAPACITY, "export: %llu entries", (unsigned long long)n);
                HIPCHK(sk->d_out_keys.grow(n + n / 4 + 1024));
                HIPCHK(sk->d_out_cnts.grow(n + n / 4 + 1024));
                continue;
            }
            for (int i = 0; i < 5; ++i) header8[i] = sk->h_exp_hdr[i];
            header8[5] = header8[6] = header8[7] = 0;
            sk->exported = n;
            sk->export_valid = true;
            sk->last_T = header8[1];
            return MHX_OK;
        }
        return fail(MHX_E_INTERNAL, "export: output kept growing");
    });
}

extern "C" int mhx_sketcher_export_pack(mhx_sketcher *sk, void *dst, uint64_t cap_entries)
{
    return entry("mhx_sketcher_export_pack", [&]() -> int {
        if (!sk || !dst) return fail(MHX_E_ARG, "null argument");
        if (!sk->export_valid) return fail(MHX_E_ARG, "export_pack without a preceding mhx_sketcher_export_begin");
        if ((cap_entries & 1) || cap_entries < sk->exported) return fail(MHX_E_ARG, "export_pack: capacity %llu is odd or below this shard's %llu entries",
                                                                         (unsigned long long)cap_entries, (unsigned long long)sk->exported);
        uint8_t *p = (uint8_t *)dst;
        if (sk->exported) { // device-to-device for RCCL send buffers, device-to-host for gloo's
            HIPCHK(hipMemcpyAsync(p, sk->d_out_keys, sk->exported * sizeof(uint64_t), hipMemcpyDefault, g.stream));
            HIPCHK(hipMemcpyAsync(p + cap_entries * sizeof(uint64_t), sk->d_out_cnts, sk->exported * sizeof(uint32_t), hipMemcpyDefault, g.stream));
        }
        HIPCHK(hipStreamSynchronize(g.stream));
        return MHX_OK;
    });
}

// ---- the merge of gathered slabs, in four parts -------------------------------------------------------------------------
namespace {

struct Gathered { // the slabs of all ranks as one merge call got them, and what their headers add up to
    const void *slabs;          // where the caller has them (device or host memory)
    const uint64_t *d_slabs;    // on the device: the caller's, or this sketcher's staging copy
    int slabs_on_device;
    uint32_t n_ranks, own_rank, hdr_words;
    uint64_t cap_entries, slab_words;
    const uint64_t *headers;    // [n_ranks][8]: n, T, flags, #(2^64-1), occupied slots
    uint64_t t_min = ~0ull, others = 0, maxkey_others = 0, flags = 0, max_n = 0;
    uint64_t header(uint32_t r, int word) const { return headers[8 * (size_t)r + word]; }
    uint64_t own(int word) const { return header(own_rank, word); }
};

// 1. the argument checks and the summary of the gathered headers: the smallest threshold, the other ranks' entries, their
//    occurrences of 2^64-1 and their longest slab, every rank's error flags; the own header must be this sketcher's export
int summarize_headers(mhx_sketcher *sk, Gathered &G, const uint64_t *hashes, const uint32_t *n_out)
{
    if (sk) sk->mg_info = {}; // (a call that ends in an argument error leaves "no path", not the previous merge's)
    if (!sk || !G.headers || !hashes || !n_out || G.n_ranks == 0) return fail(MHX_E_ARG, "null argument");
    if (G.own_rank >= G.n_ranks) return fail(MHX_E_ARG, "own_rank %u out of range (%u ranks)", G.own_rank, G.n_ranks);
    if (G.cap_entries & 1) return fail(MHX_E_ARG, "merge_slabs: odd slab capacity");
    if (sk->merged) return fail(MHX_E_ARG, "this sketcher holds a merged table already: mhx_sketcher_reset() first");
    if (!sk->export_valid) return fail(MHX_E_ARG, "merge_slabs without a preceding mhx_sketcher_export_begin on this sketcher");
    for (uint32_t r = 0; r < G.n_ranks; ++r) {
        const uint64_t *h = G.headers + 8 * (size_t)r;
        if (h[0] > G.cap_entries) return fail(MHX_E_ARG, "merge_slabs: rank %u announces %llu entries, slabs hold %llu", r, (unsigned long long)h[0], (unsigned long long)G.cap_entries);
        G.t_min = h[1] < G.t_min ? h[1] : G.t_min;
        G.flags |= h[2] & kFlagErrorMask & ~kFlagNeedLookback;
        if (r != G.own_rank) { G.others += h[0]; G.maxkey_others += h[3]; G.max_n = h[0] > G.max_n ? h[0] : G.max_n; }
    }
    if (G.own(0) != sk->exported || G.own(1) != sk->last_T)
        return fail(MHX_E_ARG, "merge_slabs: header of rank %u is not this sketcher's export", G.own_rank);
    const int rc = check_flags(G.flags); // a full table or a malformed FASTQ on ANY rank
    if (rc) return rc;
    if ((G.others || G.n_ranks > 1) && !G.slabs) return fail(MHX_E_ARG, "null slabs");
    return MHX_OK;
}

// 2. The usual case: all slabs (this rank's own among them) are binned by value and merged bin by bin in LDS; the result
//    lands in the pinned block in hash order.  Non-uniform data (a bin overflows), more than 64 ranks or more than ~16 M
//    entries are left to the table path: kUndecided, which is no error code.
constexpr int kUndecided = 1;
int merge_binned(mhx_sketcher *sk, const Gathered &G, uint64_t *hashes, uint32_t *counts, uint32_t *n_out)
{
    static const bool force_table = getenv("MHX_MERGE_TABLE") != nullptr;
    const uint64_t total = G.others + G.own(0);
    MergeGeometry geo;
    if (force_table || !merge_geometry(total, G.t_min, G.n_ranks, geo)) return kUndecided;
    const uint32_t nbins = geo.nbins;
    MergeArgs a;
    a.shift = geo.shift; a.region = geo.region; a.table_slots = geo.table_slots;
    if (!sk->d_mg_small) {
        HIPCHK(sk->d_mg_small.grow(2 * (size_t)kMergeMaxBins + 16));
        HIPCHK(hipMemsetAsync(sk->d_mg_small, 0, (2 * (size_t)kMergeMaxBins + 16) * sizeof(uint32_t), g.stream));
    }
    const size_t need = (size_t)nbins * a.region;
    if (std::min(sk->d_mg_keys.cap(), sk->d_mg_cnts.cap()) < need) {
        HIPCHK(sk->d_mg_keys.grow(need + need / 4, g.stream));
        HIPCHK(sk->d_mg_cnts.grow(need + need / 4));
    }
    a.slabs = G.d_slabs; a.slab_words = G.slab_words; a.cap = G.cap_entries; a.hdr_words = G.hdr_words; a.nranks = G.n_ranks; a.min_mult = sk->m; a.t_min = G.t_min; a.nbins = nbins;
    uint64_t max_all = 0;
    for (uint32_t r = 0; r < kMaxMergeRanks; ++r) { a.n[r] = r < G.n_ranks ? G.header(r, 0) : 0; max_all = a.n[r] > max_all ? a.n[r] : max_all; }
    a.cursor = sk->d_mg_small; a.qn = sk->d_mg_small + kMergeMaxBins; a.flags = sk->d_mg_small + 2 * kMergeMaxBins;
    a.sc_keys = sk->d_mg_keys; a.sc_cnts = sk->d_mg_cnts;
    HIPCHK(launch_merge_bins(a, max_all, sk->h_fin, sk->fin_cap, g.stream));
    HIPCHK(hipStreamSynchronize(g.stream));
    const uint64_t *h = sk->h_fin;
    const uint64_t n_q = h[0];
    sk->mg_info.attempted = 1; sk->mg_info.flags = (uint32_t)h[2];
    sk->mg_info.nbins = nbins; sk->mg_info.region = a.region; sk->mg_info.table_slots = a.table_slots;
    static const bool dbg = getenv("MHX_MERGE_DEBUG") != nullptr;
    if (dbg) fprintf(stderr, "[mhx merge] %u ranks, %llu entries, %u bins (%llu used) of %u entries, table %u: %llu qualify, flags %llu\n", G.n_ranks,
                     (unsigned long long)total, nbins, (unsigned long long)geo.bins_used, a.region, a.table_slots, (unsigned long long)n_q, (unsigned long long)h[2]);
    // (flags raised -- a bin's region or table overflowed on non-uniform data, or a count sum passed 2^32-1: the
    // table path decides)
    if (h[2] != 0) return kUndecided;
    sk->mg_info.path = kMergePathBinned;
    // (more qualify than the block holds? the bins are in value order: its first s entries are the sketch)
    const uint64_t maxkey_all = G.maxkey_others + G.own(3);
    const uint64_t n_src = n_q + (has_max_key_entry(G.t_min, maxkey_all, sk->m) ? 1 : 0);
    if (!sketch_exact(n_src, sk->s, G.t_min, sk->hash_max))
        return fail(MHX_E_CAPACITY, "sharded sketch not exact: %llu of %u entries with multiplicity >= %u below the smallest shard threshold; "
                    "every rank must sketch its shard again with a larger budget_scale", (unsigned long long)n_src, sk->s, sk->m);
    const uint32_t nn = n_src < sk->s ? (uint32_t)n_src : sk->s;
    const uint32_t from_block = nn < n_q ? nn : (uint32_t)n_q; // <= s <= fin_cap: all of them are in the block
    memcpy(hashes, h + 4, (size_t)from_block * sizeof(uint64_t));
    if (counts) memcpy(counts, reinterpret_cast<const uint32_t *>(h + 4 + sk->fin_cap), (size_t)from_block * sizeof(uint32_t));
    if (nn > from_block) { hashes[from_block] = ~0ull; if (counts) counts[from_block] = saturated_count(maxkey_all); }
    *n_out = nn;
    return MHX_OK;
}

// 3. The other shards' entries would crowd this table (tiny tables of tiny inputs, or shards that never tightened
//    their thresholds): the host merge decides instead, by the same rule on the same gathered data.
int merge_on_host(mhx_sketcher *sk, const Gathered &G, uint64_t *hashes, uint32_t *counts, uint32_t *n_out)
{
    std::vector<uint64_t> hbuf((size_t)G.n_ranks * G.slab_words);
    if (G.slabs_on_device) {
        HIPCHK(hipMemcpyAsync(hbuf.data(), G.slabs, hbuf.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, g.stream));
        HIPCHK(hipStreamSynchronize(g.stream));
    } else {
        memcpy(hbuf.data(), G.slabs, hbuf.size() * sizeof(uint64_t));
    }
    std::vector<uint64_t> ah, an(G.n_ranks), at(G.n_ranks);
    std::vector<uint32_t> ac;
    for (uint32_t r = 0; r < G.n_ranks; ++r) {
        const uint64_t n = G.header(r, 0), mk = G.header(r, 3);
        const uint64_t *hp = hbuf.data() + (size_t)r * G.slab_words + G.hdr_words;
        const uint32_t *cp = reinterpret_cast<const uint32_t *>(hp + G.cap_entries);
        an[r] = 0;
        for (uint64_t i = 0; i < n; ++i) // (2^64-1 inside a slab is a vacant slot to the kernels: it travels in header word 3 alone)
            if (hp[i] != kEmptyKey) { ah.push_back(hp[i]); ac.push_back(cp[i]); ++an[r]; }
        at[r] = G.header(r, 1);
        // the one value the table cannot hold: a shard that rejected nothing hands its occurrences on as an entry (whether
        // the sum over the shards qualifies is the merge's to say)
        if (mk && at[r] == ~0ull) { ah.push_back(~0ull); ac.push_back(saturated_count(mk)); ++an[r]; }
    }
    sk->mg_info.path = kMergePathHost;
    return mhx_merge_shard_partials(ah.data(), ac.data(), an.data(), at.data(), G.n_ranks, sk->k, sk->s, sk->m, hashes, counts, n_out);
}

// 4. the other ranks' slabs into this rank's candidate table, then the ordinary extraction
int merge_in_table(mhx_sketcher *sk, const Gathered &G, uint64_t *hashes, uint32_t *counts, uint32_t *n_out)
{
    for (uint32_t r0 = 0; r0 < G.n_ranks; r0 += kMaxMergeRanks) { // (one launch for up to 64 ranks)
        SlabMergeArgs a;
        a.slabs = G.d_slabs + (size_t)r0 * G.slab_words;
        a.slab_words = G.slab_words;
        a.cap = G.cap_entries;
        a.hdr_words = G.hdr_words;
        a.nranks = merge_launch_ranks(G.n_ranks, r0);
        for (uint32_t r = 0; r < kMaxMergeRanks; ++r) a.n[r] = r < a.nranks ? G.header(r0 + r, 0) : 0;
        a.own_rank = merge_launch_own(G.own_rank, r0, a.nranks);
        a.t_min = G.t_min;
        a.maxkey_others = r0 == 0 ? G.maxkey_others : 0;
        a.keys = sk->d_keys; a.cnts = sk->d_cnts; a.slot_mask = sk->nslots - 1; a.thresh = sk->d_thresh; a.stats = sk->d_stats;
        HIPCHK(launch_slab_insert(a, G.max_n, g.stream));
    }
    // the table now holds the union below T_min with summed counts, and T = T_min on the device: the ordinary extraction
    // (count >= m, hash <= T, ordering kernels for large sketches) and finish()'s exactness rule do the rest
    sk->table_dirty = false;
    sk->table_sampled = false;
    sk->unsettled.clear();
    sk->mg_info.path = kMergePathTable;
    return mhx_sketcher_finish(sk, hashes, counts, n_out);
}

// what mhx_sketcher_merge_slabs and mhx_sketcher_merge_gathered (hdr_words = 8: the headers ride in front of the slabs) share
int merge_slabs(mhx_sketcher *sk, const void *slabs, int slabs_on_device, uint32_t n_ranks, uint64_t cap_entries, const uint64_t *headers,
                uint32_t own_rank, uint64_t *hashes, uint32_t *counts, uint32_t *n_out, uint32_t hdr_words)
{
    Gathered G;
    G.slabs = slabs; G.d_slabs = (const uint64_t *)slabs; G.slabs_on_device = slabs_on_device;
    G.n_ranks = n_ranks; G.own_rank = own_rank; G.hdr_words = hdr_words;
    G.cap_entries = cap_entries; G.slab_words = hdr_words + cap_entries + cap_entries / 2;
    G.headers = headers;
    int rc = summarize_headers(sk, G, hashes, n_out);
    if (rc) return rc;
    if (!slabs_on_device && (G.others || G.own(0))) { // slabs gathered in host memory (gloo) go through the staging buffer
        const size_t bytes = (size_t)n_ranks * G.slab_words * sizeof(uint64_t);
        if (sk->d_merge_in.cap() * sizeof(uint64_t) < bytes)
            HIPCHK(sk->d_merge_in.grow(((bytes + bytes / 4 + (1u << 20)) & ~(size_t)((1u << 20) - 1)) / sizeof(uint64_t), g.stream));
        HIPCHK(hipMemcpyAsync(sk->d_merge_in, slabs, bytes, hipMemcpyHostToDevice, g.stream));
        G.d_slabs = sk->d_merge_in;
    }
    sk->merged = true;
    rc = merge_binned(sk, G, hashes, counts, n_out);
    if (rc != kUndecided) return rc;
    if (G.own(4) + G.others > sk->nslots / 2) return merge_on_host(sk, G, hashes, counts, n_out);
    return merge_in_table(sk, G, hashes, counts, n_out);
}

} // namespace

extern "C" int mhx_sketcher_merge_info(mhx_sketcher *sk, uint64_t *info8)
{
    return guarded("mhx_sketcher_merge_info", [&]() -> int {
        clear_error();
        if (!sk || !info8) return fail(MHX_E_ARG, "null argument");
        const MergeInfo &i = sk->mg_info;
        info8[0] = i.path; info8[1] = i.attempted; info8[2] = i.flags; info8[3] = i.nbins; info8[4] = i.region; info8[5] = i.table_slots;
        info8[6] = info8[7] = 0;
        return MHX_OK;
    });
}

extern "C" int mhx_sketcher_merge_slabs(mhx_sketcher *sk, const void *slabs, int slabs_on_device, uint32_t n_ranks, uint64_t cap_entries,
                                        const uint64_t *headers, uint32_t own_rank, uint64_t *hashes, uint32_t *counts, uint32_t *n_out)
{
    return entry("mhx_sketcher_merge_slabs", [&] { return merge_slabs(sk, slabs, slabs_on_device, n_ranks, cap_entries, headers, own_rank, hashes, counts, n_out, 0); });
}

// ---- the same exchange in ONE collective when the slabs live on the device (RCCL) -----------------------------------
// The 64-byte header rides in front of the slab: [header8 | hashes[cap] | counts u32[cap]], cap = the caller's guess (the
// last exchange's sizes, or 4 s + 4096 the first time).  mhx_sketcher_export_into writes the shard's partial result
// straight into the caller's send buffer -- no separate compaction buffer, no pack step --, the ranks all-gather the
// slabs, and mhx_sketcher_merge_gathered reads the gathered headers back itself: sizes first is then "sizes with", and
// only when some rank holds more entries than the guess does the caller repeat with the capacity that call reports
// (*need_cap; every rank sees the same headers and takes the same turn).
extern "C" int mhx_sketcher_export_into(mhx_sketcher *sk, void *d_slab, uint64_t cap_entries, uint64_t *header8)
{
    return entry("mhx_sketcher_export_into", [&]() -> int {
        if (!sk || !d_slab || !header8 || cap_entries == 0 || (cap_entries & 1) || cap_entries > 0xFFFFFFF0ull) return fail(MHX_E_ARG, "export_into: null argument or bad capacity");
        if (sk->merged) return fail(MHX_E_ARG, "this sketcher holds a merged table: mhx_sketcher_reset() first");
        const int rc = settle(sk);
        if (rc) return rc;
        uint64_t *w = (uint64_t *)d_slab, *d = sk->d_exp_hdr;
        HIPCHK(launch_extract(table_args(sk), 0, 1, w + 8, (uint32_t *)(w + 8 + cap_entries), (uint32_t)cap_entries, (uint32_t *)d, d + 2, sk->d_thresh, d + 1, d + 3,
                              g.stream, nullptr, 0, d, sk->h_exp_hdr, sk->d_done, d + 4, 8, w));
        HIPCHK(hipStreamSynchronize(g.stream));
        for (int i = 0; i < 8; ++i) header8[i] = sk->h_exp_hdr[i];
        sk->exported = header8[0];
        sk->export_valid = true;
        sk->last_T = header8[1];
        return MHX_OK;
    });
}

extern "C" int mhx_sketcher_merge_gathered(mhx_sketcher *sk, const void *d_slabs, uint32_t n_ranks, uint64_t cap_entries, uint32_t own_rank,
                                           uint64_t *hashes, uint32_t *counts, uint32_t *n_out, uint64_t *need_cap)
{
    return entry("mhx_sketcher_merge_gathered", [&]() -> int {
        if (sk) sk->mg_info = {};
        if (!sk || !d_slabs || !hashes || !n_out || !need_cap || n_ranks == 0 || (cap_entries & 1)) return fail(MHX_E_ARG, "merge_gathered: null argument or odd capacity");
        *need_cap = 0;
        const uint64_t slab_words = 8 + cap_entries + cap_entries / 2;
        std::vector<uint64_t> headers((size_t)n_ranks * 8);
        // the gathered headers: 64 bytes at the front of every slab
        HIPCHK(hipMemcpy2DAsync(headers.data(), 64, d_slabs, slab_words * sizeof(uint64_t), 64, n_ranks, hipMemcpyDeviceToHost, g.stream));
        HIPCHK(hipStreamSynchronize(g.stream));
        uint64_t max_n = 0;
        for (uint32_t r = 0; r < n_ranks; ++r) max_n = std::max(max_n, headers[8 * (size_t)r]);
        if (max_n > cap_entries) { // some slab is cut short: the caller repeats the exchange with room for all of it
            *need_cap = max_n;
            return fail(MHX_E_CAPACITY, "merge_gathered: a shard holds %llu entries, the slabs %llu", (unsigned long long)max_n, (unsigned long long)cap_entries);
        }
        return merge_slabs(sk, d_slabs, 1, n_ranks, cap_entries, headers.data(), own_rank, hashes, counts, n_out, 8);
    });
}

// Union of shard partials: sum the counts of equal hashes, keep count >= m, first s.
extern "C" int mhx_merge_partials(const uint64_t *hashes, const uint32_t *counts, uint64_t n, uint32_t s, uint32_t min_mult,
                                  uint64_t *out_hashes, uint32_t *out_counts, uint32_t *n_out)
{
    return guarded("mhx_merge_partials", [&]() -> int {
        clear_error();
        if ((!hashes || !counts) && n) return fail(MHX_E_ARG, "null input");
        if (!out_hashes || !n_out) return fail(MHX_E_ARG, "null output");
        std::vector<uint64_t> idx(n);
        for (uint64_t i = 0; i < n; ++i) idx[i] = i;
        std::sort(idx.begin(), idx.end(), [&](uint64_t a, uint64_t b) { return hashes[a] < hashes[b]; });
        uint32_t w = 0;
        const uint32_t m = min_mult ? min_mult : 1;
        for (uint64_t i = 0; i < n && w < s;) {
            uint64_t j = i, c = 0;
            while (j < n && hashes[idx[j]] == hashes[idx[i]]) c += counts[idx[j++]];
            if (c >= m) {
                out_hashes[w] = hashes[idx[i]];
                if (out_counts) out_counts[w] = saturated_count(c);
                ++w;
            }
            i = j;
        }
        *n_out = w;
        return MHX_OK;
    });
}

// The merge step of the sharded path WITH its exactness rule (what finish() checks on one GPU, applied to
// the union).  Below T_min = min_r T_r every shard's list is complete and its counts exact (a shard's
// threshold only ever falls, so a hash <= its final T_r was admitted on every occurrence).  Hence:
//   >= s merged entries with summed count >= m lie <= T_min  -> the first s are the sketch of the union;
//   T_min == hash_max (no shard ever rejected anything)      -> whatever qualifies is the (short) sketch;
//   otherwise the bound was too tight for this input         -> MHX_E_CAPACITY, never a short sketch.
// The decision uses gathered data only, so every rank reaches the same verdict.  (The entry 2^64-1 arrives here as an
// ordinary input entry: see merge_on_host.)
extern "C" int mhx_merge_shard_partials(const uint64_t *hashes, const uint32_t *counts, const uint64_t *shard_n,
                                        const uint64_t *shard_threshold, uint32_t n_shards, int k, uint32_t s, uint32_t min_mult,
                                        uint64_t *out_hashes, uint32_t *out_counts, uint32_t *n_out)
{
    return guarded("mhx_merge_shard_partials", [&]() -> int {
        clear_error();
        if (!shard_n || !shard_threshold || n_shards == 0) return fail(MHX_E_ARG, "null shard description");
        if (!out_hashes || !n_out || s == 0) return fail(MHX_E_ARG, "null output");
        if (k < 1 || k > 32) return fail(MHX_E_ARG, "k-mer size %d not supported (1..32)", k);
        const uint64_t hash_max = k <= 16 ? 0xFFFFFFFFull : ~0ull;
        uint64_t t_min = ~0ull, total = 0;
        for (uint32_t r = 0; r < n_shards; ++r) {
            t_min = shard_threshold[r] < t_min ? shard_threshold[r] : t_min;
            total += shard_n[r];
        }
        if ((!hashes || !counts) && total) return fail(MHX_E_ARG, "null input");
        std::vector<uint64_t> h;
        std::vector<uint32_t> c;
        h.reserve(total);
        c.reserve(total);
        for (uint64_t i = 0; i < total; ++i)
            if (hashes[i] <= t_min) { h.push_back(hashes[i]); c.push_back(counts[i]); }
        const int rc = mhx_merge_partials(h.data(), c.data(), h.size(), s, min_mult, out_hashes, out_counts, n_out);
        if (rc) return rc;
        if (!sketch_exact(*n_out, s, t_min, hash_max))
            return fail(MHX_E_CAPACITY, "sharded sketch not exact: %u of %u entries with multiplicity >= %u below the smallest shard threshold; "
                        "every rank must sketch its shard again with a larger budget_scale", *n_out, s, min_mult ? min_mult : 1);
        return MHX_OK;
    });
}
