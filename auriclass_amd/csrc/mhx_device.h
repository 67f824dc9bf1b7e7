// mhx_device.h -- argument structs and launchers shared between the HIP kernel files (mhx_*.hip) and the host
// engine (mhx_engine*.cpp, mhx_files*.cpp).  Internal; the public surface is include/mhx.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "mhx_device_consts.h"
#include "mhx_merge.h"

namespace mhx {

struct HashArgs {
    const uint8_t *base;   // 16-byte aligned; tiles are laid over base + [0, ...)
    uint64_t begin, end;   // logical span, byte offsets from base
    uint32_t tile0;        // first tile of this launch
    uint32_t ntiles;       // tiles in this launch (gridDim.x == ntiles * split)
    uint32_t first_tile;   // first tile of the push (its line phase is 0)
    uint32_t hash32;       // 1: keep the low 32 bits of the hash (k <= 16)
    uint32_t *ticket;      // zeroed before every launch
    uint64_t *tile_state;  // FASTQ look-back words, zeroed before every push
    const uint64_t *thresh; // admission threshold T (inclusive)
    uint64_t *keys;
    uint32_t *cnts;
    uint64_t slot_mask;
    uint64_t *stats;
    uint32_t *need_lookback; // FMT 2: set to 1 by a tile that could not find its line phase by itself (and did nothing else)
    uint32_t repair;         // FMT 1: repair pass -- tiles that CAN find their phase by themselves only publish it
    uint32_t queue_candidates; // kernel form: windows that pass the admission test are queued and finished after the hash loop (large sketches)
    uint8_t *phase_rec;      // FMT 2 / repair: one phase_record() per tile of the span (0: phase unknown), for phase_verify_kernel
    uint32_t probe;          // containment screen: keys / cnts are a screen table (mhx_screen.h) and the launch takes the probing kernels
    uint32_t split;          // workgroups per tile, a power of two <= 8 (1: the usual launch).  > 1: each one parses the tile and hashes one slice
                             // of its work list -- the first launch of a sketcher, inline kernels of formats 0 and 2 only (sketch_tile_kernel<.., SPLIT>)
};

struct TableArgs {
    uint64_t *keys;
    uint32_t *cnts;
    uint64_t nslots;
    uint64_t *thresh;
    uint32_t *hist;      // kHistBins counters, zero between rounds
    uint64_t *acc;       // kAccReplicas x 8 words: accumulators of the tighten pass (occupied, solid), zero between rounds
    uint64_t *stats;
    uint32_t *done;      // ticket of the tighten pass (its last workgroup computes the new threshold), zero between rounds
    uint32_t *need_lookback; // the sketcher's "repair pass due" word (HashArgs::need_lookback), reported by the extract kernel
    uint32_t min_mult;
    uint32_t sketch_size;
    uint32_t sample;     // tighten pass looks at one 256-slot block in `sample` (1 = exact pass)
    uint64_t next_cap;   // tighten pass, m > 1: byte-count cap to apply behind the new threshold (0: none), see cap_threshold_kernel
    const uint8_t *verify_rec; // tighten pass: HashArgs::phase_rec of the push it ends, whose chain it checks as phase_verify_kernel does (nullptr: no check)
    uint32_t verify_ntiles;    // ... and the number of tiles of that push
};

// the sketch tile kernel (mhx_sketch.hip)
hipError_t launch_hash(int k, int fmt, const HashArgs &a, hipStream_t st);
// passes over the candidate table (mhx_table.hip)
hipError_t launch_tighten(const TableArgs &a, uint32_t cus, hipStream_t st); // cus: compute units of the device (bounds the grid)
hipError_t launch_reset(const TableArgs &a, uint64_t t_init, uint32_t *tickets, uint32_t ntickets, uint32_t *out_n, hipStream_t st);
hipError_t launch_cap_threshold(uint64_t *thresh, uint64_t cap, uint64_t *stats, hipStream_t st);
hipError_t launch_order_block(const uint64_t *blk, uint32_t cap, uint32_t log2_buckets, uint32_t *cursor, uint32_t *starts,
                              uint32_t *group_total, uint64_t *grouped, uint64_t *host_blk, hipStream_t st);
hipError_t launch_phase_verify(const uint8_t *rec, uint32_t ntiles, uint64_t *stats, hipStream_t st);
// record check of the FASTQ span [begin, end) of base (mhx_fqcheck.hip): raises kFlagBadFastq in stats; scratch holds
// fastq_check_scratch_bytes(begin, end)
size_t fastq_check_scratch_bytes(uint64_t begin, uint64_t end);
hipError_t launch_fastq_check(const uint8_t *base, uint64_t begin, uint64_t end, void *scratch, uint64_t *stats, hipStream_t st);
// (mhx_table.hip)
hipError_t launch_extract(const TableArgs &a, uint64_t limit, uint32_t min_count, uint64_t *out_keys,
                          uint32_t *out_cnts, uint32_t cap, uint32_t *out_n, uint64_t *flags_out, const uint64_t *limit_dev,
                          uint64_t *limit_out, uint64_t *maxkey_out, hipStream_t st, uint32_t *order_cursor = nullptr, uint32_t order_log2 = 0,
                          uint64_t *hdr_dev = nullptr, uint64_t *hdr_host = nullptr, uint32_t *ticket = nullptr,
                          uint64_t *occ_out = nullptr, uint32_t nhdr = 4, uint64_t *hdr_copy = nullptr);

// containment screen (rules: mhx_screen.h, kernels: mhx_screen.hip): the screen table of a reference set, and what the reads left in it
struct ScreenArgs {
    const uint64_t *rows;   // [nr][stride] reference hash lists (ascending, unique within a row)
    const uint32_t *len;    // [nr] valid entries per row
    uint32_t nr, stride;
    uint64_t *keys;         // screen table
    uint32_t *cnts;
    uint64_t nslots;
    uint64_t *thresh;       // T_screen: the largest reference hash
    uint64_t *stats;        // the prober's counters (kStatReplicas x kStatCount)
    uint32_t *counts;       // tally: [nr][stride] count of every reference entry
    uint32_t *shared;       // tally: [nr] entries with a non-zero count
    uint32_t *median;       // tally: [nr] element [shared / 2] of the ascending non-zero counts (0: none)
};
hipError_t launch_screen_build(const ScreenArgs &a, hipStream_t st);  // vacates the table, inserts every reference hash, sets T_screen, then clears as launch_screen_clear
hipError_t launch_screen_clear(const ScreenArgs &a, uint32_t *tickets, uint32_t ntickets, uint32_t *need_lookback, hipStream_t st); // counters to zero, keys kept
hipError_t launch_screen_tally(const ScreenArgs &a, hipStream_t st);
// winner-take-all: win [nslots + 1] winner words at kScreenNobody, prio [nr] (screen_priorities), maxkey the occurrences of 2^64-1
hipError_t launch_screen_winner(const ScreenArgs &a, uint32_t *win, const uint32_t *prio, uint64_t maxkey, hipStream_t st);
hipError_t launch_screen_tally_winner(const ScreenArgs &a, const uint32_t *win, const uint32_t *prio, hipStream_t st);

// sharded path: the other ranks' gathered partial results go into this rank's candidate table (slab_insert_kernel, mhx_merge.hip)
// (kMaxMergeRanks ranks per launch, mhx_merge.h; more: several launches)
struct SlabMergeArgs {
    const uint64_t *slabs;  // device: nranks slabs of slab_words 8-byte words each: [hdr_words of header] hashes[cap] | counts u32[cap]
    uint64_t slab_words, cap;
    uint32_t hdr_words;
    uint64_t n[kMaxMergeRanks]; // valid entries of each slab (0: skip)
    uint32_t nranks, own_rank;  // own_rank: slab to skip (already in the table); >= nranks: none
    uint64_t t_min;
    uint64_t maxkey_others;     // occurrences of the hash value 2^64-1 on the other ranks
    uint64_t *keys;
    uint32_t *cnts;
    uint64_t slot_mask;
    uint64_t *thresh;
    uint64_t *stats;
};
hipError_t launch_slab_insert(const SlabMergeArgs &a, uint64_t max_n, hipStream_t st);

// sharded path, the usual case: the gathered slabs are binned by value and merged bin by bin in LDS (mhx_merge.hip)
struct MergeArgs {
    const uint64_t *slabs;      // device: nranks slabs of slab_words 8-byte words each: [hdr_words of header] hashes[cap] | counts u32[cap]
    uint64_t slab_words, cap;
    uint32_t hdr_words;
    uint64_t n[kMaxMergeRanks]; // valid entries of each slab
    uint32_t nranks;
    uint32_t min_mult;
    uint64_t t_min;
    uint32_t shift;             // bin of a hash = hash >> shift (< nbins for every hash <= t_min)
    uint32_t nbins;             // power of two, 256 .. kMergeMaxBins
    uint32_t region;            // entries a bin's region holds
    uint32_t table_slots;       // LDS table of merge_bin_kernel (power of two, >= 4/3 region)
    uint32_t chunk;             // slab entries per workgroup of the scatter pass (set by launch_merge_bins)
    uint32_t *cursor;           // [nbins] entries placed per bin; zero between merges (merge_bin_kernel clears it)
    uint32_t *qn;               // [nbins] qualifying entries per bin
    uint32_t *flags;            // [0]: kMergeFlag* of mhx_merge.h (a region or table overflowed, too many qualify in a bin, a count wrapped); zero between merges
    uint64_t *sc_keys;          // [nbins * region]
    uint32_t *sc_cnts;          // [nbins * region]
};
hipError_t launch_merge_bins(const MergeArgs &a, uint64_t max_n, uint64_t *out, uint32_t out_cap, hipStream_t st);
bool hash_k_supported(int k); // (mhx_sketch.hip)

// FASTA on the device (mhx_fasta.hip): raw file bytes -> dense sequence stream + record separator positions.
// ws: fasta_workspace_bytes(n) bytes; after the launch *(uint64_t *)(ws + o_off + 8 * ntiles) is the stream size,
// ((uint32_t *)(ws + o_flags))[0] the format flag (1: FASTQ syntax seen), [1] the number of separators.
constexpr int kFastaTile = 16384;
size_t fasta_workspace_bytes(uint64_t n, size_t *o_summary, size_t *o_in, size_t *o_off, size_t *o_flags);
hipError_t launch_fasta_compact(const uint8_t *base, uint64_t n, uint8_t *ws, uint8_t *out, uint64_t *seps, uint32_t seps_cap, hipStream_t st);

// segmented sketch (rules: mhx_segsketch.h, kernel: mhx_segsketch.hip): one workgroup per segment [seg_off[i], seg_off[i + 1])
// of the MHX_FMT_SEQ stream `bytes`; segments of at most kSegCut windows get min(s, stride, distinct) ascending hashes in
// rows[i][..] and their number in len[i], larger ones are left untouched (the host runs them through the sketcher).
// The aligned dwords around every segment must be readable.
hipError_t launch_segsketch(int k, const uint8_t *bytes, const uint64_t *seg_off, uint32_t n_seg, uint32_t s, uint64_t *rows,
                            uint32_t *len, uint32_t stride, hipStream_t st);

struct DistArgs {
    const uint64_t *q;
    const uint32_t *q_len;
    const uint64_t *r;
    const uint32_t *r_len;
    uint32_t nq, nr, stride, s;
    int k;
    uint32_t *common, *denom; // [nq][out_stride], this call fills columns out_off .. out_off + nr - 1
    double *dist;
    uint32_t out_stride, out_off;
};
hipError_t launch_dist_pairs(const DistArgs &a, hipStream_t st); // (mhx_dist.hip, like launch_dist_ranges below)

// all-vs-refs fast path (nr <= 32): value-range partition + LDS hash probe.  kDistRanges, kDistTableSlots, kDistSegs and
// the geometry rule (dist_windows) are in mhx_dist.h, with the logic the kernels share with the CPU emulator; this header
// does not include it (mhx_dist.hip and mhx_engine_dist.cpp do), so that a change there rebuilds those two alone.
#ifndef MHX_DIST_QCHUNKS
#define MHX_DIST_QCHUNKS 4
#endif
constexpr int kDistQueryChunks = MHX_DIST_QCHUNKS;   // query chunks per range (grid.y of the range kernel)
struct DistWork {
    uint32_t *offs_q;   // [nq][ranges + 1] first index of every range in each query list
    uint32_t *offs_r;   // [nr][ranges + 1]
    uint8_t *cpart;     // [nq][ranges][4 * ceil(nr / 4)] shared hashes per (query, range, ref), one byte each
    uint32_t *params;   // [0] shift, [1] overflow flag
    uint32_t *wtot;     // windowed form only: [nq][ranges / kDistWindowRanges][4 * ceil(nr / 4)] shared hashes per (query, window, ref)
    uint32_t ranges;    // kDistRanges * W (mhx_dist.h: dist_windows); kDistRanges = the base form, whose kernels do not read this
};
// workspace of one (query batch, reference slice) block; with ranges == kDistRanges the layout of the base form (no wtot)
size_t dist_work_bytes(uint32_t nq, uint32_t nr, uint32_t ranges, size_t *off_q, size_t *off_r, size_t *off_c, size_t *off_w, size_t *off_p);
hipError_t launch_dist_ranges(const DistArgs &a, const DistWork &w, hipStream_t st);
// The passes of the windowed form one by one (R = w.ranges, any power of two >= 16), for a caller whose offs_q and offs_r
// point into ONE [list][R + 1] table of a whole set: shift + split of the a.nq lists of a.q (a.nr = 0) into w.offs_q; the
// range pass of one block; the finish pass of one block with R >= 1024 (below: launch_tri_finish_small).
hipError_t launch_dist_offsets(const DistArgs &a, const DistWork &w, hipStream_t st);
// the same for two sets that share their ranges (the search): one shift over a.q and a.r, offsets into w.offs_q and w.offs_r
hipError_t launch_dist_offsets_both(const DistArgs &a, const DistWork &w, hipStream_t st);
hipError_t launch_dist_range_pass(const DistArgs &a, const DistWork &w, hipStream_t st);
hipError_t launch_dist_finish(const DistArgs &a, const DistWork &w, hipStream_t st);

// all pairs within one set (rules: mhx_triangle.h, kernels: mhx_triangle.hip).  A block's results lie block-local in
// loc_common / loc_denom [nq][32]; `flag` is the block's overflow word (non-zero: the results are not there, nothing is done).
struct TriOut {
    const uint32_t *loc_common, *loc_denom;
    const uint32_t *flag;
    uint32_t r0, nr, q0, nq; // the block (mhx_triangle.h: TriBlock)
    int k;
    // dense mode: packed outputs at tri_index(q, r)
    uint32_t *common, *denom;
    double *dist;            // may be null
    // edge mode: pairs that count and pass tri_keep(., ., jmin) are appended through *count; beyond cap they are only counted
    uint32_t *edge_i, *edge_j;
    unsigned long long *count;
    uint64_t cap;
    double jmin;
};
hipError_t launch_tri_finish_small(const DistArgs &a, const DistWork &w, hipStream_t st); // 16 <= w.ranges < 1024
hipError_t launch_tri_scatter(const TriOut &o, hipStream_t st);
hipError_t launch_tri_edges(const TriOut &o, hipStream_t st);

// single-linkage clustering of one set (rules: mhx_cluster.h, kernels: mhx_cluster.hip): a block's results, block-local as
// above, feed a union-find over parent[n] instead of an output of pairs
struct ClusterOut {
    const uint32_t *loc_common, *loc_denom;
    const uint32_t *flag;
    uint32_t r0, nr, q0, nq; // the block (mhx_triangle.h: TriBlock)
    const uint32_t *cmin;    // [s + 1] the bound as integers: a pair is an edge iff common >= cmin[denom]
    uint32_t s;
    uint32_t *parent;        // [n] set up by launch_cluster_init; the labels after the last launch_cluster_flatten
    uint32_t *degree;        // [n] neighbours of every list, may be null
    unsigned long long *n_edges;
};
hipError_t launch_cluster_init(uint32_t *parent, uint32_t *degree, uint32_t n, hipStream_t st);
hipError_t launch_tri_cluster(const ClusterOut &o, hipStream_t st);
// parent[i] = the root of i, in a launch of its own; count (may be null) receives the number of roots on top of what it holds
hipError_t launch_cluster_flatten(uint32_t *parent, uint32_t n, unsigned long long *count, hipStream_t st);

// medoids of a partition of one set (rules: mhx_medoid.h, kernels: mhx_medoid.hip): a block's results, block-local as above,
// add the distances of the pairs inside a cluster to sum[n]; then the pick, and the pair of every list with its target
struct MedoidOut {
    const uint32_t *loc_common, *loc_denom;
    const uint32_t *flag;
    uint32_t r0, nr, q0, nq; // the block (mhx_triangle.h: TriBlock)
    const uint32_t *label;   // [n] the partition: label[i] the lowest index of i's cluster, checked by the host
    unsigned long long *sum; // [n] zero before the first block
    int k;
};
struct DistToArgs {
    const uint64_t *rows;
    const uint32_t *len;
    uint32_t n, stride, s;
    const uint32_t *target;   // [n] below n, checked by the host
    uint32_t *common, *denom; // [n] the pair (i, target[i])
};
hipError_t launch_tri_medoid(const MedoidOut &o, hipStream_t st);
// best [n] at all ones before the launch; medoid[i] = the member of i's cluster with the smallest (sum, index)
hipError_t launch_medoid_pick(const uint32_t *label, const unsigned long long *sum, unsigned long long *best, uint32_t *medoid, uint32_t n, hipStream_t st);
hipError_t launch_dist_to(const DistToArgs &a, hipStream_t st);

// single-linkage tree of one set (rules: mhx_mst.h, kernels: mhx_mst.hip): the passes of one Boruvka round.  best [n] holds
// the best outgoing edge of every list (mst_pack), winner [n] the list that stands for a component, comp [n] the flattened
// parent of the round before (read-only within a round), parent [n] the union-find the hooks write.
struct MstOut { // propose, recomputed source: a block's results, block-local as above
    const uint32_t *loc_common, *loc_denom;
    const uint32_t *flag;
    uint32_t r0, nr, q0, nq; // the block (mhx_triangle.h: TriBlock)
    const uint32_t *comp;
    uint64_t *best;
};
struct MstScan { // propose, stored source: the packed triangle of mhx_dist_triangle's dense mode
    const uint32_t *common, *denom;
    uint32_t n;
    const uint32_t *comp;
    uint64_t *best;
};
struct MstHookArgs {
    const uint32_t *comp, *winner;
    const uint64_t *best;
    uint32_t *parent;
    uint32_t n;
    int k;
    uint32_t *edge_i, *edge_j, *common, *denom; // [cap] the result, appended through *n_edges
    double *dist;                               // may be null
    unsigned long long *n_edges;
    uint64_t cap;
};
hipError_t launch_mst_reset(uint64_t *best, uint32_t *winner, uint32_t n, hipStream_t st);
hipError_t launch_tri_mst(const MstOut &o, hipStream_t st);
hipError_t launch_mst_scan(const MstScan &o, hipStream_t st);
hipError_t launch_mst_choose(const uint64_t *best, const uint32_t *comp, uint32_t *winner, uint32_t n, hipStream_t st);
hipError_t launch_mst_hook(const MstHookArgs &o, hipStream_t st);

// complete- and average-linkage agglomeration of one set (rules: mhx_linkage.h, kernels: mhx_linkage.hip): one 64-bit word
// per cluster pair at the triangle's packed index, and the three launches of a step
struct LinkArgs {
    uint64_t *words;       // [n (n - 1) / 2]
    uint32_t *size, *nn;   // [n] each: members of cluster i (0: none), the best active partner below i
    uint32_t n;
    int linkage, k;        // kLinkComplete / kLinkAverage
    uint32_t *list;        // [n] rows to scan again, appended through ctl[4]
    uint32_t *ctl;         // [0 .. 3] the pick of the step (LinkPick), [4] rows on the list, [5] non-zero: a pick found no pair
    unsigned long long *total; // rows scanned again in all steps before the last pick
    uint32_t *merge_a, *merge_b, *size_out; // [n - 1] the result, entry t written by step t
    uint64_t *num, *den;
    double *dist;          // may be null
};
hipError_t launch_link_init(const LinkArgs &a, const uint32_t *common, const uint32_t *denom, hipStream_t st);
hipError_t launch_link_pick(const LinkArgs &a, uint32_t t, hipStream_t st);
hipError_t launch_link_update(const LinkArgs &a, hipStream_t st);
hipError_t launch_link_rescan(const LinkArgs &a, hipStream_t st);

// neighbour joining over one set (rules: mhx_nj.h, kernels: mhx_nj.hip): one 64-bit distance word per pair of nodes at the
// triangle's packed index, the row sums r, the compacted list of active ids with the running sums of their row lengths (twice:
// join t reads copy t & 1, its update writes the other), and the three launches of a join
struct NjCand;
struct NjArgs {
    uint64_t *words;       // [n (n - 1) / 2]
    uint64_t *r;           // [n]
    uint32_t n;
    int k;
    uint32_t *act[2];      // [n] each
    uint64_t *pre[2];      // [n + 1] each
    NjCand *cand;          // [kNjMaxBlocks] the candidates of the scan's workgroups
    uint64_t *ctl;         // [0 .. 3] the pick of the step (NjPick: a, b, pos_a, d), [4] updates the clamp changed, [5] non-zero: a join found no pair
    uint32_t *join_a, *join_b; // [n - 1] the result, entry t written by join t
    uint64_t *d, *r_a, *r_b;
    double *len_a, *len_b; // may be null
};
hipError_t launch_nj_init(const NjArgs &a, const uint32_t *common, const uint32_t *denom, hipStream_t st);
hipError_t launch_nj_scan(const NjArgs &a, uint32_t t, hipStream_t st);   // join t among n - t > 2 nodes
hipError_t launch_nj_join(const NjArgs &a, uint32_t t, hipStream_t st);
hipError_t launch_nj_update(const NjArgs &a, uint32_t t, hipStream_t st); // n - t > 2

// the jackknife over the hashes of one set (rules: mhx_resample.h, kernels: mhx_resample.hip): replicate `replicate` of rows /
// len [n] into out_rows / out_len (the same stride, another place), and the smallest kept count of the full lists in *s_r
struct ResampleArgs {
    const uint64_t *rows;
    const uint32_t *len;
    uint32_t n, stride, s;
    uint64_t seed, threshold; // threshold: T of mhx_resample.h, 1 .. 2^32
    uint32_t replicate;
    uint64_t *out_rows;
    uint32_t *out_len;
    uint32_t *s_r;            // one word
};
// *s_r = s, then the kept hashes of every row in order, their count and the minimum over the full rows into *s_r
hipError_t launch_resample(const ResampleArgs &a, hipStream_t st);
// every out_len cut to *s_r and the rows zero behind it up to the stride
hipError_t launch_resample_clamp(const ResampleArgs &a, hipStream_t st);

// jackknife support of search hits (rules: mhx_support.h, kernels: mhx_support.hip): one batch of queries, everything on the
// device.  q / q_len / cand / n_cand and the outputs point at the batch's first query; cand null: candidates 0 .. top - 1.
struct SupportArgs {
    const uint64_t *q, *r;
    const uint32_t *q_len, *r_len;
    uint32_t nq, nr, stride, s;
    const uint32_t *cand, *n_cand; // [nq][top], [nq]
    uint32_t top, replicates;
    uint64_t seed, threshold;      // threshold: T of mhx_resample.h
    uint32_t q0;                   // the batch's first query within the call, for *bad
    uint32_t *kept;                // [nq][top + 1][replicates] slot 0 the query, slot 1 + i candidate i
    uint32_t *s_r;                 // [nq][replicates]
    uint32_t *common, *denom;      // [nq][top][replicates]
    uint32_t *best;                // [nq][replicates] may be null
    uint32_t *first;               // [nq][top], zero before the launch
    unsigned long long *bad;       // the smallest (query << 32 | replicate) whose s_r is 0; all ones before the first batch
};
hipError_t launch_support_count(const SupportArgs &a, hipStream_t st); // kept
hipError_t launch_support_s(const SupportArgs &a, hipStream_t st);     // s_r, *bad
hipError_t launch_support_pairs(const SupportArgs &a, hipStream_t st); // common, denom
hipError_t launch_support_best(const SupportArgs &a, hipStream_t st);  // best, first

// reference-set search (rules: mhx_search.h, kernels: mhx_search.hip).  A block's results lie block-local as above; every
// query of the call has a best list of at most `top` hits, best first, in hit_ref / hit_common / hit_denom [queries][top]
// with its length in n_hits [queries] (zero before the first block), which the take-out pass of every block merges into.
struct SearchOut {
    const uint32_t *loc_common, *loc_denom;
    const uint32_t *flag;
    uint32_t r0, nr, q0, nq; // the block (mhx_search.h: SearchBlock); q0 counts from the call's first query
    uint32_t top;
    int k;
    double jmin;             // candidates must pass tri_keep(., ., jmin)
    uint32_t *hit_ref, *hit_common, *hit_denom;
    uint32_t *n_hits;
    double *hit_dist;        // launch_search_dist only
};
hipError_t launch_search_take(const SearchOut &o, hipStream_t st);
// tri_distance of the o.nq lists from query o.q0 on into hit_dist (entries behind n_hits are left alone)
hipError_t launch_search_dist(const SearchOut &o, hipStream_t st);

// all references within a distance of each query, as CSR (rules: mhx_within.h, kernels: mhx_within.hip).  A block's results
// lie block-local as above; the queries of a super-batch have one cell per slice of 32 references in mask / base
// [queries][nslices], which the take-out pass of every block fills: the ballot of the exact integer rule, and where the
// cell's keepers begin in the arrival list arr_common / arr_denom [room] (appended through *count, zero before the first
// block of the super-batch; at or beyond room they are only counted).  base null: the counting form, no list.
struct WithinOut {
    const uint32_t *loc_common, *loc_denom;
    const uint32_t *flag;    // non-zero: nothing is done
    uint32_t r0, nr, q0, nq; // the block (mhx_search.h: SearchBlock); q0 counts from the super-batch's first query
    const uint32_t *cmin;    // [s + 1] the bound as integers: a pair is a hit iff common >= cmin[denom]
    uint32_t s, nslices;
    uint32_t *mask, *base;
    uint32_t *arr_common, *arr_denom;
    uint32_t room;
    uint32_t *count;
};
hipError_t launch_within_take(const WithinOut &o, hipStream_t st);
// Behind the last block and the last fallback of a super-batch of nq queries.  row_off points at the entry of its first
// query, which holds the hits of all queries before it (0 for the first super-batch of a call).
struct WithinRows {
    const uint32_t *mask, *base;
    uint32_t nq, nslices;
    uint64_t *row_off;       // [nq + 1]
    const uint32_t *arr_common, *arr_denom;
    uint32_t room;
    uint32_t *hit_ref, *hit_common, *hit_denom; // [cap] of the call
    double *hit_dist;        // may be null
    uint64_t cap;
    int k;
};
// row_off[1 .. nq]: the scan of the set bits of every query's cells, on top of row_off[0]
hipError_t launch_within_scan(const WithinRows &o, hipStream_t st);
// every cell's keepers from the arrival list to their final place (mhx_within.h: within_dest); places at or beyond cap are left out
hipError_t launch_within_gather(const WithinRows &o, hipStream_t st);

// containment of the references in the queries (rules: mhx_contain.h, kernels: mhx_contain.hip).  The two sets have a sketch
// size each; eff / bound [lists] are written once per call by launch_contain_bounds and read by the other two, and the
// passes of mhx_dist.hip that the range route reuses take eff for their lengths.  Results go straight to [q][r] of the
// call's outputs, `out_stride` (the call's nr) words per query: cell (q, r) is q * out_stride + r - out_base.  out_base is zero
// in mhx_dist_contain; the containment search sets out_stride = 32 and out_base = q0 * 32 + r0, which makes the outputs the
// block-local [bnq][32] arrays its take-out pass reads.
struct ContainArgs {
    const uint64_t *q, *r;           // [.][stride] the rows of the call
    const uint32_t *q_len, *r_len;   // as the caller gave them (launch_contain_bounds only)
    uint32_t nq, nr, stride, s_q, s_r;
    uint32_t *q_eff, *r_eff;         // [nq], [nr] contain_eff_len
    uint64_t *q_bound, *r_bound;     // [nq], [nr] contain_bound
    uint32_t q0, bnq, r0, bnr;       // the block (mhx_search.h: SearchBlock)
    const uint32_t *shift;           // range route: the word that holds the call's shift
    uint32_t *shared, *n_qry, *n_ref;
    uint32_t out_stride;
    uint64_t out_base;               // taken off every cell index (finish pass and pair kernel); zero: the call's [nq][nr]
};
hipError_t launch_contain_bounds(const ContainArgs &a, hipStream_t st);
// the finish pass of one block over w (offsets of the block's lists, byte counters, w.params[1] the block's flag: non-zero,
// nothing is done); 16 <= w.ranges <= kDistRanges
hipError_t launch_contain_finish(const ContainArgs &a, const DistWork &w, hipStream_t st);
// the generic form: one workgroup per pair of the block
hipError_t launch_contain_pairs(const ContainArgs &a, hipStream_t st);

// winner-take-all containment (rules: mhx_contain_winner.h, kernels: mhx_contain_winner.hip) over the outputs of the plain
// pass: a batch of a.bnq queries from a.q0 on against ALL a.nr references.  words [a.bnq][width] are the winner words of the
// batch, one per position of a query's list (width >= every effective query length), zeroed by the caller.
struct ContainWinnerArgs {
    uint32_t *words;
    uint32_t width;
    const uint64_t *ref_length;   // [nr] genome lengths, or null: all equal
    uint32_t *won;                // [nq][out_stride], zeroed by the caller once per call
    unsigned long long *pairs;    // the pairs the claim pass walked (shared > 0), added up over the call
};
// the claim pass: one workgroup per pair; a pair with shared == 0 ends after that one load
hipError_t launch_contain_claim(const ContainArgs &a, const ContainWinnerArgs &w, hipStream_t st);
// the tally: one thread per word of the batch
hipError_t launch_contain_tally(const ContainArgs &a, const ContainWinnerArgs &w, hipStream_t st);

// containment search (rules: mhx_contain_search.h, kernel: mhx_contain_search.hip).  A block's three counts lie block-local,
// [queries of the block][32]; every query of the call has a best list of at most `top` hits, best first, in hit_ref /
// hit_shared / hit_n_ref / hit_n_qry [queries][top] with its length in n_hits [queries] (zero before the first block), which
// the take-out pass of every block merges into.  need [need_limit + 1]: the hit test, shared >= need[n_ref].
struct ContainSearchOut {
    const uint32_t *loc_shared, *loc_n_qry, *loc_n_ref;
    const uint32_t *flag;    // non-zero: nothing is done
    uint32_t r0, nr, q0, nq; // the block (mhx_search.h: SearchBlock); q0 counts from the call's first query
    uint32_t top;
    const uint32_t *need;
    uint32_t need_limit;
    uint32_t *hit_ref, *hit_shared, *hit_n_ref, *hit_n_qry;
    uint32_t *n_hits;
};
hipError_t launch_contain_take(const ContainSearchOut &o, hipStream_t st);

// all references a query holds, as CSR (rules: mhx_contain_within.h, kernels: mhx_contain_within.hip).  A block's three counts
// lie block-local as for the containment search; the queries of a super-batch have one cell per slice of 32 references in
// mask / base [queries][nslices] as in WithinOut, which the take-out pass of every block fills: the ballot of
// shared >= need[n_ref], and where the cell's keepers begin in the arrival list arr_shared / arr_n_ref / arr_n_qry [room]
// (appended through *count, zero before the first block of the super-batch; at or beyond room they are only counted).
// base null: the counting form, no list.
struct ContainWithinOut {
    const uint32_t *loc_shared, *loc_n_qry, *loc_n_ref;
    const uint32_t *flag;    // non-zero: nothing is done
    uint32_t r0, nr, q0, nq; // the block (mhx_search.h: SearchBlock); q0 counts from the super-batch's first query
    const uint32_t *need;
    uint32_t need_limit, nslices;
    uint32_t *mask, *base;
    uint32_t *arr_shared, *arr_n_ref, *arr_n_qry;
    uint32_t room;
    uint32_t *count;
};
hipError_t launch_contain_within_take(const ContainWithinOut &o, hipStream_t st);
// Behind the last block, the last fallback and launch_within_scan of a super-batch of nq queries: every cell's keepers from
// the arrival list to their final place (mhx_within.h: within_dest); places at or beyond cap are left out.  row_off points at
// the entry of the super-batch's first query.
struct ContainWithinRows {
    const uint32_t *mask, *base;
    uint32_t nq, nslices;
    const uint64_t *row_off; // [nq + 1]
    const uint32_t *arr_shared, *arr_n_ref, *arr_n_qry;
    uint32_t room;
    uint32_t *hit_ref, *hit_shared, *hit_n_ref, *hit_n_qry; // [cap] of the call
    uint64_t cap;
};
hipError_t launch_contain_within_gather(const ContainWithinRows &o, hipStream_t st);

} // namespace mhx
