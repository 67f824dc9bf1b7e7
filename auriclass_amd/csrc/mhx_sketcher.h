// mhx_sketcher.h -- the sketcher object as the host engine sees it: mhx_engine.cpp owns it, mhx_engine_merge.cpp exports
// and merges its table across shards, mhx_engine_screen.cpp runs a screener on top of one in screen mode.  Internal to
// those three; the other callers hold an mhx_sketcher by pointer only (mhx_engine_internal.h).
#pragma once
#include <algorithm>
#include <vector>

#include "mhx_engine_internal.h"

using mhx::DevArray; // (mhx_sketcher is the C type of include/mhx.h: global scope)
using mhx::PinnedArray;

struct SortScratch {
    std::vector<uint32_t> start;
    std::vector<uint64_t> keys;
    std::vector<uint32_t> cnts;
};

struct MergeInfo {
    uint32_t path = 0;        // kMergePath* (mhx_merge.h): what produced the answer; 0: no merge yet, or the last call ended in an error before any path ran (cleared at the entry of every merge call)
    uint32_t attempted = 0;   // 1: the binned merge ran; flags / nbins / region / table_slots are its
    uint32_t flags = 0;       // kMergeFlag* the binned attempt returned
    uint32_t nbins = 0, region = 0, table_slots = 0;
};

struct mhx_sketcher {
    SortScratch sorted;            // finish() / export(): the extracted entries in hash order
    int k = 0;
    uint32_t s = 0, m = 1;
    bool hash32 = false;
    uint64_t nslots = 0;
    uint64_t hash_max = 0;   // largest representable hash (2^64-1 or 2^32-1)
    uint64_t t_init = 0;     // initial admission threshold (everything admitted)
    // device
    DevArray<uint64_t> d_keys;
    DevArray<uint32_t> d_cnts;
    DevArray<uint64_t> d_thresh;
    DevArray<uint32_t> d_hist;
    DevArray<uint64_t> d_acc;
    DevArray<uint64_t> d_stats;   // kStatReplicas x kStatCount
    DevArray<uint32_t> d_tickets; // one per tile launch since the last reset (kTicketWords of them)
    uint32_t tickets_used = 0;
    DevArray<uint32_t> d_done;    // ticket of the tighten pass
    DevArray<uint8_t> d_phase_rec; // FASTQ: phase_record() per tile of the span being pushed (chain check)
    DevArray<uint32_t> d_need;    // FASTQ: some tile could not find its line phase by itself -> repair pass due
    struct Span { const void *ptr; uint64_t n; };
    std::vector<Span> unsettled;   // FASTQ pushes whose repair question is still open (their buffers are valid until the next sync)
    DevArray<uint64_t> d_tile_state;
    DevArray<uint8_t> d_stage;
    DevArray<uint64_t> d_out_keys;
    DevArray<uint32_t> d_out_cnts;
    DevArray<uint32_t> d_out_n;
    uint32_t out_cap() const { return (uint32_t)std::min(d_out_keys.cap(), d_out_cnts.cap()); }
    // sharded path: header of the shard export [n, T, flags, #(2^64-1), occupied, 0, 0, 0], accumulated on the device and
    // handed to the pinned mirror by the extract kernel itself (the entries stay in d_out_keys / d_out_cnts)
    DevArray<uint64_t> d_exp_hdr;
    PinnedArray<uint64_t> h_exp_hdr;
    uint64_t exported = 0;     // entries of the last export_begin (valid until the next push / reset)
    bool export_valid = false;
    bool merged = false;       // merge_slabs has added other shards' entries to the table: reset before the next push
    bool verify_fastq = false; // file-level callers: FASTQ4 pushes also run the record check (sketcher_verify_fastq)
    DevArray<uint64_t> d_merge_in; // staging of gathered slabs that arrive in host memory (gloo)
    // workspace of the binned merge (mhx_merge.hip): per-bin cursors / counts / flags (kept zero between merges by the
    // kernels), bin regions
    DevArray<uint32_t> d_mg_small;  // [kMergeMaxBins] cursor | [kMergeMaxBins] qn | [16] flags
    DevArray<uint64_t> d_mg_keys;
    DevArray<uint32_t> d_mg_cnts;
    MergeInfo mg_info;             // the last merge on this sketcher (mhx_sketcher_merge_info)
    // finish(): one device block [n, T, flags, #(2^64-1) | hashes[fin_cap] | counts[fin_cap]] and its pinned host
    // mirror, so the result comes back in ONE copy (five separate copies cost 20-60 us of idle gap each)
    DevArray<uint64_t> d_fin;
    PinnedArray<uint64_t> h_fin;
    uint32_t fin_cap = 0;
    // large sketches: a second block, the first in (almost) hash order (launch_order_block), and its bucket counters
    DevArray<uint64_t> d_fin_ordered;
    DevArray<uint32_t> d_order_buckets, d_order_starts, d_order_groups;
    uint32_t order_log2 = 0;
    bool table_dirty = true;   // tiles have been hashed since the last EXACT tighten pass
    bool table_sampled = false; // ... but a sampled pass has run after the last of them: T is valid and ~s' solid hashes lie below it
    // host
    uint64_t next_chunk_bytes = 0; // geometric schedule of the tightening phase
    uint64_t bytes_pushed = 0;
    uint64_t repair_next_chunk_bytes = 0; // the same two for the FASTQ repair passes: the schedule the left-out tiles would
    uint64_t repair_bytes = 0;            // have had on their own (T is at least as low as that schedule assumes)
    uint64_t expected_bytes = 0;
    uint64_t admit_scale = 1;      // multiplies the initial admission budget (retries after MHX_E_CAPACITY)
    double hash_ms = 0.0;
    uint64_t launches = 0;
    uint64_t last_T = 0;
    // m > 1 only: until s hashes with count >= m exist below T the table is protected by a bound that
    // follows the input seen so far (see push_device)
    bool bounded = false;      // as of the last finish(): the byte-count cap has limited T at least once (m > 1)
    bool established = false;  // as of the last finish(): a tighten pass has lowered T from solid (count >= m) entries
    uint64_t occupied = 0;     // table occupancy reported by the last tighten pass
    uint64_t solid = 0;        // entries <= T with count >= m reported by the last tighten pass
    // containment screen (mhx_screener below): d_keys / d_cnts are a screen table built from reference sketches and
    // d_thresh holds T_screen, which never moves -- a push is ONE launch of the probing kernels, no tighten pass, no stages
    bool screen = false;
    uint64_t screen_T = 0;     // T_screen as the host knows it (chooses the kernel form)
    // file-level screen: the prober of a screener rides along with the sketcher the ingest feeds -- every span pushed here is
    // pushed there too, and whatever settles this sketcher's pushes settles the follower's (sketcher_set_follower)
    mhx_sketcher *follower = nullptr;
};

namespace mhx {

constexpr uint32_t kTicketWords = 4096; // tile launches between two clears of the ticket words

// ---- when a sketch is exact: one rule for finish(), the binned merge and mhx_merge_shard_partials -----------------------
// Below a threshold T every hash was admitted on every occurrence, so the list of qualifying (count >= m) entries <= T is
// complete and its counts exact.  Either nothing was ever rejected (T still at hash_max) and whatever qualifies is the
// (possibly short) sketch, or at least s qualifying entries lie below T and the first s are the sketch.  Fewer than s
// below a lowered T means the bound was too tight for this input: MHX_E_CAPACITY, never a short sketch.  Each caller
// says so in its own words.
inline bool sketch_exact(uint64_t qualifying, uint32_t s, uint64_t T, uint64_t hash_max) { return qualifying >= s || T >= hash_max; }
// The one hash value no table holds, 2^64-1 (kEmptyKey marks a vacant slot): its occurrences travel as a number beside
// the table, and it is an entry of the result -- the last one -- when nothing was ever rejected and it qualifies.
inline bool has_max_key_entry(uint64_t T, uint64_t occurrences, uint32_t m) { return T == ~0ull && occurrences >= m; }
// Its count, and every summed count of a merge, saturates at 2^32-1 (max_key_count, mhx_merge_partials) -- except in
// finish(), which has always truncated the occurrences of 2^64-1 to their low 32 bits and still does.
inline uint32_t saturated_count(uint64_t c) { return c > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)c; }

struct TableArgs;
TableArgs table_args(mhx_sketcher *sk); // the sketcher's table as the table kernels take it (mhx_engine.cpp)

// the sketcher calls a screener makes on its prober (mhx_engine.cpp)
int settle(mhx_sketcher *sk);                      // decides the repair question of every unsettled FASTQ push
int fetch_stats(mhx_sketcher *sk, uint64_t *sum);  // the device counters, summed over their replicas
int check_flags(uint64_t flags);                   // device flags -> error code

} // namespace mhx
