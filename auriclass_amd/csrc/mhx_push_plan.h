// mhx_push_plan.h -- the schedule of a sketcher push (mhx_engine.cpp: push_span carries it out): how many tiles every launch
// takes, the threshold cap of the multiplicity filter in front of it, the kernel form, the split of a fresh sketcher's first
// launch and which tighten pass checks the FASTQ phase chain.  Host arithmetic on plain numbers: no HIP header, nothing that
// includes one, so the CPU tests run it as it is (tests/emul/push_plan_emul.cpp against tests/push_rule.py).
#pragma once
#include <math.h>
#include <stdint.h>

#include <algorithm>

#include "mhx_device_consts.h"

namespace mhx {

constexpr uint32_t kDeviceOrderMinSketch = 8192; // sketches from here on are ordered on the device (finish()) and queue their candidates

constexpr int kMaxLaunchesPerPush = 64;
#ifndef MHX_CHUNK_GROWTH
#define MHX_CHUNK_GROWTH 16
#endif
constexpr uint64_t kChunkGrowth = MHX_CHUNK_GROWTH; // smallest chunk size ratio between tighten rounds
constexpr uint64_t kUncappedBytes = 1u << 20;       // m > 1: prefix of the input that is admitted whole

inline uint64_t next_pow2(uint64_t v)
{
    uint64_t p = 1;
    while (p < v) p <<= 1;
    return p;
}

// the chunk a reset sketcher starts from (next_chunk_bytes, and its repair twin)
inline uint64_t first_chunk_bytes(uint32_t s, uint32_t m, uint64_t nslots)
{
    uint64_t c0 = next_pow2((uint64_t)s * 64);
    if (c0 < (1u << 20)) c0 = 1u << 20;
    if (m > 1) c0 = kUncappedBytes; // multiplicity filter: the first stage is admitted whole (see PushPlan)
    if (c0 > nslots / 4) c0 = nslots / 4; // first chunk may admit every position
    return c0;
}

// tiles of a span that ends `end` bytes behind its 16-byte aligned base
inline uint64_t span_tiles(uint64_t end) { return (end + kTileBytes - 1) / kTileBytes; }

// Kernel form of a launch (process_group_regs) from the share of the windows that will pass the admission test:
// candidates are queued when many will -- a large sketch, or a threshold above ~3 candidates in 10^4 windows --, and
// finished where they are found otherwise.
// (a sequence stream fills the work list -- every group of a tile is an item --, which leaves the queue no room;
// above ~0.15 candidates per window the ~1100 free entries of a FASTQ tile's list overflow and the tile would do
// its work twice, see sketch_tile_kernel: such launches finish their candidates inline)
// forced: the diagnostic override, 0 or 1 (it wins, whatever the format), negative: none.
inline uint32_t queue_form(int kfmt, uint32_t s, long double expected_rate, int forced)
{
    if (forced >= 0) return (uint32_t)(forced != 0);
    return (uint32_t)(kfmt != 0 && expected_rate <= 0.1L && (s >= kDeviceOrderMinSketch || expected_rate > 3e-4L));
}

struct PushConsts { // what the schedule reads of a sketcher
    uint32_t s, m;
    uint64_t nslots, hash_max, admit_scale;
};

struct PushStep { // one launch of the tile kernel and the tighten pass behind it
    uint32_t tile0, ntiles;
    uint32_t split;            // HashArgs::split
    uint32_t queue_candidates; // HashArgs::queue_candidates
    uint64_t cap_before;       // m > 1, first launch of a push: T is capped here by a launch of its own in front (0: none)
    uint64_t next_cap;         // the cap of the NEXT launch of this push, applied by the tighten pass behind this one (0: none)
    bool verify_chain;         // that pass also checks the phase chain of the push
    uint64_t bytes_pushed, next_chunk_bytes; // the sketcher's two counters once this launch is on the stream: the caller's to store then
};

// The host never looks at T while pushing: every launch is followed by a tighten pass on the stream and nothing
// waits for a round trip.
// No multiplicity filter: launches grow by a factor G.  After a chunk of N k-mers T sits at the s-th smallest of
// them, hence the next, G times larger chunk admits ~G*s occurrences: G is what keeps that at a sixteenth of the
// table whatever the input is.
// Multiplicity filter (m > 1): T cannot follow the data before s hashes with count >= m exist, and until then
// every admitted k-mer costs two atomics and may be a new table entry.  The first MiB is admitted whole (small
// genomes and saturated k-mer spaces show their solid hashes there); after that the bytes seen grow x8 (m <= 3) or x4 per launch
// and, in front of every launch, T is capped ON THE DEVICE at 48*s' / (bytes seen after this launch),
// s' = s + 8*sqrt(s) + 16, i.e. ~20*s admissions per stage -- unless a tighten pass has meanwhile lowered T from
// solid hashes, or the table looks like a small genome sequenced deeply (cap_threshold_kernel; inside a push the
// tighten pass in front of the launch applies the cap itself, TableArgs::next_cap).  The cap stays
// above the final s-th solid hash for any genome size while the error-free k-mer coverage c so far is <= ~17x,
// and s solid hashes appear below it as soon as c / P[Poisson(c) >= m] <= 17 (c in 0.8 .. 16 for m = 3), a window
// no x4 stage can jump over.  Inputs with fewer than s solid k-mers in total, or m > ~8, end in finish()'s
// exactness check and the retry with a 16x budget.
//
// One push, launch by launch: next() yields the steps in order, each with the two running counters as they stand behind it
// (the sketcher's, or their repair twins: a repair pass runs the same staged schedule on counters of its own -- it may be
// the first time any k-mer is admitted).  Nothing is allocated: a push is on the step's hot path.
class PushPlan {
  public:
    // kfmt: kernel format 0 (sequence), 1 (FASTQ, ticket + look-back) or 2 (FASTQ, self-synchronising); the span is
    // [begin, end) behind its aligned base (the tiles are counted from that base); the counters as they stand in front of
    // the push; force_queue: none (< 0), 0 or 1; force_split: 0 (none), 1, 2, 4, 8
    PushPlan(const PushConsts &c, int cu_count, int kfmt, bool repair, uint64_t begin, uint64_t end, uint64_t bytes_pushed,
             uint64_t next_chunk_bytes, int force_queue, uint32_t force_split)
        : c_(c), cu_count_(cu_count), kfmt_(kfmt), repair_(repair), n_(end - begin), ntiles_((uint32_t)span_tiles(end)), bytes_pushed_(bytes_pushed),
          next_chunk_bytes_(next_chunk_bytes), pushed_before_(bytes_pushed), force_queue_(force_queue), force_split_(force_split)
    {
        plan();
    }

    bool next(PushStep &st)
    {
        if (tile_ >= ntiles_) return false;
        // Kernel form of this launch (process_group_regs): candidates are queued when many windows will pass the admission
        // test -- a large sketch, or an early launch whose threshold still stems from little data (T ~ s-th smallest of
        // the k-mers seen so far, ~0.4 per FASTQ byte: above ~3 candidates in 10^4 windows the queue wins); the very first
        // launch, which admits everything, and the long launches of a small sketch finish them where they are found.
        // (nothing pushed yet: T is still at its initial value and admits everything)
        long double expected_rate = bytes_pushed_ ? std::min(1.0L, (long double)c_.s / (0.4L * (long double)bytes_pushed_)) : 1.0L;
        // staged phase of the multiplicity filter: the threshold sits at the byte-count cap until solid hashes take over
        if (cap_) expected_rate = std::max(expected_rate, (long double)cap_ / (long double)c_.hash_max);
        st.queue_candidates = queue_form(kfmt_, c_.s, expected_rate, force_queue_);
        st.tile0 = tile_;
        st.ntiles = take_;
        // The first launch of a fresh sketcher admits every window: each lane hashes AND inserts window after window, on
        // a chunk of at most nslots / 4 bytes -- a few dozen workgroups on an otherwise empty device.  It gets S workgroups
        // per tile (HashArgs::split), the smallest power of two that brings the grid up to the CU count.
        st.split = 1;
        if (kfmt_ != 1 && !repair_ && pushed_before_ == 0 && launch_ == 0 && !cap_ && !st.queue_candidates) { // (inline form: the split kernels are)
            if (force_split_) st.split = force_split_;
            else while (st.split < 8 && (uint64_t)take_ * st.split < (uint64_t)cu_count_) st.split *= 2;
        }
        st.cap_before = launch_ == 0 ? cap_ : 0;
        ++launch_;
        tile_ += take_;
        bytes_pushed_ = pushed_before_ + std::min<uint64_t>(n_, (uint64_t)tile_ * kTileBytes); // real bytes, not whole tiles: callers may push tiny spans
        if (c_.m <= 1 && next_chunk_bytes_ < (1ull << 40)) {
            uint64_t G = c_.nslots / (16ull * c_.s);
            G = std::min<uint64_t>(std::max<uint64_t>(G, kChunkGrowth), 256);
            next_chunk_bytes_ *= G;
        }
        const bool last = tile_ >= ntiles_;
        if (!last) plan();
        st.next_cap = last ? 0 : cap_;
        // the pass behind the last launch also checks the phase chain of the push (a push of one tile has no chain)
        st.verify_chain = last && (kfmt_ == 2 || repair_) && ntiles_ >= 2;
        st.bytes_pushed = bytes_pushed_;
        st.next_chunk_bytes = next_chunk_bytes_;
        return true;
    }

  private:
    void plan() // the launch that starts at tile_: take_ tiles under cap_
    {
        const bool filtered = c_.m > 1;
        take_ = ntiles_ - tile_;
        cap_ = 0;
        if (launch_ != kMaxLaunchesPerPush - 1) { // (the last launch a push may have takes the rest)
            uint64_t chunk_bytes = next_chunk_bytes_;
            if (filtered) {
                // stages are defined on the bytes actually seen (pushes may be of any size): the uncapped first MiB,
                // then never more than x4 (x8 for m <= 3) cumulative growth per launch
                // (x8 for m <= 3, round 3: the byte-count cap admits ~19 s' (1 - 1/g) occurrences per stage whatever the growth g
                // is, and the window of coverages in which s solid hashes lie below the cap -- c / P[Poisson(c) >= m] <= 17:
                // c in 0.8 .. 16 for m = 3, 1.6 .. 16 for m = 4 -- spans a factor 20 resp. 10: no x8 stage can jump over it.
                // Two launches and two passes fewer on a 3 GB input.  Larger m keep x4: 2.5 .. 16 for m = 5.)
                const uint64_t rest_of_prefix = bytes_pushed_ < kUncappedBytes ? kUncappedBytes - bytes_pushed_ : 0;
                chunk_bytes = std::max<uint64_t>(rest_of_prefix, (c_.m <= 3 ? 7 : 3) * bytes_pushed_);
            }
            const uint64_t chunk_tiles = std::max<uint64_t>(1, chunk_bytes / kTileBytes);
            if (chunk_tiles < take_) take_ = (uint32_t)chunk_tiles;
        }
        if (filtered) {
            const uint64_t after = pushed_before_ + std::min<uint64_t>(n_, (uint64_t)(tile_ + take_) * kTileBytes);
            if (after > kUncappedBytes) {
                const long double s_eff = (long double)c_.s + 8.0L * sqrtl((long double)c_.s) + 16.0L;
                const long double cap_frac = 48.0L * s_eff * (long double)c_.admit_scale / (long double)after;
                if (cap_frac < 1.0L) cap_ = std::max<uint64_t>(1, (uint64_t)(cap_frac * (long double)c_.hash_max));
            }
        }
    }

    const PushConsts c_;
    const int cu_count_, kfmt_;
    const bool repair_;
    const uint64_t n_;
    const uint32_t ntiles_;
    uint64_t bytes_pushed_, next_chunk_bytes_;
    const uint64_t pushed_before_;
    const int force_queue_;
    const uint32_t force_split_;
    uint32_t tile_ = 0, take_ = 0;
    uint64_t cap_ = 0;
    int launch_ = 0;
};

} // namespace mhx
