// mhx_sketch.hip -- the sketch tile kernel and what it inserts into.
//
//   sketch_tile_kernel<K,FMT,QUEUE,PROBE,SPLIT>
//       one workgroup per 16 KiB tile of the FASTQ / sequence byte stream: stage -> classify -> (FASTQ) line phase ->
//       candidate k-mer starts -> LDS work list -> canonical k-mer + MurmurHash3_x64_128 -> admission -> table.  The
//       phases are the functions of mhx_tile.h.  FMT 0: sequence stream; FMT 2: FASTQ, every tile finds its line phase
//       by itself (no ticket, no inter-workgroup wait); FMT 1: FASTQ with ticket + decoupled look-back, the repair pass
//       for the tiles FMT 2 had to leave out (lines too long to self-synchronise).
//   DeviceInserter / ScreenProber   what an admitted hash does: claim a slot of the candidate table, or count in the
//       screen table (PROBE)
//   launch_hash   picks the instantiation for (k, format, form); k = 1 .. 32, or MHX_ONLY_K alone in experiment builds
#include "mhx_block.h"
#include "mhx_device.h"
#include "mhx_screen.h"
#include "mhx_tile.h"

#include <type_traits>

namespace mhx {

// ---------------------------------------------------------------------------------------
// candidate table: open addressing, keys claimed with a 64-bit CAS, counts by atomic add.
// Only atomics touch the table inside a launch, so no cross-XCD visibility protocol is
// needed; the next kernel on the stream reads it with plain loads.
// ---------------------------------------------------------------------------------------
struct DeviceInserter {
    unsigned long long *keys;
    uint32_t *cnts;
    uint64_t mask;
    unsigned long long *stats; // this block's replica
    __device__ __forceinline__ void operator()(uint64_t h)
    {
        if (h == kEmptyKey) {
            atomicAdd(&stats[kStatMaxKey], 1ull);
            return;
        }
        uint64_t slot = h & mask;
        for (int probe = 0; probe < 8192; ++probe) {
            const unsigned long long prev = atomicCAS(&keys[slot], (unsigned long long)kEmptyKey, (unsigned long long)h);
            if (prev == kEmptyKey || prev == h) {
                atomicAdd(&cnts[slot], 1u);
                return;
            }
            slot = (slot + 1) & mask;
        }
        atomicOr(&stats[kStatFlags], (unsigned long long)kFlagTableFull);
    }
};

// The same place in the kernel for the containment screen (mhx_screen.h): keys / cnts are a screen table, built before the
// launch and only read here.  An admitted window counts where its hash is a key and changes nothing otherwise: plain
// loads along the probe sequence, one atomic add on a hit.  A type of its own, and with it kernels of their own
// (sketch_tile_kernel<.., PROBE = true>): a run-time switch inside DeviceInserter costs the inline form of the sketch
// kernel four VGPRs (68 -> 72 at k = 21), wherever the switch is kept.
struct ScreenProber {
    unsigned long long *keys;
    uint32_t *cnts;
    uint64_t mask;
    unsigned long long *stats; // this block's replica
    __device__ __forceinline__ void operator()(uint64_t h)
    {
        if (h == kEmptyKey) {
            atomicAdd(&stats[kStatMaxKey], 1ull);
            return;
        }
        const uint64_t at = screen_find(reinterpret_cast<const uint64_t *>(keys), mask, h);
        if (at != kScreenAbsent && !screen_count_stands(atomicAdd(&cnts[at], 1u))) {
            atomicSub(&cnts[at], 1u);
            atomicOr(&stats[kStatFlags], (unsigned long long)kFlagCountWrap);
        }
    }
};

// Not inlined on purpose: the window finished here needs ~40 registers of its own (two strands, eight words each, and
// the hash); inside the kernel body they would be the hash loop's problem.
template <int K, class Ins> __device__ __noinline__ uint32_t finish_candidate(const TileSmem &sm, uint32_t code, uint64_t T, Ins ins)
{
    return process_deferred<K>(sm, code, T, ins);
}

// What the hash loop does with a candidate window in the queue form: it appends (group << 3) | window to the free tail
// of the tile's work list (TileSmem) -- one LDS atomic and one 16-bit store, nothing else: no call, no threshold, no table
// pointers in the hot loop's live set (round 2 finished an overflowing candidate on the spot through a non-inlined call,
// which cost the kernel 32 bytes of scratch per lane for the registers saved around it).  A queue that overflows (more
// than ~1000 candidates in a tile: only while T still admits a large share of all hashes, i.e. the first launches of a
// sketch) is not used at all: the counter says so and the tile then finishes EVERY valid window through the generic
// routine after the hash loop (sketch_tile_kernel), which tests each hash against T itself.
struct CandidateQueue {
    TileSmem &sm;
    uint32_t first, cap; // list[first .. first + cap) is free
    __device__ __forceinline__ void operator()(uint32_t group, int window) const
    {
        const uint32_t slot = atomicAdd(&sm.misc[7], 1u);
        if (slot < cap) sm.list[first + slot] = (uint16_t)((group << 3) | (uint32_t)window);
    }
};
// ... of a line-relative item (process_line_rel_item, mhx_tile.h), which hands over its byte position: the window's
// position is the sum, and that is the number the code above stands for
struct CandidateQueueAt {
    TileSmem &sm;
    uint32_t first, cap;
    __device__ __forceinline__ void operator()(uint32_t pos, int window) const
    {
        const uint32_t slot = atomicAdd(&sm.misc[7], 1u);
        if (slot < cap) sm.list[first + slot] = (uint16_t)(pos + (uint32_t)window);
    }
};

// ---------------------------------------------------------------------------------------
// Decoupled look-back over per-tile newline counts (wave 0 of the block).
// tile_state[t] is ONE naturally aligned 8-byte word {flag:32 | value:32} written by one
// agent-scope store and polled by agent-scope loads: flag 1 = this tile's own count,
// flag 2 = inclusive prefix up to and including this tile.  Tiles are handed out by an
// atomic ticket, so every predecessor of a running tile is itself running or done and
// publishes its own count without waiting on anyone: the wait below always ends.
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ uint64_t ld_state(const uint64_t *p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_state(uint64_t *p, uint64_t v)
{
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ uint32_t lookback_wave(uint64_t *state, uint32_t tile, uint32_t first_tile, uint32_t agg,
                                  unsigned long long *stats)
{
    const int lane = threadIdx.x & 63;
    constexpr uint64_t A = 1ull << 32, P = 2ull << 32;
    if (tile == first_tile) {
        if (lane == 0) st_state(&state[tile], P | agg);
        return 0;
    }
    if (lane == 0) st_state(&state[tile], A | agg);
    uint32_t excl = 0;
    int64_t pos = (int64_t)tile - 1;
    // Every round polls the 4 x 64 nearest unread predecessors with four loads in flight at once:
    // tiles reach this point faster than one L2 round trip per 64 of them, so a 64-wide window
    // per round trip never catches up with the newest published prefix.
    constexpr int kWin = 4;
    bool done = false;
    for (uint32_t spins = 0; !done;) {
        uint64_t w[kWin];
#pragma unroll
        for (int j = 0; j < kWin; ++j) {
            const int64_t idx = pos - lane - 64 * j;
            w[j] = idx >= (int64_t)first_tile ? ld_state(&state[idx]) : P; // before the push: prefix 0
        }
        bool blocked = false;
#pragma unroll
        for (int j = 0; j < kWin; ++j) {
            if (done || blocked) continue;
            const uint32_t f = (uint32_t)(w[j] >> 32);
            const uint64_t notready = __ballot(f == 0);
            const uint64_t isp = __ballot(f == 2);
            uint64_t take = 0; // lanes whose value is added
            if (isp) {
                const int q = __builtin_ctzll(isp);
                const uint64_t below = q ? (~0ull >> (64 - q)) : 0ull;
                if ((notready & below) == 0) {
                    take = below | (1ull << q);
                    done = true;
                }
            } else if (!notready) {
                take = ~0ull;
            }
            if (take) {
                uint32_t v = ((take >> lane) & 1ull) ? (uint32_t)w[j] : 0u;
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
                excl += v;
                if (!done) pos -= 64;
            } else {
                blocked = true;
            }
        }
        if (blocked) {
            if (++spins > (1u << 20)) { // ~a second; never reached in a healthy launch
                if (lane == 0) atomicOr(&stats[kStatFlags], (unsigned long long)kFlagSpinTimeout);
                break;
            }
            __builtin_amdgcn_s_sleep(4);
        }
    }
    if (lane == 0) st_state(&state[tile], P | (uint64_t)(excl + agg));
    return excl;
}

// ---------------------------------------------------------------------------------------
#ifdef MHX_PARSE_LOOPS   // A/B builds: every FASTQ tile parses with the per-newline loops of phase_good
constexpr bool kParseLoops = true;
#else
constexpr bool kParseLoops = false;
#endif
#ifdef MHX_LINE_CHECK_LEN   // A/B builds: the line path counts its long records in the checks (seqline_is_long), as the map path does
constexpr bool kLineSpanRecords = false;
#else
constexpr bool kLineSpanRecords = true;
#endif
#ifndef MHX_MIN_WAVES
#define MHX_MIN_WAVES 7   // 72 VGPRs: seven waves per SIMD, matching the seven workgroups per CU the LDS footprint admits
#endif
template <int K, int FMT, bool QUEUE, bool PROBE, bool SPLIT = false> __global__ __launch_bounds__(kBlock, MHX_MIN_WAVES) void sketch_tile_kernel(const HashArgs a)
{
    __shared__ TileSmem sm;
    constexpr bool FASTQ = (FMT != 0), LOOKBACK = (FMT == 1), SELFSYNC = (FMT == 2);
    const int tid = threadIdx.x;
    // the parsing phases are latency-bound (loads, barriers, look-back): at high priority their few instructions do
    // not queue behind the hash loops of the other resident workgroups, so a wave reaches its own hash loop sooner
    // and more waves per SIMD are in VALU-dense code at any time (-2 % kernel time)
    __builtin_amdgcn_s_setprio(3);

    // split launch (SPLIT: HashArgs::split > 1, a power of two): `split` workgroups per tile, all of which stage and parse
    // it, and each of which then hashes one slice of the work list.  What a tile does once -- counters, phase record,
    // repair word, format flag -- is left to slice 0.  A form of its own, for the inline kernels of formats 0 and 2 only:
    // as a run-time stride in every kernel it cost the queue forms a VGPR (60 -> 61 at k = 21, 67 -> 68 at k = 27).
    static_assert(!SPLIT || (!LOOKBACK && !QUEUE && !PROBE), "split launches: inline sketch kernels of formats 0 and 2");
    const uint32_t split_log2 = SPLIT ? (uint32_t)__builtin_ctz(a.split) : 0u;
    const uint32_t slice = SPLIT ? blockIdx.x & (a.split - 1u) : 0u;
    const uint32_t it0 = slice * kBlock + (uint32_t)tid, it_step = (uint32_t)kBlock << split_log2;
    const bool once = slice == 0; // this workgroup speaks for the tile
    // tile id: in ticket order for FASTQ (look-back needs started-before ordering)
    uint32_t tile;
    if (LOOKBACK) {
        if (tid == 0) sm.misc[2] = a.tile0 + atomicAdd(a.ticket, 1u);
        __syncthreads();
        tile = sm.misc[2];
    } else {
        tile = a.tile0 + (blockIdx.x >> split_log2);
    }
    const uint64_t tile_off = (uint64_t)tile * kTileBytes;
    unsigned long long *stats = reinterpret_cast<unsigned long long *>(a.stats) + (tile % kStatReplicas) * kStatCount;
    // the work list from the line list (phase_line_span / phase_line_items, mhx_tile.h): the forms line_items_form names
    constexpr bool kLineItems = !kParseLoops && line_items_form<K>(FMT, QUEUE);
    // ... as line-relative items (phase_line_rel_items): full groups from the line's first start, the tails behind them
    constexpr bool kLineRel = kLineItems && line_rel_form<K>(FMT, QUEUE);
    if (tid == 0) { sm.misc[3] = 0; sm.misc[4] = 0; sm.misc[5] = 0; sm.misc[7] = 0; }
#ifdef MHX_STAMPS
    uint64_t stamp_prev = clock64();
    int stamp_idx = 0;
#define MHX_STAMP()                                                                                      \
    do {                                                                                                 \
        if (tid == 0) {                                                                                  \
            const uint64_t now_ = clock64();                                                             \
            atomicAdd(&stats[kStatStamp0 + stamp_idx], (unsigned long long)(now_ - stamp_prev));         \
            stamp_prev = now_;                                                                           \
        }                                                                                                \
        ++stamp_idx;                                                                                     \
    } while (0)
#else
#define MHX_STAMP() do { } while (0)
#endif

    phase_stage(sm, tid, a.base, tile_off, a.end);
    __syncthreads();
    MHX_STAMP(); // 0: stage (global loads -> LDS)

    ThreadState st;
    const bool interior = tile_off >= a.begin && tile_off + kTileBytes + kHaloBytes <= a.end; // nothing to mask out
    phase_classify(sm, tid, st, tile_off, a.begin, a.end, interior);

    MHX_STAMP(); // 1: classify
    uint32_t line_base = 0, excl = 0, tile_total = 0;
    bool fast_parse = false;
    // the format look-ahead may only read staged bytes that belong to the span
    const uint64_t span_left = a.end > tile_off ? a.end - tile_off : 0;
    const uint32_t check_limit = span_left < (uint64_t)(kTileBytes + kHaloBytes) ? (uint32_t)span_left : (uint32_t)(kTileBytes + kHaloBytes);
    if (FASTQ) {
        excl = block_scan_excl<kBlock>(st.nlcount, sm.cnt, tile_total); // barrier inside: the newline map is complete
        // good map without a trip per newline (mhx_tile.h): the newline positions are listed now, next to thread 0's
        // phase search; the barrier that follows it puts them in front of phase_good_events.  Workgroup-uniform.
        fast_parse = !kParseLoops && parse_events_fit(tile_total);
        if (fast_parse) phase_events(sm, tid, st, excl);
        // the tile that holds the start of the span begins a record there; every other tile looks at its own first lines
        // ... in the newline list where there is one (mhx_tile.h): four lanes of the first wave test the four triples side by
        // side where that wave has listed six newlines itself (selfsync_triple; the self-synchronising kernels), thread 0
        // takes the first six entries behind a barrier of its own otherwise (phase_selfsync_list) -- and in the map, word by
        // word, on the tiles without a list.  A look-back launch that is no repair pass takes every phase from the chain
        // and never reads what the tile finds: it does not search.  All three choices are workgroup-uniform.
        const bool no_search = tile == a.first_tile || (kSelfsyncList && LOOKBACK && !a.repair);
        const bool listed = kSelfsyncList && fast_parse && !no_search;
        const bool by_lanes = SELFSYNC && listed && selfsync_from_list(fast_parse, false, sm.cnt[0]);
        if (by_lanes) {
            if (tid < 64) {
                const bool pass = tid < (int)kSelfsyncTriples && selfsync_triple(sm, (uint32_t)tid, check_limit);
                const uint32_t phase = selfsync_phase((uint32_t)__ballot(pass));
                if (tid == 0) sm.misc[0] = phase;
            }
        } else if (listed) {
            __syncthreads(); // the list is complete
            if (tid == 0) sm.misc[0] = phase_selfsync_list(sm, st, tile_total, check_limit);
        } else if (tid == 0) {
            sm.misc[0] = no_search ? 0u : phase_selfsync(sm, check_limit);
        }
        __syncthreads();
        const uint32_t self_phase = sm.misc[0];
        if (SELFSYNC) {
            if (self_phase == 4u) { // lines too long to tell: left to the look-back pass, nothing of this tile is counted now
                if (tid == 0 && once) { a.phase_rec[tile - a.first_tile] = 0; atomicOr(a.need_lookback, 1u); }
                return; // (the newline list phase_events has just written goes unused: listing before the phase is known saves a barrier)
            }
            if (tid == 0 && once) a.phase_rec[tile - a.first_tile] = phase_record(self_phase, tile_total);
            line_base = self_phase;
        } else {
            if (a.repair && self_phase != 4u) { // repair pass: this tile was done in the first pass, it only publishes its phase
                if (tid == 0) {
                    st_state(&a.tile_state[tile], (2ull << 32) | (uint64_t)(self_phase + tile_total));
                    a.phase_rec[tile - a.first_tile] = phase_record(self_phase, tile_total);
                }
                return; // (the newline list phase_events has just written goes unused: listing before the phase is known saves a barrier)
            }
            if (tid < 64) {
                const uint32_t lb = lookback_wave(a.tile_state, tile, a.first_tile, tile_total, stats);
                if (tid == 0) sm.misc[0] = lb;
            }
            __syncthreads();
            line_base = sm.misc[0];
            if (a.repair && tid == 0) a.phase_rec[tile - a.first_tile] = phase_record(line_base, tile_total);
        }
    }
    MHX_STAMP(); // 2: newline scan + look-back
    bool bad = false;
    // workgroup-uniform: the tile's sequence lines become its work list as they stand; the lanes of the first wave take one
    // each and read its two ends before the barrier, behind which the list and the start masks go where the events and the
    // newline map were
    bool by_lines = kLineItems && line_items_try(fast_parse, interior, line_base, tile_total);
    uint32_t long_records, items_at = 0;
    LineSpan span{0u, 0u, 0u, 0u, 0u};
    if (kLineItems && by_lines) {
        // the '@' / '+' tests on every lane; the long records from the ends of the lines the first wave reads anyway, one lane
        // per line, once per record whatever becomes of the tile behind the barrier (line_span_long_record, mhx_tile.h)
        long_records = phase_event_checks<!kLineSpanRecords>(sm, tid, line_base, tile_total, check_limit, bad, tile_off, a.end, (uint32_t)K);
        if (tid < (int)kLineItemLines) {
            span = phase_line_span<K>(sm, (uint32_t)tid, line_base, tile_total);
            if (kLineSpanRecords) long_records = span.long_record;
            // the two words the path leaves for the other waves are set here, by this wave, and nowhere else: set at the kernel's
            // entry, in front of the stage loads of every tile, they cost a FASTQ of 10 kb reads 1.3 % (profiles/line_items_ab.txt, 4)
            const bool too_long = __ballot(line_span_too_long(span)) != 0ull; // wave-uniform
            if (tid == 0) { sm.misc[1] = 0u; sm.misc[6] = too_long ? 1u : 0u; }
            items_at = atomicAdd(&sm.misc[1], kLineRel ? line_rel_counts(span) : span.ngroups); // behind lane 0's store in this wave's LDS order; a wave scan (DPP) and one LDS atomic
        }
    } else {
        long_records = fast_parse
            ? phase_good_events(sm, tid, st, line_base, excl, tile_total, check_limit, bad, tile_off, a.end, (uint32_t)K)
            : phase_good<FASTQ>(sm, tid, st, line_base, excl, tile_total, check_limit, bad, tile_off, a.end, (uint32_t)K);
    }
    if (FASTQ && bad && once) atomicOr(&stats[kStatFlags], (unsigned long long)kFlagBadFastq);
    if (FASTQ && long_records) atomicAdd(&sm.misc[5], long_records);
    __syncthreads();
    MHX_STAMP(); // 3: good-base map, or the ends of the sequence lines
    if (kLineItems && by_lines && MHX_UNLIKELY(sm.misc[6] != 0u)) { // a line above the bound: the maps after all, its checks are done and its records counted
        by_lines = false;
        phase_good_events_map(sm, tid, st, line_base, excl, tile_total);
        __syncthreads();
    }

    uint32_t nitems = 0, nfull = 0; // nfull: the full items in front of the tails (line-relative items)
    bool by_rel = false;            // workgroup-uniform: this tile takes the line-relative items (line_rel_choose)
    if (kLineItems && by_lines) {
        if (tid < (int)kLineItemLines) {
            if (span.kmers) atomicAdd(&sm.misc[3], span.kmers);
            if (kLineRel) { // the packed totals: complete since the barrier above
                const uint32_t total = sm.misc[1];
                if (line_rel_choose(total)) phase_line_rel_items(sm, span, items_at, total);
                else phase_line_items(sm, span, line_rel_aligned(items_at));
            } else {
                phase_line_items(sm, span, items_at);
            }
        }
        __syncthreads();
        nitems = sm.misc[1];
        if (kLineRel) { // (nfull: compared on the scalar unit, once a trip)
            const uint32_t total = wave_uniform(nitems);
            by_rel = line_rel_choose(total);
            nfull = line_rel_full(total);
            nitems = by_rel ? line_rel_items(total) : line_rel_aligned(total);
        }
    } else {
        uint32_t items = 0;
        const uint32_t kmers = phase_runs<K>(sm, tid, items);
        if (kmers) atomicAdd(&sm.misc[3], kmers);
        const uint32_t items_before = block_scan_excl<kBlock>(items, sm.cnt + 8, nitems); // barrier inside: sm.valid complete
        phase_compact(sm, tid, items_before);
        __syncthreads();
    }
    MHX_STAMP(); // 4: valid starts + work list
    __builtin_amdgcn_s_setprio(0);

    const uint64_t T = *a.thresh;
    const uint32_t limit = admission_limit(T);
    std::conditional_t<PROBE, ScreenProber, DeviceInserter> ins{reinterpret_cast<unsigned long long *>(a.keys), a.cnts, a.slot_mask, stats};
    const uint32_t qcap = (uint32_t)kGroupsPerTile - nitems; // QUEUE: the work list's unused tail holds the candidate queue
    CandidateQueue queue{sm, nitems, qcap};
    CandidateQueueAt queue_at{sm, nitems, qcap};
    uint32_t ninsert = 0;
    const TailLutPtr lut = hot_tail_table<K>(); // once per workgroup, in front of the loop
    constexpr bool kPairs = pair_words_form<K>(FMT, QUEUE); // windows J and J + 4 share their funnel shifts (PairWords)
    if (kLineRel && by_rel) {
        // a wave's trip is 64 consecutive entries, and a lane in it means lane 0 in it: the trip's first entry, on the scalar
        // unit, tells the trips of tails alone, which stop behind their longest tail, from the hot body
        for (uint32_t it = it0; it < nitems; it += it_step) {
            if (MHX_UNLIKELY(wave_uniform(it) >= nfull)) ninsert += process_line_rel_item<K, QUEUE, kPairs, true>(sm, sm.list[it], T, limit, ins, queue_at, lut);
            else ninsert += process_line_rel_item<K, QUEUE, kPairs, false>(sm, sm.list[it], T, limit, ins, queue_at, lut);
        }
    } else {
        for (uint32_t it = it0; it < nitems; it += it_step) ninsert += process_group<K, QUEUE, kPairs>(sm, sm.list[it], T, limit, ins, queue, lut);
    }
    if (QUEUE) {
        __syncthreads();
        const uint32_t ncand = sm.misc[7];
        if (ncand <= qcap) { // the candidates the loop has queued, one per lane
            for (uint32_t c = tid; c < ncand; c += kBlock) ninsert += finish_candidate<K>(sm, sm.list[nitems + c], T, ins);
        } else { // the queue overflowed (T still admits a large share of all hashes): every valid window, whole hash, exact test
            for (uint32_t it = it0; it < nitems; it += it_step) {
                const uint32_t g = sm.list[it];
                if (kLineRel && by_rel) { // a line-relative item: its mask, and its windows from its byte position on
                    const uint32_t vm = line_rel_vm(sm, g);
                    uint32_t vmask = vm & 0xFFu;
                    while (vmask) {
                        const uint32_t j = (uint32_t)__builtin_ctz(vmask);
                        vmask &= vmask - 1u;
                        ninsert += finish_candidate<K>(sm, (vm >> 8) + j, T, ins);
                    }
                    continue;
                }
                uint32_t vmask = reinterpret_cast<const uint8_t *>(sm.valid)[g];
                while (vmask) {
                    const uint32_t j = (uint32_t)__builtin_ctz(vmask);
                    vmask &= vmask - 1u;
                    ninsert += finish_candidate<K>(sm, (g << 3) | j, T, ins);
                }
            }
        }
    }
    if (ninsert) atomicAdd(&sm.misc[4], ninsert);
    __syncthreads();
    MHX_STAMP(); // 5: work loop
    if (tid == 0) {
        if (once && sm.misc[3]) atomicAdd(&stats[kStatKmers], (unsigned long long)sm.misc[3]);
        if (sm.misc[4]) atomicAdd(&stats[kStatInserts], (unsigned long long)sm.misc[4]); // per slice: every slice adds its own
        if (once && FASTQ && tile_total) atomicAdd(&stats[kStatLines], (unsigned long long)tile_total);
        if (once && FASTQ && sm.misc[5]) atomicAdd(&stats[kStatRecords], (unsigned long long)sm.misc[5]);
    }
}

template <int K> static hipError_t launch_k(int fmt, const HashArgs &a, hipStream_t st)
{
    // a.queue_candidates: large sketches (many windows pass the admission test) finish their candidates after the hash
    // loop, one per lane; small ones where they are found (process_group_regs)
    // a.probe: the kernels of the containment screen (ScreenProber in the place of DeviceInserter)
    if (a.split > 1) { // the split forms: inline, non-probing, formats 0 and 2 (FMT 1 takes its tiles by ticket: one workgroup each)
        if (fmt == 1 || a.queue_candidates || a.probe) return hipErrorInvalidValue;
        if (fmt == 2) hipLaunchKernelGGL((sketch_tile_kernel<K, 2, false, false, true>), dim3(a.ntiles * a.split), dim3(kBlock), 0, st, a);
        else hipLaunchKernelGGL((sketch_tile_kernel<K, 0, false, false, true>), dim3(a.ntiles * a.split), dim3(kBlock), 0, st, a);
        return hipGetLastError();
    }
    const unsigned grid = a.ntiles;
#define MHX_LAUNCH_FORM(FMT_, QUEUE_) do { if (a.probe) hipLaunchKernelGGL((sketch_tile_kernel<K, FMT_, QUEUE_, true>), dim3(grid), dim3(kBlock), 0, st, a); \
                                           else hipLaunchKernelGGL((sketch_tile_kernel<K, FMT_, QUEUE_, false>), dim3(grid), dim3(kBlock), 0, st, a); } while (0)
#define MHX_LAUNCH(FMT_) do { if (a.queue_candidates) MHX_LAUNCH_FORM(FMT_, true); else MHX_LAUNCH_FORM(FMT_, false); } while (0)
    if (fmt == 1) MHX_LAUNCH(1);
    else if (fmt == 2) MHX_LAUNCH(2);
    else MHX_LAUNCH(0);
#undef MHX_LAUNCH
#undef MHX_LAUNCH_FORM
    return hipGetLastError();
}

#ifdef MHX_ONLY_K   // experiment / ISA-study builds: one k-mer size
#define MHX_K_LIST(X) X(MHX_ONLY_K)
#else
#define MHX_K_LIST(X) X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10) X(11) X(12) X(13) X(14) X(15) X(16) \
    X(17) X(18) X(19) X(20) X(21) X(22) X(23) X(24) X(25) X(26) X(27) X(28) X(29) X(30) X(31) X(32)
#endif

bool hash_k_supported(int k) { return k >= 1 && k <= 32; }

hipError_t launch_hash(int k, int fmt, const HashArgs &a, hipStream_t st)
{
    if (a.ntiles == 0) return hipSuccess;
    if (a.split == 0 || (a.split & (a.split - 1)) || a.split > 8 || (uint64_t)a.ntiles * a.split > 0x7FFFFFFFull) return hipErrorInvalidValue;
    switch (k) {
#define X(KK) case KK: return launch_k<KK>(fmt, a, st);
        MHX_K_LIST(X)
#undef X
    default: return hipErrorInvalidValue;
    }
}

} // namespace mhx
