// mhx_engine.cpp -- host side of libmhx: device selection and the sketcher object, which carries
// out the tile launches and threshold tightening that mhx_push_plan.h schedules.  The multi-GPU
// partial export and merge are in mhx_engine_merge.cpp, batched distances in mhx_engine_dist.cpp,
// the containment screen in mhx_engine_screen.cpp; the file-level calls that replace AuriClass's
// `mash sketch` / `mash dist` subprocesses live in mhx_files.cpp and mhx_files_sets.cpp.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>


#include <algorithm>
#include <chrono>
#include <exception>
#include <new>
#include <memory>
#include <string>
#include <vector>

#include "mhx_device.h"
#include "mhx_engine_internal.h"
#include "mhx_internal.h"
#include "mhx_push_plan.h"
#include "mhx_sketcher.h"

namespace mhx {

Engine &g = *new Engine; // never deleted: see Engine

int require_engine()
{
    if (!g.ready) return fail(MHX_E_NO_DEVICE, "mhx: no GPU engine (call mhx_init on a machine with a HIP device; there is no CPU fallback)");
    return MHX_OK;
}

} // namespace mhx

using namespace mhx;

extern "C" const char *mhx_version(void) { return "mhx 0.1.0 (gfx950)"; }
extern "C" void *mhx_stream(void) { return g.stream; }

extern "C" int mhx_init(int device)
{
    clear_error();
    if (g.ready && (device < 0 || device == g.device)) return MHX_OK;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return fail(MHX_E_NO_DEVICE, "mhx: no HIP device visible (MI355X required; there is no CPU fallback)");
    if (device < 0) device = 0;
    if (device >= n) return fail(MHX_E_ARG, "mhx_init: device %d out of range (%d visible)", device, n);
    if (g.ready) mhx_shutdown();
    HIPCHK(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, device));
    g.cu_count = prop.multiProcessorCount;
    HIPCHK(hipStreamCreateWithFlags(g.stream.out(), hipStreamNonBlocking));
    HIPCHK(hipEventCreate(g.ev0.out()));
    HIPCHK(hipEventCreate(g.ev1.out()));
    g.device = device;
    g.ready = true;
    return MHX_OK;
}

extern "C" void mhx_shutdown(void)
{
    if (!g.ready) return;
    hipStreamSynchronize(g.stream);
    if (g.copy_stream) hipStreamSynchronize(g.copy_stream);
    (void)std::exchange(g, Engine()); // the old state goes at the end of this statement, its streams last
}

extern "C" int mhx_device_name(char *buf, size_t cap)
{
    return entry("mhx_device_name", [&]() -> int {
        hipDeviceProp_t p;
        HIPCHK(hipGetDeviceProperties(&p, g.device));
        snprintf(buf, cap, "%s (%s, %d CUs)", p.name, p.gcnArchName, p.multiProcessorCount);
        return MHX_OK;
    });
}

extern "C" int mhx_set_profiling(int on)
{
    g.profiling = on != 0;
    return MHX_OK;
}

// ---- sketcher -------------------------------------------------------------------------
TableArgs mhx::table_args(mhx_sketcher *sk)
{
    TableArgs t;
    t.keys = sk->d_keys; t.cnts = sk->d_cnts; t.nslots = sk->nslots; t.thresh = sk->d_thresh;
    t.hist = sk->d_hist; t.acc = sk->d_acc; t.stats = sk->d_stats; t.done = sk->d_done; t.need_lookback = sk->d_need; t.min_mult = sk->m; t.sketch_size = sk->s;
    t.sample = 1;
    t.next_cap = 0;
    t.verify_rec = nullptr;
    t.verify_ntiles = 0;
    return t;
}

extern "C" int mhx_sketcher_reset(mhx_sketcher *sk)
{
    return entry("mhx_sketcher_reset", [&]() -> int {
        if (!sk) return fail(MHX_E_ARG, "null sketcher");
        if (sk->screen) return fail(MHX_E_ARG, "a screener's prober is reset through mhx_screener_reset");
        // Admission threshold: everything is admitted at first.  For m = 1 the first tighten pass already
        // finds s entries; for m > 1 push_device keeps the table safe until s solid hashes exist.
        sk->t_init = sk->hash_max;
        // one launch: table vacated, histogram / accumulators / counters / tickets cleared, T = t_init
        HIPCHK(launch_reset(table_args(sk), sk->t_init, sk->d_tickets, kTicketWords, sk->d_out_n, g.stream));
        sk->tickets_used = 0;
        sk->table_dirty = true;
        sk->merged = false;
        sk->export_valid = false;
        sk->unsettled.clear();
        sk->last_T = sk->hash_max;
        sk->bounded = false;
        sk->established = false;
        sk->occupied = 0;
        sk->solid = 0;
        const uint64_t c0 = first_chunk_bytes(sk->s, sk->m, sk->nslots);
        sk->next_chunk_bytes = c0;
        sk->bytes_pushed = 0;
        sk->repair_next_chunk_bytes = c0;
        sk->repair_bytes = 0;
        sk->hash_ms = 0.0;
        sk->launches = 0;
        return MHX_OK;
    });
}

// (no prologue of its own: its callers are entry points that have checked the engine)
int create_sketcher(int k, uint32_t s, uint32_t min_mult, uint64_t expected_bytes, uint64_t table_scale, mhx_sketcher **out)
{
    if (!out) return fail(MHX_E_ARG, "null out pointer");
    if (!hash_k_supported(k)) return fail(MHX_E_ARG, "k-mer size %d not supported (1..32)", k);
    if (s == 0) return fail(MHX_E_ARG, "sketch size must be positive");
    std::unique_ptr<mhx_sketcher> sk(new mhx_sketcher());
    sk->k = k; sk->s = s; sk->m = min_mult ? min_mult : 1;
    sk->hash32 = k <= 16;
    sk->hash_max = sk->hash32 ? 0xFFFFFFFFull : ~0ull;
    sk->expected_bytes = expected_bytes;
    sk->admit_scale = table_scale ? table_scale : 1;
    // table: >= 2^21 slots, >= 256 slots per sketch entry (worst-case admissions of the
    // occurrence bound at load 1; real inputs repeat their k-mers and stay far below)
    // (round 3: at least 2^21 slots instead of 2^22 -- the first chunk and every later one are sized as fractions of the
    // table, so the load bounds are the same, and a table half the size is reset, histogrammed and extracted in half the
    // time: +1.4 % on the headline configuration.  128 slots per entry would buy AuriClass's defaults another 0.5 % but
    // puts the worst case (every k-mer distinct) at 60 % load; 64: slower, the probe sequences get long.)
    static const uint64_t slots_per_entry = getenv("MHX_SLOTS_PER_ENTRY") ? (uint64_t)atol(getenv("MHX_SLOTS_PER_ENTRY")) : 256;
    static const int min_log2 = getenv("MHX_TABLE_MIN_LOG2") ? atoi(getenv("MHX_TABLE_MIN_LOG2")) : 21; // experiment knobs
    uint64_t want = (uint64_t)s * slots_per_entry;
    if (want < (1ull << min_log2)) want = 1ull << min_log2;
    if (expected_bytes && expected_bytes * 4 < want && expected_bytes * 4 >= (1ull << 16)) want = expected_bytes * 4;
    if (expected_bytes && expected_bytes * 4 < (1ull << 16)) want = 1ull << 16;
    want *= table_scale;
    if (want > (1ull << 30)) want = 1ull << 30; // 12.9 GB of table at most
    sk->nslots = next_pow2(want);
    const size_t out_cap = s * 2 + 65536;
    hipError_t e = hipSuccess;
    auto A = [&](auto &arr, size_t n) { if (e == hipSuccess) e = arr.grow(n); };
    A(sk->d_keys, sk->nslots);
    A(sk->d_cnts, sk->nslots);
    A(sk->d_thresh, 1);
    A(sk->d_hist, kHistBins);
    A(sk->d_acc, kAccReplicas * 8);
    A(sk->d_stats, kStatReplicas * kStatCount);
    A(sk->d_tickets, kTicketWords);
    A(sk->d_done, 1);
    A(sk->d_need, 1);
    A(sk->d_out_keys, out_cap);
    A(sk->d_out_cnts, out_cap);
    A(sk->d_out_n, 1);
    A(sk->d_exp_hdr, 8);
    if (e == hipSuccess) e = hipMemset(sk->d_exp_hdr, 0, 8 * sizeof(uint64_t)); // zero between two exports (the kernel clears them)
    A(sk->h_exp_hdr, 8);
    sk->fin_cap = (s + 16u * (uint32_t)sqrt((double)s) + 4096u + 1u) & ~1u; // what a sampled threshold leaves, with room (finish())
    const size_t fin_words = 4 + (size_t)sk->fin_cap + sk->fin_cap / 2;
    A(sk->d_fin, fin_words);
    if (e == hipSuccess) e = hipMemset(sk->d_fin, 0, 4 * sizeof(uint64_t)); // the header words are zero between two finish() calls
    if (s >= kDeviceOrderMinSketch) { // below that the host's bucket sort costs less than three more launches
        sk->order_log2 = 12;
        while ((1u << sk->order_log2) < sk->fin_cap && sk->order_log2 < 20) ++sk->order_log2;
        A(sk->d_fin_ordered, fin_words);
        A(sk->d_order_buckets, (size_t)1 << sk->order_log2);
        A(sk->d_order_starts, ((size_t)1 << sk->order_log2) + 4);
        A(sk->d_order_groups, 1024);
        if (e == hipSuccess) e = hipMemset(sk->d_order_starts, 0, (((size_t)1 << sk->order_log2) + 4) * sizeof(uint32_t)); // [nbuckets] stays zero
        if (e == hipSuccess) e = hipMemset(sk->d_order_buckets, 0, ((size_t)1 << sk->order_log2) * sizeof(uint32_t)); // every finish() leaves them zero again
    }
    A(sk->h_fin, fin_words);
    if (e != hipSuccess) return fail(MHX_E_HIP, "hipMalloc failed while creating the sketcher: %s", hipGetErrorString(e));
    const int rc = mhx_sketcher_reset(sk.get()); // (the entry point: it leaves the error text cleared)
    if (rc) return rc;
    *out = sk.release();
    return MHX_OK;
}

extern "C" int mhx_sketcher_create(int k, uint32_t s, uint32_t min_mult, uint64_t expected_bytes, mhx_sketcher **out)
{
    return entry("mhx_sketcher_create", [&] { return create_sketcher(k, s, min_mult, expected_bytes, 1, out); });
}

extern "C" int mhx_sketcher_create_scaled(int k, uint32_t s, uint32_t min_mult, uint64_t expected_bytes, uint32_t budget_scale, mhx_sketcher **out)
{
    return entry("mhx_sketcher_create_scaled", [&] { return create_sketcher(k, s, min_mult, expected_bytes, budget_scale ? budget_scale : 1, out); });
}

extern "C" void mhx_sketcher_destroy(mhx_sketcher *sk)
{
    if (g.ready) hipStreamSynchronize(g.stream);
    delete sk;
}

static int read_threshold(mhx_sketcher *sk, uint64_t *T)
{ // after a tighten pass: the threshold and the table occupancy that pass measured
    static_assert(kStatSolid == kStatOccupied + 1, "occupied and solid are read with one copy");
    uint64_t occ_solid[2] = {0, 0};
    HIPCHK(hipMemcpyAsync(T, sk->d_thresh, sizeof(uint64_t), hipMemcpyDeviceToHost, g.stream));
    HIPCHK(hipMemcpyAsync(occ_solid, sk->d_stats + kStatOccupied, 2 * sizeof(uint64_t), hipMemcpyDeviceToHost, g.stream));
    HIPCHK(hipStreamSynchronize(g.stream));
    sk->last_T = *T;
    sk->occupied = occ_solid[0];
    sk->solid = occ_solid[1];
    return MHX_OK;
}

// FASTQ runs in two kernel forms (mhx_sketch.hip): kernel format 2, every tile finds its line phase by itself -- no
// ticket, no wait between workgroups --, and format 1, ticket + decoupled look-back.  A push goes through format 2; tiles
// whose lines are too long to self-synchronise (reads beyond ~2.7 kb) leave themselves out and raise a word that
// settle() reads at the next synchronisation point; the repair pass then runs format 1 over the same span with only
// those tiles doing work.  (MHX_NO_SELFSYNC=1: format 1 for everything, as in round 1.)
static int push_span(mhx_sketcher *sk, const void *d_bytes, uint64_t n, int kfmt, bool repair);
static int check_fastq_span(mhx_sketcher *sk, const void *d_bytes, uint64_t n);

static int repair_unsettled(mhx_sketcher *sk)
{
    std::vector<mhx_sketcher::Span> spans;
    spans.swap(sk->unsettled);
    HIPCHK(hipMemsetAsync(sk->d_need, 0, sizeof(uint32_t), g.stream));
    for (const auto &sp : spans) {
        const int rc = push_span(sk, sp.ptr, sp.n, 1, true);
        if (rc) return rc;
    }
    return MHX_OK;
}

// at a synchronisation point that is not finish(): is a repair pass due for the pushes since the last one?
int mhx::settle(mhx_sketcher *sk)
{
    if (sk->follower) {
        const int rc = settle(sk->follower);
        if (rc) return rc;
    }
    if (sk->unsettled.empty()) return MHX_OK;
    uint32_t *need = reinterpret_cast<uint32_t *>((uint64_t *)sk->h_fin); // pinned landing word
    HIPCHK(hipMemcpyAsync(need, sk->d_need, sizeof(uint32_t), hipMemcpyDeviceToHost, g.stream));
    HIPCHK(hipStreamSynchronize(g.stream));
    if (*need) {
        const int rc = repair_unsettled(sk);
        if (rc) return rc;
        HIPCHK(hipStreamSynchronize(g.stream));
    }
    sk->unsettled.clear();
    return MHX_OK;
}

int sketcher_release_push(mhx_sketcher *sk, const void *d_bytes, hipStream_t side, uint32_t *word)
{
    if (!sk) return MHX_OK;
    if (sk->follower) {
        const int rc = sketcher_release_push(sk->follower, d_bytes, side, word);
        if (rc) return rc;
    }
    size_t at = sk->unsettled.size();
    for (size_t i = 0; i < sk->unsettled.size(); ++i)
        if (sk->unsettled[i].ptr == d_bytes) { at = i; break; }
    if (at == sk->unsettled.size()) return MHX_OK; // settled already (an earlier repair pass took everything there was)
    HIPCHK(hipMemcpyAsync(word, sk->d_need, sizeof(uint32_t), hipMemcpyDeviceToHost, side));
    HIPCHK(hipStreamSynchronize(side));
    if (*word == 0) {
        sk->unsettled.erase(sk->unsettled.begin() + (long)at);
        return MHX_OK;
    }
    int rc = repair_unsettled(sk); // reads every unsettled span again: all of them are still in place
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(g.stream));
    return MHX_OK;
}

extern "C" int mhx_sketcher_push_device(mhx_sketcher *sk, const void *d_bytes, uint64_t n, int fmt)
{
    return entry("mhx_sketcher_push_device", [&]() -> int {
        if (!sk || (!d_bytes && n)) return fail(MHX_E_ARG, "null argument");
        if (fmt != MHX_FMT_SEQ && fmt != MHX_FMT_FASTQ4) return fail(MHX_E_ARG, "unknown stream format %d", fmt);
        if (sk->merged) return fail(MHX_E_ARG, "this sketcher holds a merged (multi-shard) table: mhx_sketcher_reset() before the next push");
        if (n == 0) return MHX_OK;
        sk->export_valid = false;
        if (sk->follower) { // the same span for the prober that rides along (its own launch over the same resident bytes)
            const int rc = mhx_sketcher_push_device(sk->follower, d_bytes, n, fmt);
            if (rc) return rc;
        }
        if (fmt == MHX_FMT_SEQ) return push_span(sk, d_bytes, n, 0, false);
        if (sk->verify_fastq) {
            const int rc = check_fastq_span(sk, d_bytes, n);
            if (rc) return rc;
        }
        static const bool no_selfsync = getenv("MHX_NO_SELFSYNC") != nullptr;
        if (no_selfsync) return push_span(sk, d_bytes, n, 1, false);
        if (sk->unsettled.size() >= 4096) { // thousands of small pushes without a synchronisation point: settle what there is
            const int rc = settle(sk);
            if (rc) return rc;
        }
        const int rc = push_span(sk, d_bytes, n, 2, false);
        if (!rc) sk->unsettled.push_back({d_bytes, n});
        return rc;
    });
}

void sketcher_verify_fastq(mhx_sketcher *sk, bool on)
{
    if (sk) sk->verify_fastq = on;
}

// the record check of a FASTQ4 push (mhx_fqcheck.h); its verdict lands in the flags finish() reads
static int check_fastq_span(mhx_sketcher *sk, const void *d_bytes, uint64_t n)
{
    const uintptr_t p = (uintptr_t)d_bytes;
    const uintptr_t base = p & ~(uintptr_t)15;
    const uint64_t begin = p - base, end = begin + n;
    // one workspace for every sketcher (all of them run on the engine stream); earlier checks may still use the old one
    HIPCHK(g.fqcheck_ws.grow(fastq_check_scratch_bytes(begin, end), g.stream));
    HIPCHK(launch_fastq_check((const uint8_t *)base, begin, end, g.fqcheck_ws, sk->d_stats, g.stream));
    return MHX_OK;
}

static int push_span(mhx_sketcher *sk, const void *d_bytes, uint64_t n, int kfmt, bool repair)
{
    const uintptr_t p = (uintptr_t)d_bytes;
    const uintptr_t base = p & ~(uintptr_t)15;
    HashArgs a;
    a.base = (const uint8_t *)base;
    a.begin = p - base;
    a.end = a.begin + n;
    a.first_tile = 0;
    a.hash32 = sk->hash32 ? 1 : 0;
    a.thresh = sk->d_thresh;
    a.keys = sk->d_keys; a.cnts = sk->d_cnts; a.slot_mask = sk->nslots - 1; a.stats = sk->d_stats;
    a.need_lookback = sk->d_need;
    a.repair = repair ? 1u : 0u;
    a.probe = sk->screen ? 1u : 0u;
    static const char *force_queue_env = getenv("MHX_QUEUE_CANDIDATES"); // "0" / "1": diagnostic override
    const int force_queue = force_queue_env ? (int)(force_queue_env[0] == '1') : -1;
    // MHX_FIRST_SPLIT=1|2|4|8: diagnostic override of the first launch's split (read per push: the tests change it between sketches)
    const char *split_env = getenv("MHX_FIRST_SPLIT");
    const long split_val = split_env ? atol(split_env) : 0;
    const uint32_t force_split = (uint32_t)(split_val == 1 || split_val == 2 || split_val == 4 || split_val == 8 ? split_val : 0);
    const uint64_t ntiles64 = span_tiles(a.end);
    if (ntiles64 > 0x7FFFFFFFull) return fail(MHX_E_ARG, "span too large for one push (%llu bytes)", (unsigned long long)n);
    const uint32_t ntiles = (uint32_t)ntiles64;
    if (kfmt == 1) {
        HIPCHK(sk->d_tile_state.grow(ntiles, g.stream));
        HIPCHK(hipMemsetAsync(sk->d_tile_state, 0, (size_t)ntiles * sizeof(uint64_t), g.stream));
        if (sk->tickets_used + kMaxLaunchesPerPush > kTicketWords) { // every launch takes a fresh, still zero word
            HIPCHK(hipMemsetAsync(sk->d_tickets, 0, kTicketWords * sizeof(uint32_t), g.stream));
            sk->tickets_used = 0;
        }
    }
    a.tile_state = sk->d_tile_state;
    if (kfmt == 2 || repair) HIPCHK(sk->d_phase_rec.grow(ntiles, g.stream)); // every tile of the span writes its record: nothing to clear
    a.phase_rec = sk->d_phase_rec;
    auto timed_launch = [&]() -> int {
        a.ticket = sk->d_tickets + sk->tickets_used++;
        if (g.profiling) HIPCHK(hipEventRecord(g.ev0, g.stream));
        HIPCHK(launch_hash(sk->k, kfmt, a, g.stream));
        if (g.profiling) {
            HIPCHK(hipEventRecord(g.ev1, g.stream));
            HIPCHK(hipEventSynchronize(g.ev1));
            float ms = 0.f;
            HIPCHK(hipEventElapsedTime(&ms, g.ev0, g.ev1));
            sk->hash_ms += ms;
        }
        ++sk->launches;
        return MHX_OK;
    };
    if (sk->screen) { // the screen table never grows and T_screen never moves: one launch, nothing behind it
        a.split = 1;
        a.queue_candidates = queue_form(kfmt, sk->s, (long double)sk->screen_T / (long double)sk->hash_max, force_queue);
        a.tile0 = 0;
        a.ntiles = ntiles;
        const int rc = timed_launch();
        if (rc) return rc;
        if (!repair) sk->bytes_pushed += n;
        if (kfmt == 2 || repair) HIPCHK(launch_phase_verify(sk->d_phase_rec, ntiles, sk->d_stats, g.stream));
        return MHX_OK;
    }
    TableArgs ta = table_args(sk);
    if (sk->nslots >= (1ull << 23) && !getenv("MHX_EXACT_TIGHTEN")) ta.sample = 8; // big tables: sampled passes between chunks (finish() counts exactly)
    // The schedule (mhx_push_plan.h), launch by launch; a repair pass runs it on counters of its own.
    uint64_t &bytes_pushed = repair ? sk->repair_bytes : sk->bytes_pushed;
    uint64_t &next_chunk_bytes = repair ? sk->repair_next_chunk_bytes : sk->next_chunk_bytes;
    PushPlan plan({sk->s, sk->m, sk->nslots, sk->hash_max, sk->admit_scale}, g.cu_count, kfmt, repair, a.begin, a.end, bytes_pushed, next_chunk_bytes,
                  force_queue, force_split);
    bool verified = false; // the FASTQ phase chain of this push has been checked by its last tighten pass
    for (PushStep st; plan.next(st);) {
        if (st.cap_before) HIPCHK(launch_cap_threshold(sk->d_thresh, st.cap_before, sk->d_stats, g.stream)); // first launch of a push: a launch of its own
        a.tile0 = st.tile0;
        a.ntiles = st.ntiles;
        a.split = st.split;
        a.queue_candidates = st.queue_candidates;
        const int lrc = timed_launch();
        if (lrc) return lrc;
        sk->table_dirty = true;
        sk->table_sampled = false;
        bytes_pushed = st.bytes_pushed; // (only now: a launch that failed has pushed nothing)
        next_chunk_bytes = st.next_chunk_bytes;
        // tighten T from what has been seen (also after the last launch of a push: the next push starts from it).
        // Sampled passes (big tables) leave the table marked dirty (an exact pass has not seen it) but sampled: see finish().
        // (Tried in round 3: the passes between two launches on a side stream, beside the next launch.  Exactness survives
        // -- any earlier T is a valid bound -- but capacity does not: the next launch's first workgroups then run with the
        // threshold of TWO chunks ago, which for the second launch is "admit everything" and overflows the table, and
        // with a multiplicity filter the cap in front of the next launch is decided before the pass can report solid
        // hashes.  What remains safe saves < 1 % of a step; the passes stay in stream order.)
        ta.next_cap = st.next_cap;
        if (st.verify_chain) {
            ta.verify_rec = sk->d_phase_rec;
            ta.verify_ntiles = ntiles;
            verified = true;
        }
        HIPCHK(launch_tighten(ta, (uint32_t)g.cu_count, g.stream));
        if (ta.sample == 1) sk->table_dirty = false;
        else sk->table_sampled = true;
    }
    if ((kfmt == 2 || repair) && !verified) HIPCHK(launch_phase_verify(sk->d_phase_rec, ntiles, sk->d_stats, g.stream));
    return MHX_OK;
}

extern "C" int mhx_sketcher_push_host(mhx_sketcher *sk, const void *h_bytes, uint64_t n, int fmt)
{
    return entry("mhx_sketcher_push_host", [&]() -> int {
        if (!sk || (!h_bytes && n)) return fail(MHX_E_ARG, "null argument");
        if (n == 0) return MHX_OK;
        // the staging buffer is reused: earlier pushes that may still read it (or need it for a repair pass) come first
        int rc = settle(sk);
        if (rc) return rc;
        HIPCHK(hipStreamSynchronize(g.stream));
        if (sk->d_stage.cap() < n + 64) HIPCHK(sk->d_stage.grow((size_t)((n + 64 + (1u << 20) - 1) & ~(uint64_t)((1u << 20) - 1))));
        HIPCHK(hipMemcpyAsync(sk->d_stage, h_bytes, n, hipMemcpyHostToDevice, g.stream));
        return mhx_sketcher_push_device(sk, sk->d_stage, n, fmt);
    });
}

extern "C" int mhx_sketcher_sync(mhx_sketcher *sk)
{
    return entry("mhx_sketcher_sync", [&]() -> int {
        if (sk) {
            const int rc = settle(sk); // a repair pass, if one is due, runs while the pushed buffers are still the caller's to keep
            if (rc) return rc;
        }
        HIPCHK(hipStreamSynchronize(g.stream));
        return MHX_OK;
    });
}

int mhx::fetch_stats(mhx_sketcher *sk, uint64_t *sum)
{
    std::vector<uint64_t> h(kStatReplicas * kStatCount);
    HIPCHK(hipMemcpyAsync(h.data(), sk->d_stats, h.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, g.stream));
    HIPCHK(hipStreamSynchronize(g.stream));
    for (int i = 0; i < kStatCount; ++i) sum[i] = 0;
    for (int r = 0; r < kStatReplicas; ++r) {
        sum[kStatKmers] += h[r * kStatCount + kStatKmers];
        sum[kStatInserts] += h[r * kStatCount + kStatInserts];
        sum[kStatLines] += h[r * kStatCount + kStatLines];
        sum[kStatRecords] += h[r * kStatCount + kStatRecords];
        sum[kStatMaxKey] += h[r * kStatCount + kStatMaxKey];
        sum[kStatFlags] |= h[r * kStatCount + kStatFlags];
    }
    sum[kStatOccupied] = h[kStatOccupied];
    sum[kStatSolid] = h[kStatSolid];
    return MHX_OK;
}

extern "C" int mhx_sketcher_stats(mhx_sketcher *sk, uint64_t *stats8)
{
    return entry("mhx_sketcher_stats", [&]() -> int {
        if (!sk || !stats8) return fail(MHX_E_ARG, "null argument");
        int rc = settle(sk);
        if (rc) return rc;
        uint64_t s[kStatCount];
        rc = fetch_stats(sk, s);
        if (rc) return rc;
        stats8[0] = s[kStatKmers];
        stats8[1] = s[kStatInserts];
        stats8[2] = s[kStatLines];
        stats8[3] = s[kStatFlags];
        stats8[4] = s[kStatOccupied];
        double ms = sk->hash_ms;
        memcpy(&stats8[5], &ms, sizeof(double));
        stats8[6] = sk->launches;
        stats8[7] = sk->last_T;
        return MHX_OK;
    });
}

extern "C" int mhx_sketcher_record_count(mhx_sketcher *sk, uint64_t *records)
{
    return entry("mhx_sketcher_record_count", [&]() -> int {
        if (!sk || !records) return fail(MHX_E_ARG, "null argument");
        int rc = settle(sk);
        if (rc) return rc;
        uint64_t s[kStatCount];
        rc = fetch_stats(sk, s);
        if (rc) return rc;
        *records = s[kStatRecords];
        return MHX_OK;
    });
}

// diagnostic: raw per-phase cycle sums of a -DMHX_STAMPS build (zeros otherwise)
extern "C" int mhx_sketcher_debug_stamps(mhx_sketcher *sk, uint64_t *out8)
{
    return entry("mhx_sketcher_debug_stamps", [&]() -> int {
        if (!sk || !out8) return fail(MHX_E_ARG, "null argument");
        std::vector<uint64_t> h(kStatReplicas * kStatCount);
        HIPCHK(hipMemcpyAsync(h.data(), sk->d_stats, h.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, g.stream));
        HIPCHK(hipStreamSynchronize(g.stream));
        for (int i = 0; i < 8; ++i) {
            out8[i] = 0;
            for (int r = 0; r < kStatReplicas; ++r) out8[i] += h[r * kStatCount + kStatStamp0 + i];
        }
        return MHX_OK;
    });
}

extern "C" int mhx_sketcher_threshold(mhx_sketcher *sk, uint64_t *threshold)
{
    return entry("mhx_sketcher_threshold", [&]() -> int {
        if (!sk || !threshold) return fail(MHX_E_ARG, "null argument");
        int rc = settle(sk);
        if (rc) return rc;
        HIPCHK(launch_tighten(table_args(sk), (uint32_t)g.cu_count, g.stream));
        return read_threshold(sk, threshold);
    });
}

int mhx::check_flags(uint64_t flags)
{
    if (flags & kFlagSpinTimeout) return fail(MHX_E_INTERNAL, "device look-back timed out");
    if (flags & kFlagTableFull) return fail(MHX_E_CAPACITY, "device candidate table overflowed; recreate the sketcher with a larger expected_bytes");
    if (flags & kFlagBadFastq) return fail(MHX_E_FORMAT, "input is not strict 4-line FASTQ (use the record parser path)");
    return MHX_OK;
}

// entries (key <= limit, count >= min_count) -> host vectors, unsorted
static int extract(mhx_sketcher *sk, uint64_t limit, uint32_t min_count, std::vector<uint64_t> &keys, std::vector<uint32_t> &cnts)
{
    for (int attempt = 0; attempt < 2; ++attempt) {
        HIPCHK(hipMemsetAsync(sk->d_out_n, 0, sizeof(uint32_t), g.stream));
        HIPCHK(launch_extract(table_args(sk), limit, min_count, sk->d_out_keys, sk->d_out_cnts, sk->out_cap(), sk->d_out_n, nullptr, nullptr, nullptr, nullptr, g.stream));
        uint32_t n = 0;
        HIPCHK(hipMemcpyAsync(&n, sk->d_out_n, sizeof(uint32_t), hipMemcpyDeviceToHost, g.stream));
        HIPCHK(hipStreamSynchronize(g.stream));
        if (n > sk->out_cap()) { // grow once and repeat
            HIPCHK(sk->d_out_keys.grow(n + 1024));
            HIPCHK(sk->d_out_cnts.grow(n + 1024));
            continue;
        }
        keys.resize(n);
        cnts.resize(n);
        if (n) {
            HIPCHK(hipMemcpyAsync(keys.data(), sk->d_out_keys, (size_t)n * sizeof(uint64_t), hipMemcpyDeviceToHost, g.stream));
            HIPCHK(hipMemcpyAsync(cnts.data(), sk->d_out_cnts, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, g.stream));
            HIPCHK(hipStreamSynchronize(g.stream));
        }
        return MHX_OK;
    }
    return fail(MHX_E_INTERNAL, "extract: output kept growing");
}

static void insertion_pass(uint64_t *k2, uint32_t *c2, size_t n)
{ // O(n + inversions): what is left to do after a scatter by leading bits
    for (size_t i = 1; i < n; ++i) {
        const uint64_t k = k2[i];
        if (k2[i - 1] <= k) continue;
        const uint32_t c = c2[i];
        size_t j = i;
        while (j > 0 && k2[j - 1] > k) { k2[j] = k2[j - 1]; c2[j] = c2[j - 1]; --j; }
        k2[j] = k;
        c2[j] = c;
    }
}

static void sort_pairs(const uint64_t *keys, const uint32_t *cnts, size_t n, SortScratch &sc)
{ // The extracted hashes are (close to) uniform below the threshold: one scatter into ~n..2n buckets by their leading
  // bits (a shift, no division), then an insertion sort over the almost-sorted result (O(n) expected; any input still
  // ends up sorted).  Result in sc.keys / sc.cnts; the scratch vectors live with the sketcher (no page faults per call).
    sc.keys.resize(n);
    sc.cnts.resize(n);
    if (n == 0) return;
    uint64_t hi = 0;
    for (size_t i = 0; i < n; ++i) hi = keys[i] > hi ? keys[i] : hi;
    int shift = 0;
    while ((hi >> shift) >= 2 * n) ++shift;
    const size_t nb = (size_t)(hi >> shift) + 1;
    sc.start.assign(nb + 1, 0);
    uint32_t *start = sc.start.data();
    for (size_t i = 0; i < n; ++i) ++start[(size_t)(keys[i] >> shift) + 1];
    for (size_t b = 0; b < nb; ++b) start[b + 1] += start[b];
    uint64_t *k2 = sc.keys.data();
    uint32_t *c2 = sc.cnts.data();
    for (size_t i = 0; i < n; ++i) {
        const size_t d = start[(size_t)(keys[i] >> shift)]++;
        k2[d] = keys[i];
        c2[d] = cnts[i];
    }
    insertion_pass(k2, c2, n);
}

void sketcher_set_follower(mhx_sketcher *sk, mhx_sketcher *follower)
{
    if (sk) sk->follower = follower;
}

extern "C" int mhx_sketcher_finish(mhx_sketcher *sk, uint64_t *hashes, uint32_t *counts, uint32_t *n_out)
{
    return entry("mhx_sketcher_finish", [&]() -> int {
        int rc = MHX_OK;
        if (!sk || !hashes || !n_out) return fail(MHX_E_ARG, "null argument");
        if (sk->screen) return fail(MHX_E_ARG, "a screener's prober has no sketch");
        if (sk->follower) { // its spans are the ones pushed here: settled while they are still in place
            rc = settle(sk->follower);
            if (rc) return rc;
        }
        // One batch on the stream, one copy, one synchronisation: final (exact) tighten unless the last pass already was
        // one, extract with the threshold read on the device into the result block, the block to its pinned mirror.
        const uint32_t cap = sk->fin_cap;
        uint64_t *d = sk->d_fin;
        const size_t fin_bytes = (4 + (size_t)cap + cap / 2) * sizeof(uint64_t);
        static const bool dbg = getenv("MHX_FINISH_DEBUG") != nullptr; // stderr: where finish() spends its time
        const auto t_begin = std::chrono::steady_clock::now();
        bool want_exact = false;
      again:
        // big tables: the sampled pass behind the last launch left T at about the (s + 8 sqrt(s))-th solid hash, the block holds
        // twice that, and the host keeps the first s -- a second pass over the table only if that turns out not to be so
        if (sk->table_dirty && (want_exact || !sk->table_sampled)) {
            HIPCHK(launch_tighten(table_args(sk), (uint32_t)g.cu_count, g.stream));
            sk->table_dirty = false;
            sk->table_sampled = false;
        }
        const bool ordered = sk->d_fin_ordered != nullptr;
        if (ordered) { // large sketches: the kernels put the block in hash order and store it into the pinned block themselves
            HIPCHK(hipMemsetAsync(d, 0, 4 * sizeof(uint64_t), g.stream));
            HIPCHK(launch_extract(table_args(sk), 0, sk->m, d + 4, (uint32_t *)(d + 4 + cap), cap, (uint32_t *)d, d + 2, sk->d_thresh, d + 1, d + 3, g.stream,
                                  sk->d_order_buckets, sk->order_log2));
            HIPCHK(launch_order_block(d, cap, sk->order_log2, sk->d_order_buckets, sk->d_order_starts, sk->d_order_groups, sk->d_fin_ordered, sk->h_fin, g.stream));
        } else { // one kernel, nothing else: the entries go straight into the pinned block, the workgroup that finishes last
                 // adds the header words (kept on the device while they are being accumulated) and clears them for the next call
            HIPCHK(launch_extract(table_args(sk), 0, sk->m, sk->h_fin + 4, (uint32_t *)(sk->h_fin + 4 + cap), cap, (uint32_t *)d, d + 2, sk->d_thresh, d + 1, d + 3,
                                  g.stream, nullptr, 0, d, sk->h_fin, sk->d_done));
        }
        HIPCHK(hipStreamSynchronize(g.stream));
        const auto t_device = std::chrono::steady_clock::now();
        const uint64_t *h = sk->h_fin;
        const uint32_t n = (uint32_t)h[0];
        const uint64_t T = h[1], flags = h[2], maxkey = h[3];
        if ((flags & kFlagNeedLookback) && !sk->unsettled.empty()) { // FASTQ tiles left out by the self-synchronising pass
            rc = repair_unsettled(sk);
            if (rc) return rc;
            goto again;
        }
        sk->unsettled.clear();
        if (n > cap && sk->table_dirty && !want_exact) { // the sampled threshold was not the expected one: count exactly
            want_exact = true;
            goto again;
        }
        sk->last_T = T;
        sk->bounded = (flags & kFlagStateBounded) != 0;
        sk->established = (flags & kFlagStateEstablished) != 0;
        rc = check_flags(flags);
        if (rc) return rc;
        std::vector<uint64_t> keys;
        std::vector<uint32_t> cnts;
        const uint64_t *src_keys = h + 4; // the common case: sorted straight out of the pinned block
        const uint32_t *src_cnts = reinterpret_cast<const uint32_t *>(h + 4 + cap);
        size_t n_src = n;
        const bool extra = has_max_key_entry(T, maxkey, sk->m); // the one hash value the table cannot hold
        if (n > cap || extra) {
            if (n > cap) { // more entries below T than the result block holds: the general path
                rc = extract(sk, T, sk->m, keys, cnts);
                if (rc) return rc;
            } else {
                keys.assign(src_keys, src_keys + n);
                cnts.assign(src_cnts, src_cnts + n);
            }
            if (extra) {
                keys.push_back(~0ull);
                cnts.push_back((uint32_t)maxkey); // (truncated, not saturated: see saturated_count)
            }
            src_keys = keys.data();
            src_cnts = cnts.data();
            n_src = keys.size();
        }
        // exactness (sketch_exact): either nothing was ever rejected (T still at its initial value), or at least s qualifying
        // hashes lie below T.  Fewer than s below a lowered T means the bound was too tight: a host-imposed cap
        // of the m > 1 phase (sk->bounded), or -- never seen, ~1e-9 per pass -- a sampled tighten pass that overshot.
        if (!sketch_exact(n_src, sk->s, T, sk->hash_max))
            return fail(MHX_E_CAPACITY, "admission threshold was too tight for this input (%zu of %u sketch entries%s); recreate the sketcher with a larger table",
                        n_src, sk->s, sk->bounded ? ", capped threshold" : "");
        const auto t_copy = std::chrono::steady_clock::now();
        const uint32_t nn = n_src < sk->s ? (uint32_t)n_src : sk->s;
        bool in_order = ordered && src_keys == h + 4; // what the ordering kernels promise, checked
        for (size_t i = 1; in_order && i < n_src; ++i) in_order = src_keys[i - 1] < src_keys[i];
        if (in_order) {
            memcpy(hashes, src_keys, (size_t)nn * sizeof(uint64_t));
            if (counts) memcpy(counts, src_cnts, (size_t)nn * sizeof(uint32_t));
        } else {
            sort_pairs(src_keys, src_cnts, n_src, sk->sorted);
            memcpy(hashes, sk->sorted.keys.data(), (size_t)nn * sizeof(uint64_t));
            if (counts) memcpy(counts, sk->sorted.cnts.data(), (size_t)nn * sizeof(uint32_t));
        }
        *n_out = nn;
        if (dbg) {
            const auto t_end = std::chrono::steady_clock::now();
            auto us = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) { return std::chrono::duration<double, std::micro>(b - a).count(); };
            fprintf(stderr, "[mhx finish] device+copy %.0f us (block %zu bytes, %u entries), unpack %.0f us, sort+out %.0f us\n",
                    us(t_begin, t_device), fin_bytes, n, us(t_device, t_copy), us(t_copy, t_end));
        }
        return MHX_OK;
    });
}

extern "C" int mhx_sketcher_export(mhx_sketcher *sk, uint64_t limit, uint64_t *hashes, uint32_t *counts, uint32_t cap, uint32_t *n_out)
{
    return entry("mhx_sketcher_export", [&]() -> int {
        if (!sk || !n_out) return fail(MHX_E_ARG, "null argument");
        int rc = settle(sk);
        if (rc) return rc;
        uint64_t st[kStatCount];
        rc = fetch_stats(sk, st);
        if (rc) return rc;
        rc = check_flags(st[kStatFlags]);
        if (rc) return rc;
        std::vector<uint64_t> keys;
        std::vector<uint32_t> cnts;
        rc = extract(sk, limit, 1, keys, cnts);
        if (rc) return rc;
        if (limit == ~0ull && st[kStatMaxKey]) { keys.push_back(~0ull); cnts.push_back((uint32_t)st[kStatMaxKey]); }
        *n_out = (uint32_t)keys.size();
        if (keys.size() > cap) return fail(MHX_E_CAPACITY, "export: %zu entries, buffer holds %u", keys.size(), cap);
        if (!keys.empty()) {
            if (!hashes || !counts) return fail(MHX_E_ARG, "null output buffer");
            sort_pairs(keys.data(), cnts.data(), keys.size(), sk->sorted);
            memcpy(hashes, sk->sorted.keys.data(), keys.size() * sizeof(uint64_t));
            memcpy(counts, sk->sorted.cnts.data(), cnts.size() * sizeof(uint32_t));
        }
        return MHX_OK;
    });
}
