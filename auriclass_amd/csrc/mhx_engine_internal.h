// mhx_engine_internal.h -- what the engine files (mhx_engine.cpp: engine state and sketcher, mhx_engine_merge.cpp,
// mhx_engine_dist.cpp, mhx_engine_screen.cpp), mhx_files.cpp (file ingest and the calls that read sequence files) and mhx_files_sets.cpp (the
// file-level commands over sketch sets) share.  Internal; the public surface is include/mhx.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <memory>
#include <utility>
#include <vector>

#include "mhx_internal.h"

namespace mhx {

#define HIPCHK(expr)                                                                                   \
    do {                                                                                               \
        hipError_t e_ = (expr);                                                                        \
        if (e_ != hipSuccess) return fail(MHX_E_HIP, "%s failed: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

// ---- owners of HIP resources ----------------------------------------------------------
// Move-only; each releases what it holds in its destructor and when it is assigned to.  They convert to the raw handle,
// so kernels and copies take them as they are.
template <class T, bool Pinned>
class HipArray { // device (Pinned = false) or pinned host array of T, with its capacity in elements
  public:
    HipArray() = default;
    HipArray(T *p, size_t n) : p_(p), n_(n) {} // takes over an allocation of n elements of the same kind
    HipArray(HipArray &&o) noexcept { *this = std::move(o); }
    HipArray &operator=(HipArray &&o) noexcept
    {
        if (this != &o) { reset(); p_ = std::exchange(o.p_, nullptr); n_ = std::exchange(o.n_, 0); }
        return *this;
    }
    ~HipArray() { reset(); }
    operator T *() const { return p_; }
    size_t cap() const { return n_; }
    T *release() { n_ = 0; return std::exchange(p_, nullptr); }
    void reset()
    {
        if (p_) { if (Pinned) hipHostFree(p_); else hipFree(p_); }
        p_ = nullptr;
        n_ = 0;
    }
    // room for n elements: nothing to do if there is; otherwise `sync` (if any) is synchronised, the old array freed and n
    // elements allocated -- the caller decides n.  On failure the array is empty.
    hipError_t grow(size_t n, hipStream_t sync = nullptr)
    {
        if (n_ >= n) return hipSuccess;
        if (sync) { const hipError_t e = hipStreamSynchronize(sync); if (e != hipSuccess) return e; }
        reset();
        const hipError_t e = Pinned ? hipHostMalloc((void **)&p_, n * sizeof(T), hipHostMallocDefault) : hipMalloc((void **)&p_, n * sizeof(T));
        if (e != hipSuccess) { p_ = nullptr; return e; }
        n_ = n;
        return hipSuccess;
    }

  private:
    T *p_ = nullptr;
    size_t n_ = 0;
};
template <class T> using DevArray = HipArray<T, false>;
template <class T> using PinnedArray = HipArray<T, true>;

inline void hip_destroy(hipEvent_t e) { hipEventDestroy(e); }
inline void hip_destroy(hipStream_t s) { hipStreamDestroy(s); }
template <class H>
class HipHandle { // a hipEvent_t or a hipStream_t
  public:
    HipHandle() = default;
    HipHandle(HipHandle &&o) noexcept { *this = std::move(o); }
    HipHandle &operator=(HipHandle &&o) noexcept
    {
        if (this != &o) { reset(); h_ = std::exchange(o.h_, nullptr); }
        return *this;
    }
    ~HipHandle() { reset(); }
    operator H() const { return h_; }
    H *out() { reset(); return &h_; } // for the create call: hipEventCreate(ev.out())
    void reset() { if (h_) hip_destroy(h_); h_ = nullptr; }

  private:
    H h_ = nullptr;
};
using HipEvent = HipHandle<hipEvent_t>;
using HipStream = HipHandle<hipStream_t>;

struct SketcherDestroy { void operator()(mhx_sketcher *sk) const { mhx_sketcher_destroy(sk); } };
using SketcherPtr = std::unique_ptr<mhx_sketcher, SketcherDestroy>;

// FASTA through the device parser (mhx_files.cpp), kept between files and calls: device buffers sized to the largest file
// seen, one sketcher per (k, s) that is reset between files (no hipMalloc / hipFree and no 200 MB table set-up per file)
constexpr uint32_t kFastaSepsInline = 4096; // record positions that come back with the first synchronisation
struct FastaCtx {
    DevArray<uint8_t> d_raw[2]; // file i uses d_raw[i & 1]: file i + 1 is copied in while file i is parsed and sketched
    HipEvent raw_ready[2];
    DevArray<uint8_t> d_out, d_ws;
    DevArray<uint64_t> d_seps;
    PinnedArray<uint64_t> h_words; // [0] stream size, [1] {format flag, #separators}, [2 ..) the first kFastaSepsInline separators
    SketcherPtr sk;
    int k = 0;
    uint32_t s = 0;
    uint64_t scale = 0;
};

// Segmented sketch (mhx_engine_segments.cpp), kept between calls: the staging of a host-pointer call (a round's bytes,
// offsets, rows and lengths) and the sketcher that segments above the cut go through, one per (k, s), reset between them
struct SegCtx {
    DevArray<uint8_t> d_bytes;
    DevArray<uint64_t> d_off, d_rows;
    DevArray<uint32_t> d_len;
    SketcherPtr sk;
    int k = 0;
    uint32_t s = 0;
    uint64_t scale = 0;
};

// ---- engine state ---------------------------------------------------------------------
// The streams come first: they are released last.  The one Engine (g) is never destroyed -- at exit the HIP runtime may
// be gone already; mhx_shutdown releases everything while it is not.
struct Engine {
    HipStream stream;
    HipStream copy_stream; // bulk file ingest and the FASTA loader (created on first use)
    bool ready = false;
    int device = -1;
    int cu_count = 0;      // compute units of the device (mhx_init): sizes the split of a sketcher's first launch
    bool profiling = false;
    HipEvent ev0, ev1;
    double last_dist_ms = 0.0;
    DevArray<uint8_t> dist_ws; // workspace of the all-vs-refs distance path
    DevArray<uint8_t> dist_in; // staging of a host-pointer distance batch (rows, lengths, outputs)
    int last_dist_fallbacks = 0;
    uint64_t last_contain_winner_pairs = 0; // pairs the claim pass of the last mhx_dist_contain_winner call walked
    int last_dist_ranges = 0;    // value ranges per block of the last distance call (0: generic kernel only)
    // the need table of the last containment search or contain-within call (mhx_engine_contain_search.cpp: contain_need_table), on
    // the host, and what it was built from
    std::vector<uint32_t> contain_need;
    int contain_need_k = 0;
    double contain_need_min_identity = 0.0;
    uint32_t contain_need_min_shared = 0;
    // mhx_dist_within (mhx_engine_within.cpp): the cells of a super-batch of queries (mask and base, at most kWithinCells words
    // each), its arrival counter and its arrival list; and the cmin table of the last bound on the device with what it was built from
    DevArray<uint8_t> within_ws;
    DevArray<uint32_t> within_cmin;
    uint32_t within_cmin_s = 0;
    int within_cmin_k = 0;
    double within_cmin_max_dist = 0.0;
    int last_mst_rounds = 0;     // Boruvka rounds of the last mhx_dist_mst call
    int last_mst_stored = -1;    // its pair source: 1 stored, 0 recomputed, -1 none ran
    int last_linkage_rescans = 0; // rows scanned again in the steps of the last mhx_dist_linkage call
    uint64_t last_nj_clamps = 0;  // updates the clamp at 0 changed in the last mhx_dist_nj call
    uint64_t last_medoid_blocks = 0; // blocks the last mhx_dist_medoids call ran << 32 | blocks of its schedule
    PinnedArray<uint8_t> dist_img; // pinned image of the reference sketch file of mhx_dist_files
    // bulk file ingest: pinned staging ring (allocated on first use, kept)
    static constexpr int kPinnedSlots = 4;
    PinnedArray<uint8_t> pinned[kPinnedSlots];
    HipEvent pinned_free[kPinnedSlots];
    FastaCtx fasta;
    SegCtx seg;
    // chunked ingest (.gz FASTQ): pinned host buffers kept between calls, two device slots with their events, a pinned word
    static constexpr size_t kIngestPinnedKeep = 12;
    std::vector<PinnedArray<uint8_t>> ingest_pinned;
    DevArray<uint8_t> ingest_slot[2];
    HipEvent ingest_copied[2], ingest_consumed[2];
    PinnedArray<uint32_t> ingest_word;
    int last_fastq_route = 0; // mhx_last_fastq_route
    DevArray<uint8_t> fqcheck_ws; // per-workgroup summaries of the FASTQ record check (mhx_fqcheck.hip), kept between calls
};
extern Engine &g;
int require_engine();
// What an int-returning entry point of the C ABI that needs the engine runs its work in: the guard (mhx_internal.h) around
// the cleared error text, the engine check and the body.  An entry point that needs no engine uses guarded() as it is.
template <class F> int entry(const char *name, F &&body)
{
    return guarded(name, [&]() -> int {
        clear_error();
        const int rc = require_engine();
        return rc ? rc : body();
    });
}
// room for `bytes` in g.dist_in, the device staging of a host-pointer distance call (mhx_engine_dist.cpp; the triangle's too)
int dist_stage(size_t bytes, uint8_t **out);
// what the two file-level files share (mhx_files.cpp): the text of a call into the caller's buffer (*need: its size with the
// terminator; cap == 0 only asks), and [off, off + len) of fd read into dst by `nthreads` parallel preads (false: short read)
int put_text(const std::string &t, char *buf, size_t cap, size_t *need);
bool parallel_pread(int fd, uint8_t *dst, uint64_t off, size_t len, int nthreads);
// Reference-set search (mhx_engine_search.cpp) of host queries, every row where it lies, against a reference set that the
// caller has put on the device: rows [nr][stride] and len [nr] there, `longest` the largest len.  Outputs as the host form
// of mhx_dist_search.  What mhx_search_files runs per batch of queries: the references are staged once per call.
struct SearchRefs { const uint64_t *rows; const uint32_t *len; uint32_t nr, stride, longest; };
// where search_rows has left the queries on the device ([nq][refs.stride] and [nq], in g.dist_in): good until the next call that stages
struct SearchStaged { const uint64_t *q; const uint32_t *q_len; };
int search_rows(const uint64_t *const *q_rows, const uint32_t *q_len, uint32_t nq, const SearchRefs &refs, int k, uint32_t s, double max_dist,
                uint32_t top, uint32_t *hit_ref, uint32_t *hit_common, uint32_t *hit_denom, double *hit_dist, uint32_t *n_hits,
                SearchStaged *staged = nullptr);
// All references within max_dist (mhx_engine_within.cpp) of host queries, every row where it lies, against a reference set
// that the caller has put on the device (SearchRefs as for search_rows).  Outputs as the host form of mhx_dist_within, the
// capacity protocol included.  What mhx_within_files runs per batch of queries.
int within_rows(const uint64_t *const *q_rows, const uint32_t *q_len, uint32_t nq, const SearchRefs &refs, int k, uint32_t s, double max_dist,
                uint64_t *row_off, uint32_t *hit_ref, uint32_t *hit_common, uint32_t *hit_denom, double *hit_dist, uint64_t cap, uint64_t *n_out);
// Containment (mhx_engine_contain.cpp) of host lists, every row where it lies (q_rows / r_rows: len entries each) or, with the
// row pointers null, as the matrices q / r [.][stride]; host outputs [nq][nr].  What mhx_dist_contain's host form and
// mhx_contain_files run.  With `won` (host, [nq][nr]) the winner-take-all passes run behind the plain one, ref_length ([nr] genome
// lengths or null) ranking ties: mhx_dist_contain_winner's host form and mhx_contain_files_winner.
int contain_rows(const uint64_t *const *q_rows, const uint64_t *q, const uint32_t *q_len, uint32_t nq, uint32_t s_q, const uint64_t *const *r_rows,
                 const uint64_t *r, const uint32_t *r_len, uint32_t nr, uint32_t s_r, uint32_t stride, uint32_t *shared, uint32_t *n_qry, uint32_t *n_ref,
                 const uint64_t *ref_length = nullptr, uint32_t *won = nullptr);
// the geometry of the containment's range route for lists of up to `longest` entries (0: none, the pair kernel takes the call)
uint32_t contain_ranges(uint32_t longest);
// Containment search (mhx_engine_contain_search.cpp) of host queries, every row where it lies (q_len[i] <= refs.stride entries
// each), against a reference set that the caller has put on the device (SearchRefs as for search_rows).  Outputs as the host
// form of mhx_dist_contain_search.  What mhx_contain_files_search runs per batch of queries.
int contain_search_rows(const uint64_t *const *q_rows, const uint32_t *q_len, uint32_t nq, uint32_t s_q, const SearchRefs &refs, uint32_t s_r, int k,
                        double min_identity, uint32_t min_shared, uint32_t top, uint32_t *hit_ref, uint32_t *hit_shared, uint32_t *hit_n_ref,
                        uint32_t *hit_n_qry, uint32_t *n_hits);
// What the containment search and mhx_dist_contain_within share (mhx_engine_contain_search.cpp): the argument checks that
// both make (MHX_E_ARG with the message set), and the need table of a bound -- [limit + 1] on the host, kept in the engine
// state until another (limit, k, min_identity, min_shared) comes.
int contain_hit_check(uint32_t s_q, uint32_t s_r, uint32_t stride, int k, double min_identity, uint32_t min_shared);
const uint32_t *contain_need_table(uint32_t limit, int k, double min_identity, uint32_t min_shared);
// All references a query holds (mhx_engine_contain_within.cpp) of host queries, every row where it lies (q_len[i] <=
// refs.stride entries each), against a reference set that the caller has put on the device (SearchRefs as for search_rows).
// Outputs as the host form of mhx_dist_contain_within, the capacity protocol included.  What mhx_contain_files_within runs per
// batch of queries.
int contain_within_rows(const uint64_t *const *q_rows, const uint32_t *q_len, uint32_t nq, uint32_t s_q, const SearchRefs &refs, uint32_t s_r, int k,
                        double min_identity, uint32_t min_shared, uint64_t *row_off, uint32_t *hit_ref, uint32_t *hit_shared, uint32_t *hit_n_ref,
                        uint32_t *hit_n_qry, uint64_t cap, uint64_t *n_out);
// Jackknife support of search hits (mhx_engine_support.cpp) with everything on the device: what mhx_dist_support's device form
// runs, and mhx_search_files_support on the rows its search has staged.  first [nq][top] is a device pointer; the rep_*
// outputs (each may be null) are device pointers too, or host pointers with host_out.  Uses g.dist_ws, not g.dist_in.
struct SupportCall {
    const uint64_t *q, *r;
    const uint32_t *q_len, *r_len;
    uint32_t nq, nr, stride, s;
    const uint32_t *cand, *n_cand; // cand null: candidates 0 .. top - 1
    uint32_t top, replicates;
    double keep;
    uint64_t seed, T;              // T: support_check's threshold of keep
    uint32_t *first, *rep_best, *rep_s, *rep_common, *rep_denom;
    bool host_out;
};
int support_check(uint32_t stride, uint32_t s, uint32_t top, uint32_t replicates, double keep, uint64_t *T);
int support_device(const SupportCall &c);

} // namespace mhx

// FASTQ pushes stay "unsettled" (their bytes may be read again by a repair pass) until a synchronisation point.  A caller
// that recycles its device buffers push by push (the chunked ingest) asks here whether the push that read `d_bytes`, whose
// kernels it knows to have completed, can be let go: the "repair due" word is read on `side` (not behind the kernels of
// later pushes on the engine stream) into the pinned `word`; still zero -> that push needs no repair and is forgotten;
// set -> everything unsettled is repaired now, while all of it is still intact (full synchronisation).  A push that is
// not on the list any more (an earlier repair has taken it) needs nothing.
int sketcher_release_push(mhx_sketcher *sk, const void *d_bytes, hipStream_t side, uint32_t *word);

// sketcher with `table_scale` times the default candidate table and admission budget
int create_sketcher(int k, uint32_t s, uint32_t min_mult, uint64_t expected_bytes, uint64_t table_scale, mhx_sketcher **out);

// File-level callers only: every MHX_FMT_FASTQ4 push of this sketcher also runs the record check of mhx_fqcheck.h over
// its bytes (a record the kseq reader would read differently raises kFlagBadFastq, finish() returns MHX_E_FORMAT).
// Each push must then start at a record start.  Off by default: the public push API trusts its caller.
void sketcher_verify_fastq(mhx_sketcher *sk, bool on);

// Containment screen at file level: `follower` (the prober of a screener, screener_prober) sees every span that is pushed
// to sk from now on, and every call that settles sk's pushes settles its own.  nullptr: nobody rides along.  The caller
// resets the screener before it attaches its prober to another sketcher.
void sketcher_set_follower(mhx_sketcher *sk, mhx_sketcher *follower);
namespace mhx {
mhx_sketcher *screener_prober(mhx_screener *sc);
// "Estimated genome size" of a reads-mode sketch: 2^bits * n / largest hash (0 for an empty sketch)
double set_size_estimate(int k, const uint64_t *hashes, size_t n);
// Segmented sketch of a stream that lies on the device (the aligned dwords around it readable), offsets and results on the
// host: segment i = [h_off[i], h_off[i + 1]) -- ascending and inside the stream, the caller has seen to that -- gets its
// min(s, distinct) smallest hashes in h_rows[i][..] (stride >= min(s, the largest window count); zero behind h_len[i]).
// (mhx_engine_segments.cpp; what mhx_sketch_segments and the file-level `mash sketch -i` share)
int segments_resident(const uint8_t *d_bytes, const uint64_t *h_off, uint32_t n_seg, int k, uint32_t s, uint32_t stride, uint64_t *h_rows,
                      uint32_t *h_len);
} // namespace mhx
