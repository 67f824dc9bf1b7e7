// mhx_engine_screen.cpp -- host side of the containment screen (`mash screen`): the screener object and its calls.
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>

#include <algorithm>
#include <exception>
#include <new>
#include <memory>
#include <vector>

#include "mhx_device.h"
#include "mhx_internal.h"
#include "mhx_screen.h"
#include "mhx_sketcher.h"

using namespace mhx;

// ---- containment screen ----------------------------------------------------------------
// `mash screen`: which share of every REFERENCE sketch occurs in a read set, and how often.  A screener is the sketcher's
// push machinery with another table behind it (mhx_screen.h): its prober is an mhx_sketcher in screen mode, so the FASTQ
// line phase, the repair pass for long reads, the chain check, the device flags and the sync contract are the sketcher's
// own code.  For the set size of the mixture it owns an ordinary sketcher (k, s_ref, m = 1) that sees every span too.
struct mhx_screener {
    SketcherPtr probe, setsk;
    int k = 0;
    uint32_t nr = 0, stride = 0, s_ref = 0;
    DevArray<uint64_t> d_rows;
    DevArray<uint32_t> d_len, d_counts, d_res; // d_res: shared[nr] | median[nr]
    DevArray<uint32_t> d_win, d_prio;          // winner-take-all (mhx_screen.h): win[nslots + 1], prio[nr]; allocated by the first winner finish
};

static ScreenArgs screen_args(mhx_screener *sc)
{
    mhx_sketcher *p = sc->probe.get();
    ScreenArgs a;
    a.rows = sc->d_rows; a.len = sc->d_len; a.nr = sc->nr; a.stride = sc->stride;
    a.keys = p->d_keys; a.cnts = p->d_cnts; a.nslots = p->nslots; a.thresh = p->d_thresh; a.stats = p->d_stats;
    a.counts = sc->d_counts; a.shared = sc->d_res; a.median = sc->d_res + sc->nr;
    return a;
}

// counts, counters, tickets and the "repair due" word of the prober to zero; the keys stay
static int screener_clear(mhx_screener *sc)
{
    mhx_sketcher *p = sc->probe.get();
    HIPCHK(launch_screen_clear(screen_args(sc), p->d_tickets, kTicketWords, p->d_need, g.stream));
    p->tickets_used = 0;
    p->unsettled.clear();
    p->bytes_pushed = 0;
    p->hash_ms = 0.0;
    p->launches = 0;
    return MHX_OK;
}

extern "C" int mhx_screener_create(int k, const uint64_t *ref_rows, const uint32_t *ref_len, uint32_t nr, uint32_t stride, uint32_t s_ref,
                                   int with_set_size, int device_ptrs, mhx_screener **out)
{
    return entry("mhx_screener_create", [&]() -> int {
        if (!out) return fail(MHX_E_ARG, "null out pointer");
        if (!hash_k_supported(k)) return fail(MHX_E_ARG, "k-mer size %d not supported (1..32)", k);
        if (nr && (!ref_rows || !ref_len || stride == 0)) return fail(MHX_E_ARG, "null reference rows");
        if (s_ref == 0) return fail(MHX_E_ARG, "sketch size must be positive");
        const uint64_t entries = (uint64_t)nr * stride;
        if (entries > (1ull << 31)) return fail(MHX_E_ARG, "reference set too large for one screen table (%llu entries)", (unsigned long long)entries);
        std::unique_ptr<mhx_screener> sc(new mhx_screener());
        sc->k = k; sc->nr = nr; sc->stride = stride ? stride : 1; sc->s_ref = s_ref;
        std::unique_ptr<mhx_sketcher> p(new mhx_sketcher());
        p->k = k; p->s = s_ref; p->m = 1;
        p->hash32 = k <= 16;
        p->hash_max = p->hash32 ? 0xFFFFFFFFull : ~0ull;
        p->screen = true;
        p->nslots = screen_table_slots(entries);
        hipError_t e = hipSuccess;
        auto A = [&](auto &arr, size_t n) { if (e == hipSuccess) e = arr.grow(n); };
        A(p->d_keys, p->nslots);
        A(p->d_cnts, p->nslots);
        A(p->d_thresh, 1);
        A(p->d_stats, kStatReplicas * kStatCount);
        A(p->d_tickets, kTicketWords);
        A(p->d_need, 1);
        A(p->h_fin, 8); // the pinned landing word of settle()
        A(sc->d_rows, std::max<uint64_t>(entries, 1));
        A(sc->d_len, std::max<uint32_t>(nr, 1));
        A(sc->d_counts, std::max<uint64_t>(entries, 1));
        A(sc->d_res, 2 * (size_t)std::max<uint32_t>(nr, 1));
        if (e != hipSuccess) return fail(MHX_E_HIP, "hipMalloc failed while creating the screener: %s", hipGetErrorString(e));
        sc->probe.reset(p.release());
        if (!device_ptrs)
            for (uint32_t i = 0; i < nr; ++i)
                if (ref_len[i] > stride) return fail(MHX_E_ARG, "ref_len[%u] exceeds stride", i);
        const hipMemcpyKind kind = device_ptrs ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
        if (entries) HIPCHK(hipMemcpyAsync(sc->d_rows, ref_rows, entries * sizeof(uint64_t), kind, g.stream));
        if (nr) HIPCHK(hipMemcpyAsync(sc->d_len, ref_len, (size_t)nr * sizeof(uint32_t), kind, g.stream));
        HIPCHK(hipMemsetAsync(sc->d_counts, 0, std::max<uint64_t>(entries, 1) * sizeof(uint32_t), g.stream));
        HIPCHK(hipMemsetAsync(sc->probe->d_stats, 0, kStatReplicas * kStatCount * sizeof(uint64_t), g.stream));
        HIPCHK(launch_screen_build(screen_args(sc.get()), g.stream));
        uint64_t T = 0, flags = 0;
        HIPCHK(hipMemcpyAsync(&T, sc->probe->d_thresh, sizeof(uint64_t), hipMemcpyDeviceToHost, g.stream));
        HIPCHK(hipMemcpyAsync(&flags, sc->probe->d_stats + kStatFlags, sizeof(uint64_t), hipMemcpyDeviceToHost, g.stream));
        HIPCHK(hipStreamSynchronize(g.stream)); // (the caller's rows are free again)
        if (flags & kFlagTableFull) return fail(MHX_E_INTERNAL, "screen table overflowed while it was built");
        sc->probe->screen_T = T;
        sc->probe->last_T = T;
        int rc = screener_clear(sc.get());
        if (rc) return rc;
        if (with_set_size) {
            mhx_sketcher *ss = nullptr;
            rc = create_sketcher(k, s_ref, 1, 0, 1, &ss);
            if (rc) return rc;
            sc->setsk.reset(ss);
        }
        *out = sc.release();
        return MHX_OK;
    });
}

extern "C" void mhx_screener_destroy(mhx_screener *sc)
{
    if (g.ready) hipStreamSynchronize(g.stream);
    delete sc;
}

extern "C" int mhx_screener_reset(mhx_screener *sc)
{
    return entry("mhx_screener_reset", [&]() -> int {
        if (!sc) return fail(MHX_E_ARG, "null screener");
        int rc = screener_clear(sc);
        if (rc) return rc;
        return sc->setsk ? mhx_sketcher_reset(sc->setsk.get()) : MHX_OK;
    });
}

extern "C" int mhx_screener_push_device(mhx_screener *sc, const void *d_bytes, uint64_t n, int fmt)
{
    return entry("mhx_screener_push_device", [&]() -> int {
        if (!sc) return fail(MHX_E_ARG, "null argument");
        int rc = mhx_sketcher_push_device(sc->probe.get(), d_bytes, n, fmt);
        if (rc || !sc->setsk) return rc;
        return mhx_sketcher_push_device(sc->setsk.get(), d_bytes, n, fmt); // a second launch over the same resident bytes
    });
}

extern "C" int mhx_screener_push_host(mhx_screener *sc, const void *h_bytes, uint64_t n, int fmt)
{
    return entry("mhx_screener_push_host", [&]() -> int {
        if (!sc || (!h_bytes && n)) return fail(MHX_E_ARG, "null argument");
        if (n == 0) return MHX_OK;
        mhx_sketcher *p = sc->probe.get();
        // one staging buffer (the prober's) for both: earlier pushes of either that may still read it come first
        int rc = settle(p);
        if (!rc && sc->setsk) rc = settle(sc->setsk.get());
        if (rc) return rc;
        HIPCHK(hipStreamSynchronize(g.stream));
        if (p->d_stage.cap() < n + 64) HIPCHK(p->d_stage.grow((size_t)((n + 64 + (1u << 20) - 1) & ~(uint64_t)((1u << 20) - 1))));
        HIPCHK(hipMemcpyAsync(p->d_stage, h_bytes, n, hipMemcpyHostToDevice, g.stream));
        return mhx_screener_push_device(sc, p->d_stage, n, fmt);
    });
}

extern "C" int mhx_screener_sync(mhx_screener *sc)
{
    return entry("mhx_screener_sync", [&]() -> int {
        if (!sc) return fail(MHX_E_ARG, "null argument");
        int rc = mhx_sketcher_sync(sc->probe.get());
        if (rc || !sc->setsk) return rc;
        return mhx_sketcher_sync(sc->setsk.get());
    });
}

namespace mhx {
double set_size_estimate(int k, const uint64_t *hashes, size_t n)
{
    return n ? pow(2.0, k > 16 ? 64.0 : 32.0) * (double)n / (double)hashes[n - 1] : 0.0;
}
mhx_sketcher *screener_prober(mhx_screener *sc) { return sc ? sc->probe.get() : nullptr; }
} // namespace mhx

// Winner-take-all behind the plain tally, which has just been launched: its shared[] comes to the host and becomes the
// priority order, the winner words go back to "nobody" (the counts have changed since the last call), every entry claims
// its key, and the tally runs again in its winner form into the same result buffers.
static int screener_winner_passes(mhx_screener *sc, const uint64_t *ref_length, uint64_t maxkey)
{
    mhx_sketcher *p = sc->probe.get();
    const uint32_t nr = sc->nr;
    std::vector<uint32_t> shared0(nr), len(nr), prio(nr);
    HIPCHK(hipMemcpyAsync(shared0.data(), sc->d_res, (size_t)nr * sizeof(uint32_t), hipMemcpyDeviceToHost, g.stream));
    HIPCHK(hipMemcpyAsync(len.data(), sc->d_len, (size_t)nr * sizeof(uint32_t), hipMemcpyDeviceToHost, g.stream));
    HIPCHK(hipStreamSynchronize(g.stream));
    screen_priorities(shared0.data(), len.data(), ref_length, nr, prio.data());
    if (!sc->d_win.cap()) {
        hipError_t e = sc->d_win.grow(p->nslots + 1);
        if (e == hipSuccess) e = sc->d_prio.grow(nr);
        if (e != hipSuccess) return fail(MHX_E_HIP, "hipMalloc failed for the winner words of the screener: %s", hipGetErrorString(e));
    }
    HIPCHK(hipMemcpyAsync(sc->d_prio, prio.data(), (size_t)nr * sizeof(uint32_t), hipMemcpyHostToDevice, g.stream));
    static_assert(kScreenNobody == 0, "the winner words are vacated by a memset");
    HIPCHK(hipMemsetAsync(sc->d_win, 0, (size_t)(p->nslots + 1) * sizeof(uint32_t), g.stream));
    const ScreenArgs a = screen_args(sc);
    HIPCHK(launch_screen_winner(a, sc->d_win, sc->d_prio, maxkey, g.stream));
    HIPCHK(launch_screen_tally_winner(a, sc->d_win, sc->d_prio, g.stream));
    HIPCHK(hipStreamSynchronize(g.stream)); // (prio is free again)
    return MHX_OK;
}

static int screener_finish_impl(mhx_screener *sc, bool winner, const uint64_t *ref_length, uint32_t *shared, uint32_t *median, double *set_size,
                                uint32_t *counts)
{
    if (!sc || (sc->nr && (!shared || !median))) return fail(MHX_E_ARG, "null argument");
    mhx_sketcher *p = sc->probe.get();
    int rc = settle(p); // the repair pass of long reads, if one is due
    if (rc) return rc;
    uint64_t st[kStatCount];
    rc = fetch_stats(p, st);
    if (rc) return rc;
    rc = check_flags(st[kStatFlags]);
    if (rc) return rc;
    if (st[kStatFlags] & kFlagCountWrap) return fail(MHX_E_CAPACITY, "a multiplicity counter of the screen table reached its limit");
    if (sc->nr) {
        HIPCHK(launch_screen_tally(screen_args(sc), g.stream));
        if (winner) {
            rc = screener_winner_passes(sc, ref_length, st[kStatMaxKey]);
            if (rc) return rc;
        }
        std::vector<uint32_t> res(2 * (size_t)sc->nr);
        HIPCHK(hipMemcpyAsync(res.data(), sc->d_res, res.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, g.stream));
        if (counts) HIPCHK(hipMemcpyAsync(counts, sc->d_counts, (size_t)sc->nr * sc->stride * sizeof(uint32_t), hipMemcpyDeviceToHost, g.stream));
        HIPCHK(hipStreamSynchronize(g.stream));
        memcpy(shared, res.data(), (size_t)sc->nr * sizeof(uint32_t));
        memcpy(median, res.data() + sc->nr, (size_t)sc->nr * sizeof(uint32_t));
    }
    double size = 0.0;
    if (sc->setsk) {
        std::vector<uint64_t> h(sc->s_ref);
        uint32_t n = 0;
        rc = mhx_sketcher_finish(sc->setsk.get(), h.data(), nullptr, &n);
        if (rc) return rc;
        size = set_size_estimate(sc->k, h.data(), n);
    }
    if (set_size) *set_size = size;
    return MHX_OK;
}

extern "C" int mhx_screener_finish(mhx_screener *sc, uint32_t *shared, uint32_t *median, double *set_size, uint32_t *counts)
{
    return entry("mhx_screener_finish", [&] { return screener_finish_impl(sc, false, nullptr, shared, median, set_size, counts); });
}

extern "C" int mhx_screener_finish_winner(mhx_screener *sc, const uint64_t *ref_length, uint32_t *shared, uint32_t *median, double *set_size,
                                          uint32_t *counts)
{
    return entry("mhx_screener_finish_winner", [&] { return screener_finish_impl(sc, true, ref_length, shared, median, set_size, counts); });
}
