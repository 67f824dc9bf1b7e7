// mhx_engine_support.cpp -- host side of the jackknife support of search hits (mhx_dist_support): the checks, the staging of a
// host-pointer call, the cut of the queries into batches whose workspace stays below kSupportWorkLimit (MHX_SUPPORT_WORK_MB),
// the four launches of a batch and the one word that tells of a replicate without hashes.  What mhx_search_files_support runs
// on the rows its search has staged is support_device below.  Rules: mhx_support.h; kernels: mhx_support.hip.
#include <hip/hip_runtime.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "mhx_device.h"
#include "mhx_support.h"
#include "mhx_engine_sets.h"
#include "mhx_internal.h"

using namespace mhx;

namespace mhx {

int support_check(uint32_t stride, uint32_t s, uint32_t top, uint32_t replicates, double keep, uint64_t *T)
{
    if (s == 0 || stride == 0) return fail(MHX_E_ARG, "bad s / stride");
    if (top < 1 || top > kSupportMaxTop) return fail(MHX_E_ARG, "top must be 1 .. %u", kSupportMaxTop);
    if (!resample_threshold(keep, T)) return fail(MHX_E_ARG, "keep must lie in (0, 1] (%g)", keep);
    if (replicates < 1 || replicates > kResampleMaxReplicates) return fail(MHX_E_ARG, "replicates must be 1 .. %u (%u)", kResampleMaxReplicates, replicates);
    return MHX_OK;
}

// Launches the whole call on the engine's stream and waits for it.  The workspace (g.dist_ws) holds one batch; outputs that
// are device pointers are written where they belong, host outputs are copied out batch by batch.
int support_device(const SupportCall &c)
{
    const uint32_t R = c.replicates;
    uint64_t limit = kSupportWorkLimit;
    if (const char *e = getenv("MHX_SUPPORT_WORK_MB")) { const long v = atol(e); if (v > 0) limit = (uint64_t)v << 20; }
    const uint32_t batch = std::min(support_batch(c.top, R, limit), c.nq);
    const size_t b_one = (size_t)batch * R * 4, b_pair = (size_t)batch * c.top * R * 4;
    Carve work;
    const size_t o_bad = work.take(8), o_kept = work.take((size_t)batch * (c.top + 1) * R * 4), o_s = work.take(b_one), o_best = work.take(b_one);
    const size_t o_common = work.take(b_pair), o_denom = work.take(b_pair);
    if (g.dist_ws.grow(work.bytes, g.stream) != hipSuccess) return fail(MHX_E_HIP, "hipMalloc failed for the support workspace (%zu bytes)", work.bytes);
    uint8_t *ws = g.dist_ws;
    unsigned long long *bad = (unsigned long long *)(ws + o_bad);
    hipEventRecord(g.ev0, g.stream);
    hipError_t le = hipMemsetAsync(bad, 0xFF, 8, g.stream);
    if (le == hipSuccess) le = hipMemsetAsync(c.first, 0, (size_t)c.nq * c.top * 4, g.stream);
    const bool direct = !c.host_out;
    for (uint32_t q0 = 0; q0 < c.nq && le == hipSuccess; q0 += batch) {
        const uint32_t nq = std::min(batch, c.nq - q0);
        const size_t one = (size_t)q0 * R, pair = (size_t)q0 * c.top * R;
        SupportArgs a{};
        a.q = c.q + (uint64_t)q0 * c.stride; a.q_len = c.q_len + q0; a.r = c.r; a.r_len = c.r_len;
        a.nq = nq; a.nr = c.nr; a.stride = c.stride; a.s = c.s;
        a.cand = c.cand ? c.cand + (size_t)q0 * c.top : nullptr; a.n_cand = c.cand ? c.n_cand + q0 : nullptr;
        a.top = c.top; a.replicates = R; a.seed = c.seed; a.threshold = c.T; a.q0 = q0;
        a.kept = (uint32_t *)(ws + o_kept);
        a.s_r = direct && c.rep_s ? c.rep_s + one : (uint32_t *)(ws + o_s);
        a.best = direct ? (c.rep_best ? c.rep_best + one : nullptr) : (uint32_t *)(ws + o_best);
        a.common = direct && c.rep_common ? c.rep_common + pair : (uint32_t *)(ws + o_common);
        a.denom = direct && c.rep_denom ? c.rep_denom + pair : (uint32_t *)(ws + o_denom);
        a.first = c.first + (size_t)q0 * c.top;
        a.bad = bad;
        le = launch_support_count(a, g.stream);
        if (le == hipSuccess) le = launch_support_s(a, g.stream);
        if (le == hipSuccess) le = launch_support_pairs(a, g.stream);
        if (le == hipSuccess) le = launch_support_best(a, g.stream);
        if (direct) continue;
        if (le == hipSuccess && c.rep_best) le = hipMemcpyAsync(c.rep_best + one, a.best, (size_t)nq * R * 4, hipMemcpyDeviceToHost, g.stream);
        if (le == hipSuccess && c.rep_s) le = hipMemcpyAsync(c.rep_s + one, a.s_r, (size_t)nq * R * 4, hipMemcpyDeviceToHost, g.stream);
        if (le == hipSuccess && c.rep_common) le = hipMemcpyAsync(c.rep_common + pair, a.common, (size_t)nq * c.top * R * 4, hipMemcpyDeviceToHost, g.stream);
        if (le == hipSuccess && c.rep_denom) le = hipMemcpyAsync(c.rep_denom + pair, a.denom, (size_t)nq * c.top * R * 4, hipMemcpyDeviceToHost, g.stream);
    }
    hipEventRecord(g.ev1, g.stream);
    if (le != hipSuccess) return fail(MHX_E_HIP, "support kernel launch failed: %s", hipGetErrorString(le));
    unsigned long long back = 0;
    hipError_t se = hipMemcpyAsync(&back, bad, 8, hipMemcpyDeviceToHost, g.stream);
    if (se == hipSuccess) se = hipStreamSynchronize(g.stream);
    float ms = 0.f;
    hipEventElapsedTime(&ms, g.ev0, g.ev1);
    g.last_dist_ms = ms;
    g.last_dist_fallbacks = -1;
    g.last_dist_ranges = 0;
    if (se != hipSuccess) return fail(MHX_E_HIP, "support kernel failed: %s", hipGetErrorString(se));
    if (back != ~0ull)
        return fail(MHX_E_ARG, "query %u: replicate %u keeps no hash of a full list at keep = %g", (uint32_t)(back >> 32), (uint32_t)back, c.keep);
    return MHX_OK;
}

} // namespace mhx

extern "C" int mhx_dist_support(const uint64_t *q, const uint32_t *q_len, uint32_t nq, const uint64_t *r, const uint32_t *r_len, uint32_t nr, uint32_t stride,
                                uint32_t s, const uint32_t *cand, const uint32_t *n_cand, uint32_t top, uint32_t replicates, double keep, uint64_t seed,
                                uint32_t *first, uint32_t *rep_best, uint32_t *rep_s, uint32_t *rep_common, uint32_t *rep_denom, int device_ptrs)
{
    return entry("mhx_dist_support", [&]() -> int {
        uint64_t T = 0;
        int rc = support_check(stride, s, top, replicates, keep, &T);
        if (rc) return rc;
        if (!cand && (nr > kSupportMaxTop || top != nr)) return fail(MHX_E_ARG, "without a candidate list top must be nr, and nr at most %u", kSupportMaxTop);
        if (nq == 0) return MHX_OK;
        if (!q || !q_len || !first || (nr && (!r || !r_len)) || (cand && !n_cand) || !rep_common != !rep_denom) return fail(MHX_E_ARG, "null argument");
        SupportCall c{};
        c.nq = nq; c.nr = nr; c.stride = stride; c.s = s; c.top = top; c.replicates = replicates; c.keep = keep; c.seed = seed; c.T = T;
        c.rep_best = rep_best; c.rep_s = rep_s; c.rep_common = rep_common; c.rep_denom = rep_denom;
        if (device_ptrs) {
            c.q = q; c.q_len = q_len; c.r = r; c.r_len = r_len; c.cand = cand; c.n_cand = n_cand; c.first = first;
            return support_device(c);
        }
        for (uint32_t i = 0; i < nq; ++i) if (q_len[i] > stride) return fail(MHX_E_ARG, "q_len[%u] exceeds stride", i);
        for (uint32_t i = 0; i < nr; ++i) if (r_len[i] > stride) return fail(MHX_E_ARG, "r_len[%u] exceeds stride", i);
        if (cand)
            for (uint32_t i = 0; i < nq; ++i) {
                const uint32_t *row = cand + (size_t)i * top;
                if (n_cand[i] > top) return fail(MHX_E_ARG, "n_cand[%u] exceeds top", i);
                for (uint32_t x = 0; x < n_cand[i]; ++x) {
                    if (row[x] >= nr) return fail(MHX_E_ARG, "candidate %u of query %u is no reference (%u of %u)", x, i, row[x], nr);
                    for (uint32_t y = 0; y < x; ++y) if (row[y] == row[x]) return fail(MHX_E_ARG, "query %u names reference %u twice", i, row[x]);
                }
            }
        // staging: [query rows][query lengths][reference rows][reference lengths][candidates][their numbers][first]
        Carve in;
        const size_t o_q = in.take((size_t)nq * stride * 8), o_ql = in.take((size_t)nq * 4), o_r = in.take((size_t)nr * stride * 8), o_rl = in.take((size_t)nr * 4);
        const size_t o_c = in.take((size_t)nq * top * 4), o_n = in.take((size_t)nq * 4), o_f = in.take((size_t)nq * top * 4);
        uint8_t *base = nullptr;
        rc = dist_stage(in.bytes, &base);
        if (rc) return rc;
        uint8_t *dq = base + o_q, *dql = base + o_ql, *dr = base + o_r, *drl = base + o_rl, *dc = base + o_c, *dn = base + o_n, *df = base + o_f;
        hipError_t ce = hipMemcpyAsync(dq, q, (size_t)nq * stride * 8, hipMemcpyHostToDevice, g.stream);
        if (ce == hipSuccess) ce = hipMemcpyAsync(dql, q_len, (size_t)nq * 4, hipMemcpyHostToDevice, g.stream);
        if (ce == hipSuccess && nr) ce = hipMemcpyAsync(dr, r, (size_t)nr * stride * 8, hipMemcpyHostToDevice, g.stream);
        if (ce == hipSuccess && nr) ce = hipMemcpyAsync(drl, r_len, (size_t)nr * 4, hipMemcpyHostToDevice, g.stream);
        if (ce == hipSuccess && cand) ce = hipMemcpyAsync(dc, cand, (size_t)nq * top * 4, hipMemcpyHostToDevice, g.stream);
        if (ce == hipSuccess && cand) ce = hipMemcpyAsync(dn, n_cand, (size_t)nq * 4, hipMemcpyHostToDevice, g.stream);
        if (ce != hipSuccess) return fail(MHX_E_HIP, "H2D copy failed in dist_support: %s", hipGetErrorString(ce));
        c.q = (const uint64_t *)dq; c.q_len = (const uint32_t *)dql; c.r = (const uint64_t *)dr; c.r_len = (const uint32_t *)drl;
        c.cand = cand ? (const uint32_t *)dc : nullptr; c.n_cand = cand ? (const uint32_t *)dn : nullptr;
        c.first = (uint32_t *)df;
        c.host_out = true;
        rc = support_device(c);
        return rc ? rc : read_back("dist_support", {{first, c.first, (size_t)nq * top * 4}});
    });
}
