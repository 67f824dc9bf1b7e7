// mhx_engine_dist.cpp -- host side of the batched distance call: staging of a host-pointer batch, the choice between the
// all-vs-refs fast path and the generic pair kernel (mhx_dist.hip), and the figures of the last call.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdlib.h>

#include <algorithm>
#include <exception>
#include <new>
#include <vector>

#include "mhx_device.h"
#include "mhx_dist.h"
#include "mhx_engine_sets.h"
#include "mhx_internal.h"

using namespace mhx;

// ---- batched distance ------------------------------------------------------------------
extern "C" double mhx_last_dist_kernel_ms(void) { return g.last_dist_ms; }
extern "C" int mhx_last_dist_fallback_blocks(void) { return g.last_dist_fallbacks; }
extern "C" int mhx_last_dist_ranges(void) { return g.last_dist_ranges; }

// Persistent device staging of the host-pointer form (one buffer, grown on demand): six hipMalloc / hipFree pairs per
// call cost more than the kernels of an AuriClass-sized comparison (1 query x 24 references).
namespace mhx {
int dist_stage(size_t bytes, uint8_t **out)
{
    if (g.dist_in.cap() < bytes) {
        const size_t cap = (bytes + bytes / 4 + (1u << 20)) & ~(size_t)((1u << 20) - 1);
        if (g.dist_in.grow(cap, g.stream) != hipSuccess) return fail(MHX_E_HIP, "hipMalloc failed for the distance staging area (%zu bytes)", cap);
    }
    *out = g.dist_in;
    return MHX_OK;
}
} // namespace mhx

// q_rows / r_rows (host form only): the rows where they lie, one pointer each (q / r are then unused) -- mhx_dist_files
// hands over the hash lists inside its pinned image of the reference sketch file instead of building padded matrices
static int dist_batch_core(const uint64_t *q, const uint32_t *q_len, uint32_t nq, const uint64_t *r, const uint32_t *r_len,
                           uint32_t nr, uint32_t stride, int k, uint32_t s, uint32_t *common, uint32_t *denom, double *dist,
                           int device_ptrs, const uint64_t *const *q_rows, const uint64_t *const *r_rows)
{
    if (nq == 0 || nr == 0) return MHX_OK;
    if ((!q && !q_rows) || !q_len || (!r && !r_rows) || !r_len || !common || !denom) return fail(MHX_E_ARG, "null argument");
    if (device_ptrs && (q_rows || r_rows)) return fail(MHX_E_ARG, "row pointers are a host form");
    if (k < 1 || k > 32 || s == 0 || stride == 0) return fail(MHX_E_ARG, "bad k / s / stride");
    const uint64_t pairs = (uint64_t)nq * nr;
    if (pairs > 0x7FFFFFFFull) return fail(MHX_E_ARG, "too many pairs for one call");
    DistArgs a;
    a.nq = nq; a.nr = nr; a.stride = stride; a.s = s; a.k = k; a.out_stride = nr; a.out_off = 0;
    uint32_t *dc = nullptr, *dd = nullptr;
    if (device_ptrs) {
        a.q = q; a.q_len = q_len; a.r = r; a.r_len = r_len; a.common = common; a.denom = denom; a.dist = dist;
    } else {
        for (uint32_t i = 0; i < nq; ++i) if (q_len[i] > stride) return fail(MHX_E_ARG, "q_len[%u] exceeds stride", i);
        for (uint32_t i = 0; i < nr; ++i) if (r_len[i] > stride) return fail(MHX_E_ARG, "r_len[%u] exceeds stride", i);
        const size_t bq = up256((size_t)nq * stride * 8), br = up256((size_t)nr * stride * 8), bql = up256((size_t)nq * 4), brl = up256((size_t)nr * 4), bo = up256(pairs * 4);
        uint8_t *base = nullptr;
        const int rc = dist_stage(bq + br + bql + brl + 2 * bo, &base);
        if (rc) return rc;
        uint8_t *dq = base, *dr = dq + bq, *dql = dr + br, *drl = dql + bql;
        dc = (uint32_t *)(drl + brl);
        dd = (uint32_t *)(drl + brl + bo);
        // rows that are mostly padding travel one by one (valid prefix only), full ones as one block
        hipError_t ce = hipSuccess;
        auto rows = [&](uint8_t *dst, const uint64_t *src, const uint32_t *len, uint32_t n, const uint64_t *const *ptrs) {
            if (ptrs) { // every row from its own place
                for (uint32_t i = 0; i < n && ce == hipSuccess; ++i)
                    if (len[i]) ce = hipMemcpyAsync(dst + (size_t)i * stride * 8, ptrs[i], (size_t)len[i] * 8, hipMemcpyHostToDevice, g.stream);
                return;
            }
            uint64_t valid = 0;
            for (uint32_t i = 0; i < n; ++i) valid += len[i];
            if (n > 64 || valid * 2 >= (uint64_t)n * stride) {
                if (ce == hipSuccess) ce = hipMemcpyAsync(dst, src, (size_t)n * stride * 8, hipMemcpyHostToDevice, g.stream);
                return;
            }
            for (uint32_t i = 0; i < n && ce == hipSuccess; ++i)
                if (len[i]) ce = hipMemcpyAsync(dst + (size_t)i * stride * 8, src + (size_t)i * stride, (size_t)len[i] * 8, hipMemcpyHostToDevice, g.stream);
        };
        rows(dq, q, q_len, nq, q_rows);
        rows(dr, r, r_len, nr, r_rows);
        if (ce == hipSuccess) ce = hipMemcpyAsync(dql, q_len, (size_t)nq * 4, hipMemcpyHostToDevice, g.stream);
        if (ce == hipSuccess) ce = hipMemcpyAsync(drl, r_len, (size_t)nr * 4, hipMemcpyHostToDevice, g.stream);
        if (ce != hipSuccess) return fail(MHX_E_HIP, "H2D copy failed in dist_batch: %s", hipGetErrorString(ce));
        a.q = (const uint64_t *)dq; a.q_len = (const uint32_t *)dql; a.r = (const uint64_t *)dr; a.r_len = (const uint32_t *)drl;
        a.common = dc; a.denom = dd; a.dist = nullptr; // distances in host libm below
    }
    // all-vs-refs fast path: the references go through in slices of 32 (one bit each in the range kernel's masks), the
    // queries in batches (MHX_DIST_QBATCH; default: all at once), every (batch, slice) filling its block of the [nq][nr]
    // outputs; the generic pair-per-workgroup kernel serves tiny batches and is the fallback of a block whose value
    // ranges are too uneven for the LDS table.  Nothing is read back between the blocks: every block has its own flag
    // word, all of them come back with ONE copy behind the last launch.
    // (few pairs of LONG lists take it too -- AuriClass's own call, 1 query x 24 references at s = 50 000: 0.48 ms in the
    // generic kernel, whose 24 workgroups each walk 100 000 elements)
    // The number of value ranges follows the longest list of the call (its length, never its values; the row stride where
    // the lengths are on the device): 1024 x W, W = 1 up to 65 536 entries -- the kernels, grids and workspace of round 3 --
    // up to 16 at 2^20 (mhx_dist.h: dist_windows), so that sketches of up to 1 000 000 hashes keep slices of at most 64
    // entries and stay on this path; longer lists have no geometry and go to the generic kernel.
    uint32_t longest = stride;
    if (!device_ptrs) {
        longest = 0;
        for (uint32_t i = 0; i < nq; ++i) longest = std::max(longest, q_len[i]);
        for (uint32_t i = 0; i < nr; ++i) longest = std::max(longest, r_len[i]);
    }
    const uint32_t windows = dist_windows(longest), ranges = (uint32_t)kDistRanges * windows;
    const bool fast = (pairs >= 64 || (pairs >= 8 && pairs * (uint64_t)s >= 400000)) && windows != 0 && getenv("MHX_DIST_GENERIC") == nullptr;
    uint32_t qbatch = nq;
    if (const char *e = getenv("MHX_DIST_QBATCH")) { const long v = atol(e); if (v > 0 && (uint64_t)v < nq) qbatch = (uint32_t)v; }
    if (windows > 1) qbatch = std::min(qbatch, dist_wide_max_queries(nr < 32 ? nr : 32, ranges)); // the workspace stays below kDistWideWorkLimit
    const uint32_t nslices = (nr + 31) / 32, nbatches = (nq + qbatch - 1) / qbatch, nblocks = nslices * nbatches;
    DistWork w{};
    uint32_t *d_params = nullptr;
    if (fast) {
        size_t oq, orr, oc, ow, op;
        const size_t need = dist_work_bytes(qbatch, nr < 32 ? nr : 32, ranges, &oq, &orr, &oc, &ow, &op) + (size_t)std::min(nblocks, kBlockGroup) * 8;
        if (g.dist_ws.grow(need, g.stream) != hipSuccess) return fail(MHX_E_HIP, "hipMalloc failed for the distance workspace");
        w.offs_q = (uint32_t *)(g.dist_ws + oq); w.offs_r = (uint32_t *)(g.dist_ws + orr);
        w.cpart = g.dist_ws + oc;
        w.wtot = (uint32_t *)(g.dist_ws + ow);
        w.ranges = ranges;
        d_params = (uint32_t *)(g.dist_ws + op); // [block][2]: shift, overflow flag
    }
    auto block_args = [&](uint32_t b) {
        const uint32_t q0 = (b / nslices) * qbatch, r0 = (b % nslices) * 32;
        DistArgs x = a;
        x.q = a.q + (uint64_t)q0 * stride;
        x.q_len = a.q_len + q0;
        x.nq = nq - q0 < qbatch ? nq - q0 : qbatch;
        x.r = a.r + (uint64_t)r0 * stride;
        x.r_len = a.r_len + r0;
        x.nr = nr - r0 < 32 ? nr - r0 : 32;
        x.common = a.common + (uint64_t)q0 * nr;
        x.denom = a.denom + (uint64_t)q0 * nr;
        x.dist = a.dist ? a.dist + (uint64_t)q0 * nr : nullptr;
        x.out_off = r0;
        return x;
    };
    hipEventRecord(g.ev0, g.stream);
    hipError_t le = hipSuccess;
    if (!fast) { le = launch_dist_pairs(a, g.stream); g.last_dist_fallbacks = -1; }
    if (fast) g.last_dist_fallbacks = 0;
    g.last_dist_ranges = 0;
    if (fast) {
        const int rc = run_block_groups(
            BlockGroups{nblocks, true, d_params, std::min(nblocks, kBlockGroup), false, false, true, "dist"}, le,
            [&](uint64_t b, uint32_t *params) { w.params = params; return launch_dist_ranges(block_args((uint32_t)b), w, g.stream); },
            [&](uint64_t b) { return launch_dist_pairs(block_args((uint32_t)b), g.stream); });
        if (rc) return rc;
    }
    hipEventRecord(g.ev1, g.stream);
    if (fast && (uint32_t)g.last_dist_fallbacks < nblocks) g.last_dist_ranges = (int)ranges; // (0: the generic kernel did all the work)
    if (le != hipSuccess) return fail(MHX_E_HIP, "dist kernel launch failed: %s", hipGetErrorString(le));
    hipError_t se = hipSuccess;
    if (!device_ptrs) {
        se = hipMemcpyAsync(common, dc, pairs * 4, hipMemcpyDeviceToHost, g.stream);
        if (se == hipSuccess) se = hipMemcpyAsync(denom, dd, pairs * 4, hipMemcpyDeviceToHost, g.stream);
    }
    if (se == hipSuccess) se = hipStreamSynchronize(g.stream);
    float ms = 0.f;
    hipEventElapsedTime(&ms, g.ev0, g.ev1);
    g.last_dist_ms = ms;
    if (se != hipSuccess) return fail(MHX_E_HIP, "dist kernel failed: %s", hipGetErrorString(se));
    if (!device_ptrs && dist) {
        for (uint64_t i = 0; i < pairs; ++i) dist[i] = tri_distance(common[i], denom[i], k);
    }
    return MHX_OK;
}

extern "C" int mhx_dist_batch(const uint64_t *q, const uint32_t *q_len, uint32_t nq, const uint64_t *r, const uint32_t *r_len,
                              uint32_t nr, uint32_t stride, int k, uint32_t s, uint32_t *common, uint32_t *denom, double *dist,
                              int device_ptrs)
{
    return entry("mhx_dist_batch", [&] { return dist_batch_core(q, q_len, nq, r, r_len, nr, stride, k, s, common, denom, dist, device_ptrs, nullptr, nullptr); });
}

namespace mhx {
int dist_batch_rows(const uint64_t *const *q_rows, const uint32_t *q_len, uint32_t nq, const uint64_t *const *r_rows, const uint32_t *r_len,
                    uint32_t nr, int k, uint32_t s, uint32_t *common, uint32_t *denom, double *dist)
{
    uint32_t stride = 16;
    for (uint32_t i = 0; i < nq; ++i) stride = q_len[i] > stride ? q_len[i] : stride;
    for (uint32_t i = 0; i < nr; ++i) stride = r_len[i] > stride ? r_len[i] : stride;
    stride = (stride + 15u) & ~15u; // rows of whole 128-byte lines on the device
    return dist_batch_core(nullptr, q_len, nq, nullptr, r_len, nr, stride, k, s, common, denom, dist, 0, q_rows, r_rows);
}
} // namespace mhx
