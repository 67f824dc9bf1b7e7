// mhx_engine_linkage.cpp -- host side of the complete- and average-linkage agglomeration of a sketch set (mhx_dist_linkage):
// the packed triangle of the dense mode computed once, the init pass that turns it into one word per cluster pair, the n - 1
// steps of three launches each, enqueued without a readback between them, and the heights on the host; the cut of finished
// merges (mhx_linkage_labels) and the fixed-point distance (mhx_linkage_fixed_distance), which need no device.
// Rules: mhx_linkage.h; kernels: mhx_linkage.hip and, through the triangle, mhx_triangle.hip and mhx_dist.hip.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdlib.h>

#include <vector>

#include "mhx_device.h"
#include "mhx_linkage.h"
#include "mhx_triangle.h"
#include "mhx_engine_internal.h"
#include "mhx_engine_triangle.h"
#include "mhx_internal.h"

using namespace mhx;

extern "C" int mhx_last_linkage_rescans(void) { return g.last_linkage_rescans; }

extern "C" uint64_t mhx_linkage_fixed_distance(uint32_t common, uint32_t denom, int k)
{
    if (common > denom || denom >= 2 * kMstMaxS || k < 1 || k > 32) return UINT64_MAX;
    return linkage_fixed_distance(common, denom, k);
}

// the cut of finished merges (mhx_linkage.h: linkage_labels): host arithmetic only, no engine needed
extern "C" int64_t mhx_linkage_labels(const uint32_t *merge_a, const uint32_t *merge_b, const double *dist, uint32_t n, double max_dist, uint32_t *label)
{
    return guarded("mhx_linkage_labels", [&]() -> int {
        clear_error();
        if ((n && !label) || (n > 1 && (!merge_a || !merge_b || !dist))) return fail(MHX_E_ARG, "null argument");
        if (n > kTriMaxLists) return fail(MHX_E_ARG, "too many lists (%u, at most %u)", n, kTriMaxLists);
        if (!(max_dist == max_dist)) return fail(MHX_E_ARG, "max_dist is not a number");
        for (uint32_t t = 0; t + 1 < n; ++t)
            if (merge_a[t] >= n || merge_b[t] >= merge_a[t]) return fail(MHX_E_ARG, "merge %u does not name two clusters b < a of 0 .. %u", t, n - 1);
        return (int)linkage_labels(merge_a, merge_b, dist, n, max_dist, label);
    });
}

// Complete / average linkage: the dense mode writes the packed common / denom once, the init pass turns them into the pair
// words, and every step is a pick by one workgroup, an update by one thread per cluster and a rescan of the flagged rows.
// Device memory of size n^2: 8 n (n - 1) / 2 bytes of words for the whole call, and as many again for the triangle's two arrays
// until the init pass has read them (peak 16 n (n - 1) / 2 bytes); the words must fit MHX_LINKAGE_STORE_MB.
extern "C" int mhx_dist_linkage(const uint64_t *rows, const uint32_t *len, uint32_t n, uint32_t stride, int k, uint32_t s, int linkage, uint32_t *merge_a,
                                uint32_t *merge_b, uint32_t *size, uint64_t *num, uint64_t *den, double *dist, int device_ptrs)
{
    return guarded("mhx_dist_linkage", [&]() -> int {
        g.last_linkage_rescans = 0;
        bool done;
        int rc = triangle_check(rows, len, n, stride, k, s, device_ptrs, &done);
        if (rc) return rc;
        if (linkage != kLinkComplete && linkage != kLinkAverage) return fail(MHX_E_ARG, "linkage must be 1 (complete) or 2 (average)");
        if (s >= kMstMaxS) return fail(MHX_E_ARG, "sketch size too large for the linkage (%u, below %u)", s, kMstMaxS);
        if (done) return MHX_OK; // no pair, no merge
        if (!merge_a || !merge_b || !size || !num || !den) return fail(MHX_E_ARG, "null argument");
        const uint64_t pairs = (uint64_t)n * (n - 1) / 2;
        uint64_t budget_mb = 4096;
        if (const char *e = getenv("MHX_LINKAGE_STORE_MB")) { const long long v = atoll(e); if (v >= 0) budget_mb = (uint64_t)v; }
        if (8 * pairs > budget_mb << 20)
            return fail(MHX_E_CAPACITY, "the pair words of %u lists (%llu bytes) do not fit MHX_LINKAGE_STORE_MB = %llu", n, (unsigned long long)(8 * pairs),
                        (unsigned long long)budget_mb);
        // staging: [size][nn][list][ctl, total], host form: [merge_a][merge_b][size][num][den], then rows and lengths
        const size_t bn = up256((size_t)n * 4), be = up256(((size_t)n - 1) * 4), be8 = up256(((size_t)n - 1) * 8);
        const size_t state = 3 * bn + 256;
        TriCall c;
        uint8_t *base = nullptr;
        rc = stage_rows(rows, len, n, stride, k, s, device_ptrs, device_ptrs ? state : state + 3 * be + 2 * be8, &base, c);
        if (rc) return rc;
        LinkArgs a{};
        a.size = (uint32_t *)base; a.nn = (uint32_t *)(base + bn); a.list = (uint32_t *)(base + 2 * bn);
        a.ctl = (uint32_t *)(base + 3 * bn); a.total = (unsigned long long *)(base + 3 * bn + 64);
        a.n = n; a.linkage = linkage; a.k = k;
        if (device_ptrs) { a.merge_a = merge_a; a.merge_b = merge_b; a.size_out = size; a.num = num; a.den = den; a.dist = dist; }
        else {
            uint8_t *out = base + state;
            a.merge_a = (uint32_t *)out; a.merge_b = (uint32_t *)(out + be); a.size_out = (uint32_t *)(out + 2 * be);
            a.num = (uint64_t *)(out + 3 * be); a.den = (uint64_t *)(out + 3 * be + be8);
            a.dist = nullptr; // heights in host arithmetic below
        }
        DevArray<uint64_t> words; // released when the call returns
        DevArray<uint8_t> packed; // the triangle's two arrays: released behind the init pass
        const size_t bp = up256((size_t)pairs * 4);
        if (words.grow(pairs, g.stream) != hipSuccess) return fail(MHX_E_HIP, "hipMalloc failed for the pair words of the linkage (%llu bytes)", (unsigned long long)(8 * pairs));
        if (packed.grow(2 * bp, g.stream) != hipSuccess) return fail(MHX_E_HIP, "hipMalloc failed for the stored pairs of the linkage (%zu bytes)", 2 * bp);
        a.words = words;
        uint32_t *p_common = (uint32_t *)(uint8_t *)packed, *p_denom = (uint32_t *)((uint8_t *)packed + bp);
        rc = run_dense(c, p_common, p_denom, nullptr);
        if (rc) return rc;
        const double tri_ms = g.last_dist_ms;
        hipEventRecord(g.ev0, g.stream);
        hipError_t le = launch_link_init(a, p_common, p_denom, g.stream);
        if (le == hipSuccess) le = launch_link_rescan(a, g.stream);
        if (le == hipSuccess && hipStreamSynchronize(g.stream) != hipSuccess) return fail(MHX_E_HIP, "linkage init kernel failed");
        packed.reset();
        // the steps: nothing comes back between them
        for (uint32_t t = 0; t + 1 < n && le == hipSuccess; ++t) {
            le = launch_link_pick(a, t, g.stream);
            if (le == hipSuccess) le = launch_link_update(a, g.stream);
            if (le == hipSuccess) le = launch_link_rescan(a, g.stream);
        }
        if (le != hipSuccess) return fail(MHX_E_HIP, "linkage kernel launch failed: %s", hipGetErrorString(le));
        hipEventRecord(g.ev1, g.stream);
        uint32_t ctl[6] = {0, 0, 0, 0, 0, 0};
        unsigned long long total = 0;
        hipError_t se = hipMemcpyAsync(ctl, a.ctl, sizeof ctl, hipMemcpyDeviceToHost, g.stream);
        if (se == hipSuccess) se = hipMemcpyAsync(&total, a.total, 8, hipMemcpyDeviceToHost, g.stream);
        if (se == hipSuccess) se = hipStreamSynchronize(g.stream);
        if (se != hipSuccess) return fail(MHX_E_HIP, "linkage kernel failed: %s", hipGetErrorString(se));
        float ms = 0.f;
        hipEventElapsedTime(&ms, g.ev0, g.ev1);
        g.last_dist_ms = tri_ms + ms; // the triangle and the steps (the release of the triangle's arrays between them included)
        total += ctl[4];
        g.last_linkage_rescans = total > (unsigned long long)INT_MAX ? INT_MAX : (int)total;
        if (ctl[5]) return fail(MHX_E_INTERNAL, "a linkage step found no pair to merge");
        if (device_ptrs) return MHX_OK;
        const size_t m = (size_t)n - 1;
        if (hipMemcpy(merge_a, a.merge_a, m * 4, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(merge_b, a.merge_b, m * 4, hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(size, a.size_out, m * 4, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(num, a.num, m * 8, hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(den, a.den, m * 8, hipMemcpyDeviceToHost) != hipSuccess)
            return fail(MHX_E_HIP, "D2H copy failed in dist_linkage");
        if (dist)
            for (size_t t = 0; t < m; ++t) dist[t] = link_height(linkage, num[t], den[t], k);
        return MHX_OK;
    });
}
