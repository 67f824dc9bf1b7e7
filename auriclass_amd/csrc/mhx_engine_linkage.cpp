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
        rc = store_fits("MHX_LINKAGE_STORE_MB", n);
        if (rc) return rc;
        const size_t m = (size_t)n - 1;
        Carve in; // staging: [size][nn][list][ctl, total], host form: [merge_a][merge_b][size][num][den], then rows and lengths
        const size_t o_size = in.take((size_t)n * 4), o_nn = in.take((size_t)n * 4), o_list = in.take((size_t)n * 4), o_ctl = in.take(256);
        const size_t o_a = in.take(device_ptrs ? 0 : m * 4), o_b = in.take(device_ptrs ? 0 : m * 4), o_sz = in.take(device_ptrs ? 0 : m * 4);
        const size_t o_num = in.take(device_ptrs ? 0 : m * 8), o_den = in.take(device_ptrs ? 0 : m * 8);
        TriCall c;
        uint8_t *base = nullptr;
        rc = stage_rows(rows, len, n, stride, k, s, device_ptrs, in, &base, c);
        if (rc) return rc;
        LinkArgs a{};
        a.size = (uint32_t *)(base + o_size); a.nn = (uint32_t *)(base + o_nn); a.list = (uint32_t *)(base + o_list);
        a.ctl = (uint32_t *)(base + o_ctl); a.total = (unsigned long long *)(base + o_ctl + 64);
        a.n = n; a.linkage = linkage; a.k = k;
        if (device_ptrs) { a.merge_a = merge_a; a.merge_b = merge_b; a.size_out = size; a.num = num; a.den = den; a.dist = dist; }
        else {
            a.merge_a = (uint32_t *)(base + o_a); a.merge_b = (uint32_t *)(base + o_b); a.size_out = (uint32_t *)(base + o_sz);
            a.num = (uint64_t *)(base + o_num); a.den = (uint64_t *)(base + o_den);
            a.dist = nullptr; // heights in host arithmetic below
        }
        StoredTriangle tri; // the words: released when the call returns; the triangle's two arrays: behind the init pass
        rc = tri.alloc((uint64_t)n * (n - 1) / 2, "the linkage", true);
        if (rc) return rc;
        a.words = tri.words;
        rc = run_dense(c, tri.common, tri.denom, nullptr);
        if (rc) return rc;
        StepsClock clock;
        hipError_t le = launch_link_init(a, tri.common, tri.denom, g.stream);
        if (le == hipSuccess) le = launch_link_rescan(a, g.stream);
        if (le == hipSuccess && hipStreamSynchronize(g.stream) != hipSuccess) return fail(MHX_E_HIP, "linkage init kernel failed");
        tri.reset();
        // the steps: nothing comes back between them
        for (uint32_t t = 0; t + 1 < n && le == hipSuccess; ++t) {
            le = launch_link_pick(a, t, g.stream);
            if (le == hipSuccess) le = launch_link_update(a, g.stream);
            if (le == hipSuccess) le = launch_link_rescan(a, g.stream);
        }
        if (le != hipSuccess) return fail(MHX_E_HIP, "linkage kernel launch failed: %s", hipGetErrorString(le));
        clock.stop();
        uint32_t ctl[6] = {0, 0, 0, 0, 0, 0};
        unsigned long long total = 0;
        hipError_t se = hipMemcpyAsync(ctl, a.ctl, sizeof ctl, hipMemcpyDeviceToHost, g.stream);
        if (se == hipSuccess) se = hipMemcpyAsync(&total, a.total, 8, hipMemcpyDeviceToHost, g.stream);
        if (se == hipSuccess) se = hipStreamSynchronize(g.stream);
        if (se != hipSuccess) return fail(MHX_E_HIP, "linkage kernel failed: %s", hipGetErrorString(se));
        clock.note(); // the triangle and the steps (the release of the triangle's arrays between them included)
        total += ctl[4];
        g.last_linkage_rescans = total > (unsigned long long)INT_MAX ? INT_MAX : (int)total;
        if (ctl[5]) return fail(MHX_E_INTERNAL, "a linkage step found no pair to merge");
        if (device_ptrs) return MHX_OK;
        rc = read_back("dist_linkage", {{merge_a, a.merge_a, m * 4}, {merge_b, a.merge_b, m * 4}, {size, a.size_out, m * 4}, {num, a.num, m * 8}, {den, a.den, m * 8}});
        if (rc) return rc;
        if (dist)
            for (size_t t = 0; t < m; ++t) dist[t] = link_height(linkage, num[t], den[t], k);
        return MHX_OK;
    });
}
