// mhx_engine_medoid.cpp -- host side of the medoids of a partition of a sketch set (mhx_dist_medoids) and of the pair of every
// list with a target (mhx_dist_to): the argument checks -- labels and targets are validated on the host in both forms, so
// that no kernel indexes with an unchecked value --, the staging, and the readback.  The block mode itself, run_medoid, is
// the triangle's (mhx_engine_triangle.cpp).
// Rules: mhx_medoid.h; kernels: mhx_medoid.hip and, through the triangle, mhx_triangle.hip and mhx_dist.hip.
#include <hip/hip_runtime.h>

#include <vector>

#include "mhx_device.h"
#include "mhx_medoid.h"
#include "mhx_engine_internal.h"
#include "mhx_engine_triangle.h"
#include "mhx_internal.h"

using namespace mhx;

namespace {

// triangle_check, the tree's bound on s, and for a single list what triangle_check leaves to the pair kernels; *done: n == 0
int medoid_check(const uint64_t *rows, const uint32_t *len, uint32_t n, uint32_t stride, int k, uint32_t s, int device_ptrs, bool *done)
{
    int rc = triangle_check(rows, len, n, stride, k, s, device_ptrs, done);
    if (rc) return rc;
    if (s >= kMstMaxS) return fail(MHX_E_ARG, "sketch size too large for the medoids (%u, below %u)", s, kMstMaxS);
    *done = n == 0;
    if (n != 1) return MHX_OK;
    if (!rows || !len) return fail(MHX_E_ARG, "null argument");
    if (k < 1 || k > 32 || s == 0 || stride == 0) return fail(MHX_E_ARG, "bad k / s / stride");
    if (!device_ptrs && len[0] > stride) return fail(MHX_E_ARG, "len[0] exceeds stride");
    return MHX_OK;
}

// the caller's index array on the host, copied when it lies on the device (4 n bytes, at most 256 KiB)
int host_indices(const uint32_t *v, uint32_t n, int device_ptrs, std::vector<uint32_t> &copy, const uint32_t **out)
{
    *out = v;
    if (!device_ptrs) return MHX_OK;
    copy.resize(n);
    if (hipMemcpy(copy.data(), v, (size_t)n * 4, hipMemcpyDeviceToHost) != hipSuccess) return fail(MHX_E_HIP, "D2H copy of the indices failed");
    *out = copy.data();
    return MHX_OK;
}

} // namespace

extern "C" uint64_t mhx_last_medoid_blocks(void) { return g.last_medoid_blocks; }

// Medoids: the labels are checked on the host, the blocks of the triangle that hold a pair of one cluster add the fixed-point
// distances to sum [n] (run_medoid), a 64-bit minimum per cluster picks the medoid, and the pair kernel compares every list
// with it.  Device memory: 8 n bytes each for the sums and the keys, nothing of size n^2.
extern "C" int mhx_dist_medoids(const uint64_t *rows, const uint32_t *len, uint32_t n, uint32_t stride, int k, uint32_t s, const uint32_t *label,
                                uint32_t *medoid, uint64_t *sum, uint32_t *common, uint32_t *denom, int device_ptrs)
{
    return guarded("mhx_dist_medoids", [&]() -> int {
        bool done;
        int rc = medoid_check(rows, len, n, stride, k, s, device_ptrs, &done);
        if (rc) return rc;
        g.last_medoid_blocks = 0;
        if ((common == nullptr) != (denom == nullptr)) return fail(MHX_E_ARG, "common and denom go together");
        if (done) return MHX_OK;
        if (!label || !medoid) return fail(MHX_E_ARG, "null argument");
        std::vector<uint32_t> copy;
        const uint32_t *h_label;
        rc = host_indices(label, n, device_ptrs, copy, &h_label);
        if (rc) return rc;
        for (uint32_t i = 0; i < n; ++i)
            if (h_label[i] >= n) return fail(MHX_E_ARG, "label[%u] = %u is no index of the set", i, h_label[i]);
        const uint32_t bad = medoid_first_bad_label(h_label, n);
        if (bad < n) return fail(MHX_E_ARG, "label[%u] = %u is not the lowest index of a cluster", bad, h_label[bad]);
        // staging: [sum][best] in 64-bit words, [label][medoid][common][denom], then (host form) rows and lengths
        Carve in;
        const size_t o_sum = in.take((size_t)n * 8), o_best = in.take((size_t)n * 8);
        const size_t o_label = in.take((size_t)n * 4), o_medoid = in.take((size_t)n * 4), o_common = in.take((size_t)n * 4), o_denom = in.take((size_t)n * 4);
        TriCall c;
        uint8_t *base = nullptr;
        rc = stage_rows(rows, len, n, stride, k, s, device_ptrs, in, &base, c);
        if (rc) return rc;
        MedoidRun m{};
        m.h_label = h_label;
        m.sum = (unsigned long long *)(base + o_sum);
        m.best = (unsigned long long *)(base + o_best);
        uint32_t *d_label = (uint32_t *)(base + o_label);
        m.medoid = (uint32_t *)(base + o_medoid);
        if (common) { m.common = (uint32_t *)(base + o_common); m.denom = (uint32_t *)(base + o_denom); }
        if (device_ptrs) {
            m.label = label; m.medoid = medoid;
            if (sum) m.sum = (unsigned long long *)sum;
            if (common) { m.common = common; m.denom = denom; }
        } else {
            if (hipMemcpyAsync(d_label, label, (size_t)n * 4, hipMemcpyHostToDevice, g.stream) != hipSuccess) return fail(MHX_E_HIP, "H2D copy of the labels failed");
            m.label = d_label;
        }
        rc = run_medoid(c, m);
        if (rc || device_ptrs) return rc;
        return read_back("dist_medoids", {{medoid, m.medoid, (size_t)n * 4}, {sum, m.sum, (size_t)n * 8, sum != nullptr},
                                          {common, m.common, (size_t)n * 4, common != nullptr}, {denom, m.denom, (size_t)n * 4, common != nullptr}});
    });
}

// The pair rule of every list with its target: one workgroup per list, no triangle pass.
extern "C" int mhx_dist_to(const uint64_t *rows, const uint32_t *len, uint32_t n, uint32_t stride, int k, uint32_t s, const uint32_t *target,
                           uint32_t *common, uint32_t *denom, int device_ptrs)
{
    return guarded("mhx_dist_to", [&]() -> int {
        bool done;
        int rc = medoid_check(rows, len, n, stride, k, s, device_ptrs, &done);
        if (rc || done) return rc;
        if (!target || !common || !denom) return fail(MHX_E_ARG, "null argument");
        std::vector<uint32_t> copy;
        const uint32_t *h_target;
        rc = host_indices(target, n, device_ptrs, copy, &h_target);
        if (rc) return rc;
        for (uint32_t i = 0; i < n; ++i)
            if (h_target[i] >= n) return fail(MHX_E_ARG, "target[%u] = %u is no index of the set", i, h_target[i]);
        Carve in; // host form: [target][common][denom], then rows and lengths
        const size_t b4 = device_ptrs ? 0 : (size_t)n * 4, o_target = in.take(b4), o_common = in.take(b4), o_denom = in.take(b4);
        TriCall c;
        uint8_t *base = nullptr;
        rc = stage_rows(rows, len, n, stride, k, s, device_ptrs, in, &base, c);
        if (rc) return rc;
        DistToArgs a{c.rows, c.len, n, stride, s, target, common, denom};
        if (!device_ptrs) {
            a.target = (uint32_t *)(base + o_target); a.common = (uint32_t *)(base + o_common); a.denom = (uint32_t *)(base + o_denom);
            if (hipMemcpyAsync((void *)a.target, target, (size_t)n * 4, hipMemcpyHostToDevice, g.stream) != hipSuccess) return fail(MHX_E_HIP, "H2D copy of the targets failed");
        }
        hipEventRecord(g.ev0, g.stream);
        hipError_t le = launch_dist_to(a, g.stream);
        hipEventRecord(g.ev1, g.stream);
        if (le != hipSuccess) return fail(MHX_E_HIP, "pair kernel launch failed: %s", hipGetErrorString(le));
        if (hipStreamSynchronize(g.stream) != hipSuccess) return fail(MHX_E_HIP, "pair kernel failed");
        float ms = 0.f;
        hipEventElapsedTime(&ms, g.ev0, g.ev1);
        g.last_dist_ms = ms;
        if (device_ptrs) return MHX_OK;
        return read_back("dist_to", {{common, a.common, b4}, {denom, a.denom, b4}});
    });
}
