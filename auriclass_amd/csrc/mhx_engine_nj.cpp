// mhx_engine_nj.cpp -- host side of neighbour joining over a sketch set (mhx_dist_nj): the packed triangle of the dense mode
// computed once, the init pass that turns it into one distance word per pair and the first row sums, the n - 1 joins of three
// launches each, enqueued without a readback between them, and the branch lengths on the host.  Everything behind "the rows
// are staged" is nj_tree (mhx_engine_nj.h), which the jackknife (mhx_engine_resample.cpp) runs once per replicate.
// Rules: mhx_nj.h; kernels: mhx_nj.hip and, through the triangle, mhx_triangle.hip and mhx_dist.hip.
#include <hip/hip_runtime.h>
#include <stdlib.h>

#include "mhx_device.h"
#include "mhx_nj.h"
#include "mhx_triangle.h"
#include "mhx_engine_internal.h"
#include "mhx_engine_nj.h"
#include "mhx_engine_triangle.h"
#include "mhx_internal.h"

using namespace mhx;

extern "C" uint64_t mhx_last_nj_clamps(void) { return g.last_nj_clamps; }

namespace mhx {

int nj_check(const uint64_t *rows, const uint32_t *len, uint32_t n, uint32_t stride, int k, uint32_t s, int device_ptrs, bool *done)
{
    const int rc = triangle_check(rows, len, n, stride, k, s, device_ptrs, done);
    if (rc) return rc;
    if (s >= kMstMaxS) return fail(MHX_E_ARG, "sketch size too large for neighbour joining (%u, below %u)", s, kMstMaxS);
    return MHX_OK;
}

int nj_budget(uint32_t n)
{
    const uint64_t pairs = (uint64_t)n * (n - 1) / 2;
    uint64_t budget_mb = 4096;
    if (const char *e = getenv("MHX_LINKAGE_STORE_MB")) { const long long v = atoll(e); if (v >= 0) budget_mb = (uint64_t)v; }
    if (8 * pairs > budget_mb << 20)
        return fail(MHX_E_CAPACITY, "the pair words of %u lists (%llu bytes) do not fit MHX_LINKAGE_STORE_MB = %llu", n, (unsigned long long)(8 * pairs),
                    (unsigned long long)budget_mb);
    return MHX_OK;
}

size_t nj_state_bytes(uint32_t n)
{
    return up256((size_t)n * 8) + 2 * up256((size_t)n * 4) + 2 * up256(((size_t)n + 1) * 8) + up256((size_t)kNjMaxBlocks * sizeof(NjCand)) + 256;
}
size_t nj_records_bytes(uint32_t n) { return 2 * up256(((size_t)n - 1) * 4) + 3 * up256(((size_t)n - 1) * 8); }

void nj_place_state(NjArgs &a, uint8_t *at, uint32_t n, int k)
{
    const size_t bn = up256((size_t)n * 4), bn8 = up256((size_t)n * 8), bp8 = up256(((size_t)n + 1) * 8), bc = up256((size_t)kNjMaxBlocks * sizeof(NjCand));
    a.r = (uint64_t *)at;
    a.act[0] = (uint32_t *)(at + bn8); a.act[1] = (uint32_t *)(at + bn8 + bn);
    a.pre[0] = (uint64_t *)(at + bn8 + 2 * bn); a.pre[1] = (uint64_t *)(at + bn8 + 2 * bn + bp8);
    a.cand = (NjCand *)(at + bn8 + 2 * bn + 2 * bp8);
    a.ctl = (uint64_t *)(at + bn8 + 2 * bn + 2 * bp8 + bc);
    a.n = n; a.k = k;
}
void nj_place_records(NjArgs &a, uint8_t *at, uint32_t n)
{
    const size_t be = up256(((size_t)n - 1) * 4), be8 = up256(((size_t)n - 1) * 8);
    a.join_a = (uint32_t *)at; a.join_b = (uint32_t *)(at + be);
    a.d = (uint64_t *)(at + 2 * be); a.r_a = (uint64_t *)(at + 2 * be + be8); a.r_b = (uint64_t *)(at + 2 * be + 2 * be8);
}

// The dense mode writes the packed common / denom once, the init pass turns them into the pair words and the row sums, and
// every join is a scan of the active rows, the pick by one workgroup and an update by one thread per node.
int nj_tree(const TriCall &c, const NjArgs &a, uint32_t *p_common, uint32_t *p_denom, DevArray<uint8_t> *release, uint64_t *clamps)
{
    const uint32_t n = c.n;
    int rc = run_dense(c, p_common, p_denom, nullptr);
    if (rc) return rc;
    const double tri_ms = g.last_dist_ms;
    hipEventRecord(g.ev0, g.stream);
    hipError_t le = launch_nj_init(a, p_common, p_denom, g.stream);
    if (release) {
        if (le == hipSuccess && hipStreamSynchronize(g.stream) != hipSuccess) return fail(MHX_E_HIP, "neighbour joining init kernel failed");
        release->reset();
    }
    // the joins: nothing comes back between them
    for (uint32_t t = 0; t + 1 < n && le == hipSuccess; ++t) {
        if (n - t > 2) le = launch_nj_scan(a, t, g.stream);
        if (le == hipSuccess) le = launch_nj_join(a, t, g.stream);
        if (le == hipSuccess && n - t > 2) le = launch_nj_update(a, t, g.stream);
    }
    if (le != hipSuccess) return fail(MHX_E_HIP, "neighbour joining kernel launch failed: %s", hipGetErrorString(le));
    hipEventRecord(g.ev1, g.stream);
    uint64_t ctl[6] = {0, 0, 0, 0, 0, 0};
    hipError_t se = hipMemcpyAsync(ctl, a.ctl, sizeof ctl, hipMemcpyDeviceToHost, g.stream);
    if (se == hipSuccess) se = hipStreamSynchronize(g.stream);
    if (se != hipSuccess) return fail(MHX_E_HIP, "neighbour joining kernel failed: %s", hipGetErrorString(se));
    float ms = 0.f;
    hipEventElapsedTime(&ms, g.ev0, g.ev1);
    g.last_dist_ms = tri_ms + ms; // the triangle and the joins (the release of the triangle's arrays between them included)
    *clamps = ctl[4];
    if (ctl[5]) return fail(MHX_E_INTERNAL, "a join of neighbour joining found no pair");
    return MHX_OK;
}

} // namespace mhx

// Neighbour joining: one tree (nj_tree) of the staged rows.
// Device memory of size n^2: 8 n (n - 1) / 2 bytes of words for the whole call, and as many again for the triangle's two arrays
// until the init pass has read them (peak 16 n (n - 1) / 2 bytes); the words must fit MHX_LINKAGE_STORE_MB.
extern "C" int mhx_dist_nj(const uint64_t *rows, const uint32_t *len, uint32_t n, uint32_t stride, int k, uint32_t s, uint32_t *join_a, uint32_t *join_b,
                           uint64_t *d, uint64_t *r_a, uint64_t *r_b, double *len_a, double *len_b, int device_ptrs)
{
    return guarded("mhx_dist_nj", [&]() -> int {
        g.last_nj_clamps = 0;
        bool done;
        int rc = nj_check(rows, len, n, stride, k, s, device_ptrs, &done);
        if (rc) return rc;
        if (done) return MHX_OK; // no pair, no join
        if (!join_a || !join_b || !d || !r_a || !r_b || !len_a != !len_b) return fail(MHX_E_ARG, "null argument");
        rc = nj_budget(n);
        if (rc) return rc;
        const uint64_t pairs = (uint64_t)n * (n - 1) / 2;
        // staging: the state, host form: the records behind it, then rows and lengths
        const size_t state = nj_state_bytes(n);
        TriCall c;
        uint8_t *base = nullptr;
        rc = stage_rows(rows, len, n, stride, k, s, device_ptrs, device_ptrs ? state : state + nj_records_bytes(n), &base, c);
        if (rc) return rc;
        NjArgs a{};
        nj_place_state(a, base, n, k);
        if (device_ptrs) { a.join_a = join_a; a.join_b = join_b; a.d = d; a.r_a = r_a; a.r_b = r_b; a.len_a = len_a; a.len_b = len_b; }
        else {
            nj_place_records(a, base + state, n);
            a.len_a = a.len_b = nullptr; // lengths in host arithmetic below: the same doubles
        }
        DevArray<uint64_t> words; // released when the call returns
        DevArray<uint8_t> packed; // the triangle's two arrays: released behind the init pass
        const size_t bp = up256((size_t)pairs * 4);
        if (words.grow(pairs, g.stream) != hipSuccess) return fail(MHX_E_HIP, "hipMalloc failed for the pair words of neighbour joining (%llu bytes)", (unsigned long long)(8 * pairs));
        if (packed.grow(2 * bp, g.stream) != hipSuccess) return fail(MHX_E_HIP, "hipMalloc failed for the stored pairs of neighbour joining (%zu bytes)", 2 * bp);
        a.words = words;
        uint32_t *p_common = (uint32_t *)(uint8_t *)packed, *p_denom = (uint32_t *)((uint8_t *)packed + bp);
        rc = nj_tree(c, a, p_common, p_denom, &packed, &g.last_nj_clamps);
        if (rc) return rc;
        if (device_ptrs) return MHX_OK;
        const size_t m = (size_t)n - 1;
        if (hipMemcpy(join_a, a.join_a, m * 4, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(join_b, a.join_b, m * 4, hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(d, a.d, m * 8, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(r_a, a.r_a, m * 8, hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(r_b, a.r_b, m * 8, hipMemcpyDeviceToHost) != hipSuccess)
            return fail(MHX_E_HIP, "D2H copy failed in dist_nj");
        if (len_a)
            for (size_t t = 0; t < m; ++t) nj_lengths(NjRecord{join_a[t], join_b[t], d[t], r_a[t], r_b[t]}, n - (uint32_t)t, len_a[t], len_b[t]);
        return MHX_OK;
    });
}
