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

NjStateAt::NjStateAt(Carve &in, uint32_t n)
{
    o_r = in.take((size_t)n * 8);
    for (size_t &o : o_act) o = in.take((size_t)n * 4);
    for (size_t &o : o_pre) o = in.take(((size_t)n + 1) * 8);
    o_cand = in.take((size_t)kNjMaxBlocks * sizeof(NjCand));
    o_ctl = in.take(256);
}
void NjStateAt::place(NjArgs &a, uint8_t *base, uint32_t n, int k) const
{
    a.r = (uint64_t *)(base + o_r);
    for (int i = 0; i < 2; ++i) { a.act[i] = (uint32_t *)(base + o_act[i]); a.pre[i] = (uint64_t *)(base + o_pre[i]); }
    a.cand = (NjCand *)(base + o_cand);
    a.ctl = (uint64_t *)(base + o_ctl);
    a.n = n; a.k = k;
}
NjRecordsAt::NjRecordsAt(Carve &in, uint32_t n, bool wanted)
{
    const size_t m = wanted ? (size_t)n - 1 : 0;
    o_a = in.take(m * 4); o_b = in.take(m * 4);
    o_d = in.take(m * 8); o_ra = in.take(m * 8); o_rb = in.take(m * 8);
}
void NjRecordsAt::place(NjArgs &a, uint8_t *base) const
{
    a.join_a = (uint32_t *)(base + o_a); a.join_b = (uint32_t *)(base + o_b);
    a.d = (uint64_t *)(base + o_d); a.r_a = (uint64_t *)(base + o_ra); a.r_b = (uint64_t *)(base + o_rb);
}

// The dense mode writes the packed common / denom once, the init pass turns them into the pair words and the row sums, and
// every join is a scan of the active rows, the pick by one workgroup and an update by one thread per node.
int nj_tree(const TriCall &c, const NjArgs &a, StoredTriangle &tri, bool release, uint64_t *clamps)
{
    const uint32_t n = c.n;
    int rc = run_dense(c, tri.common, tri.denom, nullptr);
    if (rc) return rc;
    StepsClock clock;
    hipError_t le = launch_nj_init(a, tri.common, tri.denom, g.stream);
    if (release) {
        if (le == hipSuccess && hipStreamSynchronize(g.stream) != hipSuccess) return fail(MHX_E_HIP, "neighbour joining init kernel failed");
        tri.reset();
    }
    // the joins: nothing comes back between them
    for (uint32_t t = 0; t + 1 < n && le == hipSuccess; ++t) {
        if (n - t > 2) le = launch_nj_scan(a, t, g.stream);
        if (le == hipSuccess) le = launch_nj_join(a, t, g.stream);
        if (le == hipSuccess && n - t > 2) le = launch_nj_update(a, t, g.stream);
    }
    if (le != hipSuccess) return fail(MHX_E_HIP, "neighbour joining kernel launch failed: %s", hipGetErrorString(le));
    clock.stop();
    uint64_t ctl[6] = {0, 0, 0, 0, 0, 0};
    hipError_t se = hipMemcpyAsync(ctl, a.ctl, sizeof ctl, hipMemcpyDeviceToHost, g.stream);
    if (se == hipSuccess) se = hipStreamSynchronize(g.stream);
    if (se != hipSuccess) return fail(MHX_E_HIP, "neighbour joining kernel failed: %s", hipGetErrorString(se));
    clock.note(); // the triangle and the joins (the release of the triangle's arrays between them included)
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
        rc = store_fits("MHX_LINKAGE_STORE_MB", n);
        if (rc) return rc;
        Carve in; // staging: the state, host form: the records behind it, then rows and lengths
        const NjStateAt state(in, n);
        const NjRecordsAt records(in, n, !device_ptrs);
        TriCall c;
        uint8_t *base = nullptr;
        rc = stage_rows(rows, len, n, stride, k, s, device_ptrs, in, &base, c);
        if (rc) return rc;
        NjArgs a{};
        state.place(a, base, n, k);
        if (device_ptrs) { a.join_a = join_a; a.join_b = join_b; a.d = d; a.r_a = r_a; a.r_b = r_b; a.len_a = len_a; a.len_b = len_b; }
        else {
            records.place(a, base);
            a.len_a = a.len_b = nullptr; // lengths in host arithmetic below: the same doubles
        }
        StoredTriangle tri; // the words: released when the call returns; the triangle's two arrays: behind the init pass
        rc = tri.alloc((uint64_t)n * (n - 1) / 2, "neighbour joining", true);
        if (rc) return rc;
        a.words = tri.words;
        rc = nj_tree(c, a, tri, true, &g.last_nj_clamps);
        if (rc || device_ptrs) return rc;
        const size_t m = (size_t)n - 1;
        rc = read_back("dist_nj", {{join_a, a.join_a, m * 4}, {join_b, a.join_b, m * 4}, {d, a.d, m * 8}, {r_a, a.r_a, m * 8}, {r_b, a.r_b, m * 8}});
        if (rc) return rc;
        if (len_a)
            for (size_t t = 0; t < m; ++t) nj_lengths(NjRecord{join_a[t], join_b[t], d[t], r_a[t], r_b[t]}, n - (uint32_t)t, len_a[t], len_b[t]);
        return MHX_OK;
    });
}
