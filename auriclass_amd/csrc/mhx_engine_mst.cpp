// mhx_engine_mst.cpp -- host side of the single-linkage tree of a sketch set (mhx_dist_mst): the state of a call between
// its Boruvka rounds, the steps of a round around the proposals of either pair source, the order of the edges on the
// host, and the cut of a finished tree (mhx_mst_labels).  The pairs come from mhx_engine_triangle.cpp.
// Rules: mhx_mst.h; kernels: mhx_mst.hip, mhx_cluster.hip and, through the triangle, mhx_triangle.hip and mhx_dist.hip.
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <numeric>
#include <vector>

#include "mhx_device.h"
#include "mhx_cluster.h"
#include "mhx_mst.h"
#include "mhx_triangle.h"
#include "mhx_engine_internal.h"
#include "mhx_engine_triangle.h"
#include "mhx_internal.h"

using namespace mhx;

namespace {

// every list its own component, no edge yet
hipError_t mst_begin(MstRun &m)
{
    m.components = m.n; m.rounds = 0; m.appended = 0;
    hipError_t e = hipMemsetAsync(m.counters, 0, 16, g.stream);
    if (e == hipSuccess) e = launch_cluster_init(m.parent, nullptr, m.n, g.stream);
    if (e == hipSuccess) e = hipMemcpyAsync(m.comp, m.parent, (size_t)m.n * 4, hipMemcpyDeviceToDevice, g.stream);
    return e;
}

} // namespace

namespace mhx {

// step 1; the proposals of step 2 follow, from either pair source
hipError_t mst_round_open(MstRun &m)
{
    const hipError_t e = hipMemsetAsync(m.counters + 1, 0, 8, g.stream);
    return e != hipSuccess ? e : launch_mst_reset(m.best, m.winner, m.n, g.stream);
}
// steps 3 to 5 and the one small readback of a round.  comp is a copy of the flattened parent: the hooks of the next round
// move roots of parent while others still ask which component a list was in.
int mst_round_close(MstRun &m)
{
    hipError_t e = launch_mst_choose(m.best, m.comp, m.winner, m.n, g.stream);
    MstHookArgs h{};
    h.comp = m.comp; h.winner = m.winner; h.best = m.best; h.parent = m.parent; h.n = m.n; h.k = m.k;
    h.edge_i = m.edge_i; h.edge_j = m.edge_j; h.common = m.common; h.denom = m.denom; h.dist = m.dist;
    h.n_edges = m.counters; h.cap = (uint64_t)m.n - 1;
    if (e == hipSuccess) e = launch_mst_hook(h, g.stream);
    if (e == hipSuccess) e = launch_cluster_flatten(m.parent, m.n, m.counters + 1, g.stream);
    if (e == hipSuccess) e = hipMemcpyAsync(m.comp, m.parent, (size_t)m.n * 4, hipMemcpyDeviceToDevice, g.stream);
    unsigned long long back[2] = {0, 0};
    if (e == hipSuccess) e = hipMemcpyAsync(back, m.counters, 16, hipMemcpyDeviceToHost, g.stream);
    if (e == hipSuccess) e = hipStreamSynchronize(g.stream);
    if (e != hipSuccess) return fail(MHX_E_HIP, "tree round failed: %s", hipGetErrorString(e));
    ++m.rounds;
    // a strict total order leaves mutual picks as the only cycles: every appended edge costs exactly one component
    if (back[1] == 0 || back[1] > m.components || back[0] - m.appended != (uint64_t)m.components - back[1])
        return fail(MHX_E_INTERNAL, "tree round %u: %llu edges appended, components %u -> %llu", m.rounds, back[0] - (unsigned long long)m.appended,
                    m.components, back[1]);
    if (back[1] == m.components) return fail(MHX_E_INTERNAL, "tree round %u joined nothing (%u components)", m.rounds, m.components);
    m.appended = back[0];
    m.components = (uint32_t)back[1];
    return MHX_OK;
}

} // namespace mhx

extern "C" int mhx_last_mst_rounds(void) { return g.last_mst_rounds; }
extern "C" int mhx_last_mst_stored(void) { return g.last_mst_stored; }

// the cut of a finished tree (mhx_mst.h: mst_labels): host arithmetic only, no engine needed
extern "C" int mhx_mst_labels(const uint32_t *edge_i, const uint32_t *edge_j, const uint32_t *common, const uint32_t *denom, uint32_t n, int k,
                              double max_dist, uint32_t *label, uint32_t *n_clusters)
{
    clear_error();
    if (n_clusters) *n_clusters = 0;
    if (!n_clusters || (n && !label) || (n > 1 && (!edge_i || !edge_j || !common || !denom))) return fail(MHX_E_ARG, "null argument");
    if (k < 1 || k > 32) return fail(MHX_E_ARG, "bad k");
    if (!(max_dist == max_dist)) return fail(MHX_E_ARG, "max_dist is not a number");
    for (uint32_t e = 0; e + 1 < n; ++e)
        if (edge_i[e] >= n || edge_j[e] >= n) return fail(MHX_E_ARG, "edge %u names a list outside 0 .. %u", e, n - 1);
    *n_clusters = mst_labels(edge_i, edge_j, common, denom, n, k, max_dist, label);
    return MHX_OK;
}

// Single-linkage tree: Boruvka rounds over best / winner / parent (mhx_mst.h).  The pairs of a round come from the packed
// triangle, written once by the dense mode (stored: the only thing of size n^2 this call ever holds, and only when it fits
// the budget), or from the triangle's blocks run again every round (recomputed: O(n) workspace).
extern "C" int mhx_dist_mst(const uint64_t *rows, const uint32_t *len, uint32_t n, uint32_t stride, int k, uint32_t s, uint32_t *edge_i, uint32_t *edge_j,
                            uint32_t *common, uint32_t *denom, double *dist, int device_ptrs)
{
    return guarded("mhx_dist_mst", [&]() -> int {
        g.last_mst_rounds = 0;
        g.last_mst_stored = -1;
        bool done;
        int rc = triangle_check(rows, len, n, stride, k, s, device_ptrs, &done);
        if (rc) return rc;
        if (s >= kMstMaxS) return fail(MHX_E_ARG, "sketch size too large for the tree (%u, below %u)", s, kMstMaxS);
        if (done) return MHX_OK; // no pair, no edge
        if (!edge_i || !edge_j || !common || !denom) return fail(MHX_E_ARG, "null argument");
        const uint64_t pairs = (uint64_t)n * (n - 1) / 2;
        bool stored = 8 * pairs <= store_budget_mb("MHX_MST_STORE_MB") << 20;
        if (const char *e = getenv("MHX_MST_STORE")) stored = strcmp(e, "0") != 0;
        // staging: [best][winner][parent][comp][counters], host form: [the four edge arrays], then rows and lengths
        const size_t e_n = (size_t)n - 1;
        Carve in;
        const size_t o_best = in.take((size_t)n * 8), o_winner = in.take((size_t)n * 4), o_parent = in.take((size_t)n * 4), o_comp = in.take((size_t)n * 4);
        const size_t o_counters = in.take(16);
        const size_t o_i = in.take(device_ptrs ? 0 : e_n * 4), o_j = in.take(device_ptrs ? 0 : e_n * 4);
        const size_t o_common = in.take(device_ptrs ? 0 : e_n * 4), o_denom = in.take(device_ptrs ? 0 : e_n * 4);
        TriCall c;
        uint8_t *base = nullptr;
        rc = stage_rows(rows, len, n, stride, k, s, device_ptrs, in, &base, c);
        if (rc) return rc;
        MstRun m{};
        m.best = (uint64_t *)(base + o_best);
        m.winner = (uint32_t *)(base + o_winner); m.parent = (uint32_t *)(base + o_parent); m.comp = (uint32_t *)(base + o_comp);
        m.counters = (unsigned long long *)(base + o_counters);
        m.n = n; m.k = k;
        if (device_ptrs) { m.edge_i = edge_i; m.edge_j = edge_j; m.common = common; m.denom = denom; m.dist = dist; }
        else {
            m.edge_i = (uint32_t *)(base + o_i); m.edge_j = (uint32_t *)(base + o_j); m.common = (uint32_t *)(base + o_common); m.denom = (uint32_t *)(base + o_denom);
            m.dist = nullptr; // distances in host libm below
        }
        if (stored) {
            StoredTriangle tri; // released when the call returns
            rc = tri.alloc(pairs, "the tree", false);
            if (rc == MHX_OK) rc = run_dense(c, tri.common, tri.denom, nullptr);
            if (rc) return rc;
            MstScan sc{};
            sc.common = tri.common; sc.denom = tri.denom; sc.n = n; sc.comp = m.comp; sc.best = m.best;
            StepsClock clock;
            hipError_t le = mst_begin(m);
            rc = mst_rounds(m, le, [&](uint32_t) { le = launch_mst_scan(sc, g.stream); return MHX_OK; });
            if (rc) return rc;
            if (le != hipSuccess) return fail(MHX_E_HIP, "tree kernel launch failed: %s", hipGetErrorString(le));
            clock.stop();
            if (hipStreamSynchronize(g.stream) != hipSuccess) return fail(MHX_E_HIP, "tree kernel failed");
            clock.note(); // the triangle and the rounds; the recomputed source: the whole call
        } else {
            const hipError_t le = mst_begin(m);
            if (le != hipSuccess) return fail(MHX_E_HIP, "tree kernel launch failed: %s", hipGetErrorString(le));
            rc = run_mst_recomputed(c, m);
            if (rc) return rc;
        }
        g.last_mst_rounds = (int)m.rounds;
        g.last_mst_stored = stored ? 1 : 0;
        if (m.components != 1 || m.appended != (uint64_t)n - 1) return fail(MHX_E_INTERNAL, "the tree has %llu edges for %u lists", (unsigned long long)m.appended, n);
        if (device_ptrs) return MHX_OK; // the edges lie where the caller wants them, in the order of arrival
        std::vector<uint32_t> ei(e_n), ej(e_n), ec(e_n), ed(e_n);
        rc = read_back("dist_mst", {{ei.data(), m.edge_i, e_n * 4}, {ej.data(), m.edge_j, e_n * 4}, {ec.data(), m.common, e_n * 4}, {ed.data(), m.denom, e_n * 4}});
        if (rc) return rc;
        // the edge order: the merge order of the dendrogram
        std::vector<size_t> order(e_n);
        std::iota(order.begin(), order.end(), (size_t)0);
        std::sort(order.begin(), order.end(), [&](size_t a, size_t b) { return mst_precedes(mst_edge(ec[a], ed[a], ei[a], ej[a]), mst_edge(ec[b], ed[b], ei[b], ej[b])); });
        for (size_t t = 0; t < e_n; ++t) {
            const size_t e = order[t];
            edge_i[t] = ei[e]; edge_j[t] = ej[e]; common[t] = ec[e]; denom[t] = ed[e];
            if (dist) dist[t] = tri_distance(ec[e], ed[e], k);
        }
        return MHX_OK;
    });
}

