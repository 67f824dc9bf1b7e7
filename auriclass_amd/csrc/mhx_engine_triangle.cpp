// mhx_engine_triangle.cpp -- host side of the all-pairs distance within one sketch set (mhx_dist_triangle,
// mhx_dist_triangle_edges, mhx_dist_cluster and mhx_dist_mst): staging of a host-pointer call, the schedule of (query batch, reference
// slice) blocks over ONE offsets table of the whole set, the fallback of a flagged block to the generic pair kernel, the
// exact distance rule and the order of the edge list on the host, the bound of the clustering as a table of integers, and
// the rounds of the single-linkage tree.
// Rules: mhx_triangle.h, mhx_cluster.h, mhx_mst.h; kernels: mhx_triangle.hip, mhx_cluster.hip, mhx_mst.hip and mhx_dist.hip.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <exception>
#include <new>
#include <numeric>
#include <vector>

#include "mhx_device.h"
#include "mhx_cluster.h"
#include "mhx_mst.h"
#include "mhx_triangle.h"
#include "mhx_engine_internal.h"
#include "mhx_internal.h"

using namespace mhx;

namespace {

// The state of a single-linkage tree call (mhx_mst.h) between its rounds, everything on the device: what the five steps of
// a round read and write, and the counters that come back once per round.
struct MstRun {
    uint64_t *best; // [n]
    uint32_t *winner, *parent, *comp; // [n] each
    unsigned long long *counters; // [0] edges appended so far, [1] roots of the last flatten pass
    uint32_t *edge_i, *edge_j, *common, *denom; // [n - 1] the result
    double *dist;             // may be null
    uint32_t n;
    int k;
    uint32_t components, rounds; // host: after the last round closed
    uint64_t appended;
};

// every list its own component, no edge yet
hipError_t mst_begin(MstRun &m)
{
    m.components = m.n; m.rounds = 0; m.appended = 0;
    hipError_t e = hipMemsetAsync(m.counters, 0, 16, g.stream);
    if (e == hipSuccess) e = launch_cluster_init(m.parent, nullptr, m.n, g.stream);
    if (e == hipSuccess) e = hipMemcpyAsync(m.comp, m.parent, (size_t)m.n * 4, hipMemcpyDeviceToDevice, g.stream);
    return e;
}
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

struct TriCall { // everything on the device
    const uint64_t *rows;
    const uint32_t *len;
    uint32_t n, stride, s, longest;
    int k;
    bool edges;
    uint32_t *common, *denom; // dense: packed triangle; edges: [cap]
    double *dist;             // may be null
    uint32_t *edge_i, *edge_j;
    uint64_t cap;
    double jmin;
    uint64_t found; // out, edge mode: pairs that passed the prefilter; cluster mode: the edges
    // cluster mode (mhx_cluster.h): the pairs feed a union-find over parent [n] instead of an output of pairs
    bool cluster;
    const uint32_t *h_cmin; // host, [s + 1]: copied into the workspace
    uint32_t *parent, *degree; // degree may be null
    uint32_t clusters;      // out
    // tree mode (mhx_mst.h), recomputed pair source: the blocks run once per round and propose to mst->best; the offsets
    // table is built once.  The caller has run mst_begin.
    MstRun *mst;
};

size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

// Launches the whole call on the engine's stream and waits for it.  The set's lists are split into value ranges ONCE
// (launch_dist_offsets over all n lists); every block then runs the range pass and a finish pass into its block-local
// [queries][32] results, and the scatter or the edge pass takes the pairs that count from there.  Block flags come back
// once per group of blocks; a flagged block is redone by the generic pair kernel into the same block-local arrays.
int triangle_device(TriCall &c)
{
    const uint64_t pairs = (uint64_t)c.n * (c.n - 1) / 2;
    const char *geo = getenv("MHX_TRI_GEOMETRY");
    const uint32_t ranges = geo && strcmp(geo, "dist") == 0 ? tri_ranges_dist(c.longest) : tri_ranges(c.longest);
    const bool fast = (pairs >= 64 || (pairs >= 8 && pairs * (uint64_t)c.s >= 400000)) && ranges != 0 && getenv("MHX_DIST_GENERIC") == nullptr;
    uint32_t qbatch = tri_max_queries(fast ? ranges : kTriMinRanges);
    if (const char *e = getenv("MHX_TRI_QBATCH")) { const long v = atol(e); if (v > 0 && (uint64_t)v < qbatch) qbatch = (uint32_t)v; }
    qbatch = std::min(qbatch, c.n);
    std::vector<TriBlock> blocks;
    {
        TriBlock b;
        for (bool more = tri_first_block(c.n, qbatch, b); more; more = tri_next_block(c.n, qbatch, b)) blocks.push_back(b);
    }
    const uint32_t nblocks = (uint32_t)blocks.size();
    constexpr uint32_t kBlockGroup = 4096; // blocks whose flag words come back together
    const uint32_t group = std::min(nblocks, kBlockGroup);
    // workspace: [offsets of the set][byte counters][window totals][block-local common, denom][words: shift, 0, the edge
    // counter (two words), then two per block of a group][cluster mode: the root counter, the cmin table]
    const uint64_t per = (uint64_t)ranges + 1;
    size_t o = 0;
    const size_t o_offs = o; if (fast) o += up256((size_t)c.n * per * 4);
    const size_t o_cpart = o; if (fast) o += up256((size_t)qbatch * ranges * kTriSlice);
    const size_t o_wtot = o; if (fast && ranges > (uint32_t)kDistRanges) o += up256((size_t)qbatch * (ranges / kDistWindowRanges) * kTriSlice * 4);
    const size_t o_lc = o; o += up256((size_t)qbatch * kTriSlice * 4);
    const size_t o_ld = o; o += up256((size_t)qbatch * kTriSlice * 4);
    const size_t o_words = o; o += up256((size_t)(4 + 2 * group) * 4);
    const size_t o_roots = o; if (c.cluster) o += 256;
    const size_t o_cmin = o; if (c.cluster) o += up256(((size_t)c.s + 1) * 4);
    if (g.dist_ws.grow(o, g.stream) != hipSuccess) return fail(MHX_E_HIP, "hipMalloc failed for the triangle workspace (%zu bytes)", o);
    uint32_t *offs = (uint32_t *)(g.dist_ws + o_offs), *loc_c = (uint32_t *)(g.dist_ws + o_lc), *loc_d = (uint32_t *)(g.dist_ws + o_ld);
    uint32_t *words = (uint32_t *)(g.dist_ws + o_words), *flags = words + 4;
    unsigned long long *counter = (unsigned long long *)(words + 2), *roots = (unsigned long long *)(g.dist_ws + o_roots);
    uint32_t *cmin = (uint32_t *)(g.dist_ws + o_cmin);
    DistWork w{};
    w.cpart = g.dist_ws + o_cpart;
    w.wtot = (uint32_t *)(g.dist_ws + o_wtot);
    w.ranges = ranges;
    DistArgs all{};
    all.q = c.rows; all.q_len = c.len; all.nq = c.n; all.nr = 0; all.stride = c.stride; all.s = c.s; all.k = c.k;
    auto block_args = [&](const TriBlock &b) {
        DistArgs x = all;
        x.q = c.rows + (uint64_t)b.q0 * c.stride; x.q_len = c.len + b.q0; x.nq = b.nq;
        x.r = c.rows + (uint64_t)b.r0 * c.stride; x.r_len = c.len + b.r0; x.nr = b.nr;
        x.common = loc_c; x.denom = loc_d; x.dist = nullptr; x.out_stride = kTriSlice; x.out_off = 0;
        return x;
    };
    auto take_out = [&](const TriBlock &b, const uint32_t *flag) {
        if (c.mst) {
            MstOut t{};
            t.loc_common = loc_c; t.loc_denom = loc_d; t.flag = flag;
            t.r0 = b.r0; t.nr = b.nr; t.q0 = b.q0; t.nq = b.nq;
            t.comp = c.mst->comp; t.best = c.mst->best;
            return launch_tri_mst(t, g.stream);
        }
        if (c.cluster) {
            ClusterOut t{};
            t.loc_common = loc_c; t.loc_denom = loc_d; t.flag = flag;
            t.r0 = b.r0; t.nr = b.nr; t.q0 = b.q0; t.nq = b.nq;
            t.cmin = cmin; t.s = c.s; t.parent = c.parent; t.degree = c.degree; t.n_edges = counter;
            return launch_tri_cluster(t, g.stream);
        }
        TriOut t{};
        t.loc_common = loc_c; t.loc_denom = loc_d; t.flag = flag;
        t.r0 = b.r0; t.nr = b.nr; t.q0 = b.q0; t.nq = b.nq; t.k = c.k;
        t.common = c.common; t.denom = c.denom; t.dist = c.dist;
        t.edge_i = c.edge_i; t.edge_j = c.edge_j; t.count = counter; t.cap = c.cap; t.jmin = c.jmin;
        return c.edges ? launch_tri_edges(t, g.stream) : launch_tri_scatter(t, g.stream);
    };
    hipEventRecord(g.ev0, g.stream);
    hipError_t le = hipMemsetAsync(words, 0, (size_t)(4 + 2 * group) * 4, g.stream);
    g.last_dist_fallbacks = fast ? 0 : -1;
    g.last_dist_ranges = 0;
    if (c.cluster && le == hipSuccess) le = hipMemsetAsync(roots, 0, 8, g.stream);
    if (c.cluster && le == hipSuccess) le = hipMemcpyAsync(cmin, c.h_cmin, ((size_t)c.s + 1) * 4, hipMemcpyHostToDevice, g.stream);
    if (c.cluster && le == hipSuccess) le = launch_cluster_init(c.parent, c.degree, c.n, g.stream);
    if (fast && le == hipSuccess) {
        DistWork wa = w;
        wa.offs_q = offs; wa.offs_r = offs; wa.params = words; // words[0] the shift of the call, words[1] stays 0
        le = launch_dist_offsets(all, wa, g.stream);
    }
    // every block once: range, finish and take-out pass, the flagged ones again through the generic kernel.  first: the flag
    // words are still zero and the fallbacks are counted (tree mode runs the blocks once per round)
    auto all_blocks = [&](bool first) -> int {
        for (uint32_t b0 = 0; b0 < nblocks && le == hipSuccess; b0 += kBlockGroup) {
            const uint32_t b1 = std::min(nblocks, b0 + kBlockGroup);
            if (b0 != 0 || !first) le = hipMemsetAsync(flags, 0, (size_t)2 * group * 4, g.stream);
            for (uint32_t b = b0; b < b1 && le == hipSuccess; ++b) {
                const TriBlock &blk = blocks[b];
                const DistArgs x = block_args(blk);
                if (!fast) {
                    le = launch_dist_pairs(x, g.stream);
                    if (le == hipSuccess) le = take_out(blk, words + 1);
                    continue;
                }
                w.offs_q = offs + (uint64_t)blk.q0 * per;
                w.offs_r = offs + (uint64_t)blk.r0 * per;
                w.params = flags + 2 * (b - b0);
                le = launch_dist_range_pass(x, w, g.stream);
                if (le == hipSuccess) le = ranges < (uint32_t)kDistRanges ? launch_tri_finish_small(x, w, g.stream) : launch_dist_finish(x, w, g.stream);
                if (le == hipSuccess) le = take_out(blk, w.params + 1);
                // cluster mode: the trees stay shallow when every reference slice ends with a flatten pass
                if (c.cluster && le == hipSuccess && (b + 1 == b1 || blocks[b + 1].r0 != blk.r0)) le = launch_cluster_flatten(c.parent, c.n, nullptr, g.stream);
            }
            if (!fast || le != hipSuccess) continue;
            std::vector<uint32_t> back((size_t)(b1 - b0) * 2);
            if (hipMemcpyAsync(back.data(), flags, back.size() * 4, hipMemcpyDeviceToHost, g.stream) != hipSuccess ||
                hipStreamSynchronize(g.stream) != hipSuccess)
                return fail(MHX_E_HIP, "triangle kernel failed");
            for (uint32_t b = b0; b < b1 && le == hipSuccess; ++b)
                if (back[2 * (b - b0) + 1]) { // a value range overflowed the LDS table or the byte counters
                    le = launch_dist_pairs(block_args(blocks[b]), g.stream);
                    if (le == hipSuccess) le = take_out(blocks[b], words + 1);
                    if (first) ++g.last_dist_fallbacks;
                }
        }
        return MHX_OK;
    };
    if (!c.mst && le == hipSuccess) {
        const int rc = all_blocks(true);
        if (rc) return rc;
    }
    // tree mode: a round opens, the blocks propose, the round closes -- until one component is left (mst_max_rounds bounds it)
    for (uint32_t round = 0; c.mst && le == hipSuccess; ++round) {
        if (round == mst_max_rounds(c.n)) return fail(MHX_E_INTERNAL, "the tree is not finished after %u rounds (%u components)", round, c.mst->components);
        le = mst_round_open(*c.mst);
        int rc = le == hipSuccess ? all_blocks(round == 0) : MHX_OK;
        if (rc == MHX_OK && le == hipSuccess) rc = mst_round_close(*c.mst);
        if (rc) return rc;
        if (c.mst->components == 1) break;
    }
    if (c.cluster && le == hipSuccess) le = launch_cluster_flatten(c.parent, c.n, roots, g.stream); // behind the last block: the labels
    hipEventRecord(g.ev1, g.stream);
    if (fast && (uint32_t)g.last_dist_fallbacks < nblocks) g.last_dist_ranges = (int)ranges;
    if (le != hipSuccess) return fail(MHX_E_HIP, "triangle kernel launch failed: %s", hipGetErrorString(le));
    unsigned long long found = 0, nroots = 0;
    hipError_t se = hipSuccess;
    if (c.edges || c.cluster) se = hipMemcpyAsync(&found, counter, 8, hipMemcpyDeviceToHost, g.stream);
    if (c.cluster && se == hipSuccess) se = hipMemcpyAsync(&nroots, roots, 8, hipMemcpyDeviceToHost, g.stream);
    if (se == hipSuccess) se = hipStreamSynchronize(g.stream);
    float ms = 0.f;
    hipEventElapsedTime(&ms, g.ev0, g.ev1);
    g.last_dist_ms = ms;
    if (se != hipSuccess) return fail(MHX_E_HIP, "triangle kernel failed: %s", hipGetErrorString(se));
    c.found = found;
    c.clusters = (uint32_t)nroots;
    return MHX_OK;
}

// what all calls check first; *done: nothing to compute (n <= 1)
int triangle_check(const uint64_t *rows, const uint32_t *len, uint32_t n, uint32_t stride, int k, uint32_t s, int device_ptrs, bool *done)
{
    clear_error();
    *done = false;
    const int rc = require_engine();
    if (rc) return rc;
    if (n <= 1) { *done = true; return MHX_OK; }
    if (n > kTriMaxLists) return fail(MHX_E_ARG, "too many lists for one triangle (%u, at most %u)", n, kTriMaxLists);
    if (!rows || !len) return fail(MHX_E_ARG, "null argument");
    if (k < 1 || k > 32 || s == 0 || stride == 0) return fail(MHX_E_ARG, "bad k / s / stride");
    if (!device_ptrs)
        for (uint32_t i = 0; i < n; ++i) if (len[i] > stride) return fail(MHX_E_ARG, "len[%u] exceeds stride", i);
    return MHX_OK;
}

// rows and lengths of a host-pointer call behind `extra` bytes of the staging area
int stage_rows(const uint64_t *rows, const uint32_t *len, uint32_t n, uint32_t stride, size_t extra, uint8_t **base, TriCall &c)
{
    const size_t br = up256((size_t)n * stride * 8), bl = up256((size_t)n * 4);
    const int rc = dist_stage(up256(extra) + br + bl, base);
    if (rc) return rc;
    uint8_t *dr = *base + up256(extra), *dl = dr + br;
    hipError_t ce = hipMemcpyAsync(dr, rows, (size_t)n * stride * 8, hipMemcpyHostToDevice, g.stream);
    if (ce == hipSuccess) ce = hipMemcpyAsync(dl, len, (size_t)n * 4, hipMemcpyHostToDevice, g.stream);
    if (ce != hipSuccess) return fail(MHX_E_HIP, "H2D copy failed in dist_triangle: %s", hipGetErrorString(ce));
    c.rows = (const uint64_t *)dr;
    c.len = (const uint32_t *)dl;
    c.longest = 0;
    for (uint32_t i = 0; i < n; ++i) c.longest = std::max(c.longest, len[i]);
    return MHX_OK;
}

int triangle_dense(const uint64_t *rows, const uint32_t *len, uint32_t n, uint32_t stride, int k, uint32_t s, uint32_t *common,
                   uint32_t *denom, double *dist, int device_ptrs)
{
    bool done;
    int rc = triangle_check(rows, len, n, stride, k, s, device_ptrs, &done);
    if (rc || done) return rc;
    if (!common || !denom) return fail(MHX_E_ARG, "null argument");
    const uint64_t pairs = (uint64_t)n * (n - 1) / 2;
    TriCall c{};
    c.n = n; c.stride = stride; c.s = s; c.k = k; c.edges = false;
    if (device_ptrs) {
        c.rows = rows; c.len = len; c.longest = stride; // the lengths are on the device: the row stride bounds them
        c.common = common; c.denom = denom; c.dist = dist;
        return triangle_device(c);
    }
    const size_t bo = up256(pairs * 4);
    uint8_t *base = nullptr;
    rc = stage_rows(rows, len, n, stride, 2 * bo, &base, c);
    if (rc) return rc;
    c.common = (uint32_t *)base; c.denom = (uint32_t *)(base + bo); c.dist = nullptr; // distances in host libm below
    rc = triangle_device(c);
    if (rc) return rc;
    if (hipMemcpy(common, c.common, pairs * 4, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(denom, c.denom, pairs * 4, hipMemcpyDeviceToHost) != hipSuccess)
        return fail(MHX_E_HIP, "D2H copy failed in dist_triangle");
    if (dist)
        for (uint64_t i = 0; i < pairs; ++i) dist[i] = tri_distance(common[i], denom[i], k);
    return MHX_OK;
}

int triangle_edges(const uint64_t *rows, const uint32_t *len, uint32_t n, uint32_t stride, int k, uint32_t s, double max_dist,
                   uint32_t *edge_i, uint32_t *edge_j, uint32_t *common, uint32_t *denom, double *dist, uint64_t cap, uint64_t *n_out,
                   int device_ptrs)
{
    if (n_out) *n_out = 0;
    bool done;
    int rc = triangle_check(rows, len, n, stride, k, s, device_ptrs, &done);
    if (rc || done) return rc;
    if (!n_out || (cap && (!edge_i || !edge_j || !common || !denom))) return fail(MHX_E_ARG, "null argument");
    if (!(max_dist == max_dist)) return fail(MHX_E_ARG, "max_dist is not a number");
    const uint64_t pairs = (uint64_t)n * (n - 1) / 2;
    TriCall c{};
    c.n = n; c.stride = stride; c.s = s; c.k = k; c.edges = true;
    c.jmin = tri_jmin(max_dist, k);
    if (device_ptrs) { // the list stays where it is: prefiltered only, in the order of arrival
        c.rows = rows; c.len = len; c.longest = stride;
        c.edge_i = edge_i; c.edge_j = edge_j; c.common = common; c.denom = denom; c.dist = dist; c.cap = cap;
        rc = triangle_device(c);
        if (rc) return rc;
        *n_out = c.found;
        if (c.found > cap) return fail(MHX_E_CAPACITY, "edge list too small (%llu needed)", (unsigned long long)c.found);
        return MHX_OK;
    }
    // The device list holds what passes the prefilter; its size is not known before the run.  A first run with room for
    // the caller's cap (at least 2^20 edges) counts them all; only when they did not fit does a second run follow.
    uint64_t room = std::min<uint64_t>(pairs, std::max<uint64_t>(cap, 1u << 20));
    std::vector<uint32_t> ei, ej, ec, ed;
    for (int attempt = 0;; ++attempt) {
        const size_t be = up256(room * 4);
        uint8_t *base = nullptr;
        rc = stage_rows(rows, len, n, stride, 4 * be, &base, c);
        if (rc) return rc;
        c.edge_i = (uint32_t *)base; c.edge_j = (uint32_t *)(base + be); c.common = (uint32_t *)(base + 2 * be); c.denom = (uint32_t *)(base + 3 * be);
        c.dist = nullptr; c.cap = room;
        rc = triangle_device(c);
        if (rc) return rc;
        if (c.found <= room) break;
        if (attempt) return fail(MHX_E_INTERNAL, "edge count changed between two runs");
        room = c.found;
    }
    const size_t m = (size_t)c.found;
    ei.resize(m); ej.resize(m); ec.resize(m); ed.resize(m);
    if (m && (hipMemcpy(ei.data(), c.edge_i, m * 4, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(ej.data(), c.edge_j, m * 4, hipMemcpyDeviceToHost) != hipSuccess ||
              hipMemcpy(ec.data(), c.common, m * 4, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(ed.data(), c.denom, m * 4, hipMemcpyDeviceToHost) != hipSuccess))
        return fail(MHX_E_HIP, "D2H copy failed in dist_triangle_edges");
    // the exact rule (the libm distance that is printed) on the survivors, then Mash's order: i ascending, j < i ascending
    std::vector<size_t> keep;
    keep.reserve(m);
    for (size_t e = 0; e < m; ++e)
        if (tri_distance(ec[e], ed[e], k) <= max_dist) keep.push_back(e);
    std::sort(keep.begin(), keep.end(), [&](size_t a, size_t b) { return ei[a] != ei[b] ? ei[a] < ei[b] : ej[a] < ej[b]; });
    *n_out = keep.size();
    if (keep.size() > cap) return fail(MHX_E_CAPACITY, "edge list too small (%zu needed)", keep.size());
    for (size_t t = 0; t < keep.size(); ++t) {
        const size_t e = keep[t];
        edge_i[t] = ei[e]; edge_j[t] = ej[e]; common[t] = ec[e]; denom[t] = ed[e];
        if (dist) dist[t] = tri_distance(ec[e], ed[e], k);
    }
    return MHX_OK;
}

// Single-linkage clustering: the triangle's blocks feed the union-find of mhx_cluster.h.  The bound goes to the device as the
// cmin table, built here with host libm, so both forms are exact; nothing of the size of the pair count exists anywhere.
int triangle_cluster(const uint64_t *rows, const uint32_t *len, uint32_t n, uint32_t stride, int k, uint32_t s, double max_dist,
                     uint32_t *label, uint32_t *degree, uint32_t *n_clusters, uint64_t *n_edges, int device_ptrs)
{
    if (n_clusters) *n_clusters = 0;
    if (n_edges) *n_edges = 0;
    bool done;
    int rc = triangle_check(rows, len, n, stride, k, s, device_ptrs, &done);
    if (rc) return rc;
    if (!(max_dist == max_dist)) return fail(MHX_E_ARG, "max_dist is not a number");
    if (!n_clusters || !n_edges || (n && !label)) return fail(MHX_E_ARG, "null argument");
    if (done) { // no pair: a list on its own is a cluster
        if (n == 0) return MHX_OK;
        if (!device_ptrs) { label[0] = 0; if (degree) degree[0] = 0; }
        else if (hipMemset(label, 0, 4) != hipSuccess || (degree && hipMemset(degree, 0, 4) != hipSuccess))
            return fail(MHX_E_HIP, "hipMemset failed in dist_cluster");
        *n_clusters = 1;
        return MHX_OK;
    }
    std::vector<uint32_t> cmin((size_t)s + 1);
    cluster_cmin_build(s, k, max_dist, cmin.data());
    TriCall c{};
    c.n = n; c.stride = stride; c.s = s; c.k = k; c.edges = false; c.cluster = true; c.h_cmin = cmin.data();
    if (device_ptrs) {
        c.rows = rows; c.len = len; c.longest = stride;
        c.parent = label; c.degree = degree;
        rc = triangle_device(c);
        if (rc) return rc;
    } else {
        const size_t bn = up256((size_t)n * 4);
        uint8_t *base = nullptr;
        rc = stage_rows(rows, len, n, stride, 2 * bn, &base, c);
        if (rc) return rc;
        c.parent = (uint32_t *)base; c.degree = degree ? (uint32_t *)(base + bn) : nullptr;
        rc = triangle_device(c);
        if (rc) return rc;
        if (hipMemcpy(label, c.parent, (size_t)n * 4, hipMemcpyDeviceToHost) != hipSuccess ||
            (degree && hipMemcpy(degree, c.degree, (size_t)n * 4, hipMemcpyDeviceToHost) != hipSuccess))
            return fail(MHX_E_HIP, "D2H copy failed in dist_cluster");
    }
    *n_clusters = c.clusters;
    *n_edges = c.found;
    return MHX_OK;
}

// Single-linkage tree: Boruvka rounds over best / winner / parent (mhx_mst.h).  The pairs of a round come from the packed
// triangle, written once by the dense mode (stored: the only thing of size n^2 this call ever holds, and only when it fits
// the budget), or from the triangle's blocks run again every round (recomputed: O(n) workspace).
int triangle_mst(const uint64_t *rows, const uint32_t *len, uint32_t n, uint32_t stride, int k, uint32_t s, uint32_t *edge_i, uint32_t *edge_j,
                 uint32_t *common, uint32_t *denom, double *dist, int device_ptrs)
{
    g.last_mst_rounds = 0;
    g.last_mst_stored = -1;
    bool done;
    int rc = triangle_check(rows, len, n, stride, k, s, device_ptrs, &done);
    if (rc) return rc;
    if (s >= kMstMaxS) return fail(MHX_E_ARG, "sketch size too large for the tree (%u, below %u)", s, kMstMaxS);
    if (done) return MHX_OK; // no pair, no edge
    if (!edge_i || !edge_j || !common || !denom) return fail(MHX_E_ARG, "null argument");
    const uint64_t pairs = (uint64_t)n * (n - 1) / 2;
    uint64_t budget_mb = 4096;
    if (const char *e = getenv("MHX_MST_STORE_MB")) { const long long v = atoll(e); if (v >= 0) budget_mb = (uint64_t)v; }
    bool stored = 8 * pairs <= budget_mb << 20;
    if (const char *e = getenv("MHX_MST_STORE")) stored = strcmp(e, "0") != 0;
    TriCall c{};
    c.n = n; c.stride = stride; c.s = s; c.k = k; c.edges = false;
    // staging: [best][winner][parent][comp][counters], host form: [the four edge arrays], then rows and lengths
    const size_t bn = up256((size_t)n * 4), be = up256(((size_t)n - 1) * 4);
    const size_t state = 2 * bn + 3 * bn + 256;
    uint8_t *base = nullptr;
    if (device_ptrs) {
        rc = dist_stage(state, &base);
        if (rc) return rc;
        c.rows = rows; c.len = len; c.longest = stride;
    } else {
        rc = stage_rows(rows, len, n, stride, state + 4 * be, &base, c);
        if (rc) return rc;
    }
    MstRun m{};
    m.best = (uint64_t *)base;
    m.winner = (uint32_t *)(base + 2 * bn); m.parent = (uint32_t *)(base + 3 * bn); m.comp = (uint32_t *)(base + 4 * bn);
    m.counters = (unsigned long long *)(base + 5 * bn);
    m.n = n; m.k = k;
    if (device_ptrs) { m.edge_i = edge_i; m.edge_j = edge_j; m.common = common; m.denom = denom; m.dist = dist; }
    else {
        uint8_t *out = base + state;
        m.edge_i = (uint32_t *)out; m.edge_j = (uint32_t *)(out + be); m.common = (uint32_t *)(out + 2 * be); m.denom = (uint32_t *)(out + 3 * be);
        m.dist = nullptr; // distances in host libm below
    }
    if (stored) {
        DevArray<uint8_t> packed; // released when the call returns
        const size_t bp = up256((size_t)pairs * 4);
        if (packed.grow(2 * bp, g.stream) != hipSuccess) return fail(MHX_E_HIP, "hipMalloc failed for the stored pairs of the tree (%zu bytes)", 2 * bp);
        c.common = (uint32_t *)(uint8_t *)packed; c.denom = (uint32_t *)((uint8_t *)packed + bp); c.dist = nullptr;
        rc = triangle_device(c);
        if (rc) return rc;
        const double tri_ms = g.last_dist_ms;
        hipEventRecord(g.ev0, g.stream);
        hipError_t le = mst_begin(m);
        MstScan sc{};
        sc.common = c.common; sc.denom = c.denom; sc.n = n; sc.comp = m.comp; sc.best = m.best;
        for (uint32_t round = 0; le == hipSuccess && m.components > 1; ++round) {
            if (round == mst_max_rounds(n)) return fail(MHX_E_INTERNAL, "the tree is not finished after %u rounds (%u components)", round, m.components);
            le = mst_round_open(m);
            if (le == hipSuccess) le = launch_mst_scan(sc, g.stream);
            if (le != hipSuccess) break;
            rc = mst_round_close(m);
            if (rc) return rc;
        }
        if (le != hipSuccess) return fail(MHX_E_HIP, "tree kernel launch failed: %s", hipGetErrorString(le));
        hipEventRecord(g.ev1, g.stream);
        if (hipStreamSynchronize(g.stream) != hipSuccess) return fail(MHX_E_HIP, "tree kernel failed");
        float ms = 0.f;
        hipEventElapsedTime(&ms, g.ev0, g.ev1);
        g.last_dist_ms = tri_ms + ms;
    } else {
        const hipError_t le = mst_begin(m);
        if (le != hipSuccess) return fail(MHX_E_HIP, "tree kernel launch failed: %s", hipGetErrorString(le));
        c.mst = &m;
        rc = triangle_device(c);
        if (rc) return rc;
    }
    g.last_mst_rounds = (int)m.rounds;
    g.last_mst_stored = stored ? 1 : 0;
    if (m.components != 1 || m.appended != (uint64_t)n - 1) return fail(MHX_E_INTERNAL, "the tree has %llu edges for %u lists", (unsigned long long)m.appended, n);
    if (device_ptrs) return MHX_OK; // the edges lie where the caller wants them, in the order of arrival
    const size_t e_n = (size_t)n - 1;
    std::vector<uint32_t> ei(e_n), ej(e_n), ec(e_n), ed(e_n);
    if (hipMemcpy(ei.data(), m.edge_i, e_n * 4, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(ej.data(), m.edge_j, e_n * 4, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(ec.data(), m.common, e_n * 4, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(ed.data(), m.denom, e_n * 4, hipMemcpyDeviceToHost) != hipSuccess)
        return fail(MHX_E_HIP, "D2H copy failed in dist_mst");
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
}

} // namespace

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

extern "C" int mhx_dist_mst(const uint64_t *rows, const uint32_t *len, uint32_t n, uint32_t stride, int k, uint32_t s, uint32_t *edge_i,
                            uint32_t *edge_j, uint32_t *common, uint32_t *denom, double *dist, int device_ptrs)
{
    try {
        return triangle_mst(rows, len, n, stride, k, s, edge_i, edge_j, common, denom, dist, device_ptrs);
    } catch (const std::bad_alloc &) {
        return fail(MHX_E_INTERNAL, "mhx_dist_mst: out of host memory");
    } catch (const std::exception &e) {
        return fail(MHX_E_INTERNAL, "mhx_dist_mst: %s", e.what());
    }
}

extern "C" int mhx_dist_cluster(const uint64_t *rows, const uint32_t *len, uint32_t n, uint32_t stride, int k, uint32_t s, double max_dist,
                                uint32_t *label, uint32_t *degree, uint32_t *n_clusters, uint64_t *n_edges, int device_ptrs)
{
    try {
        return triangle_cluster(rows, len, n, stride, k, s, max_dist, label, degree, n_clusters, n_edges, device_ptrs);
    } catch (const std::bad_alloc &) {
        return fail(MHX_E_INTERNAL, "mhx_dist_cluster: out of host memory");
    } catch (const std::exception &e) {
        return fail(MHX_E_INTERNAL, "mhx_dist_cluster: %s", e.what());
    }
}

extern "C" int mhx_dist_triangle(const uint64_t *rows, const uint32_t *len, uint32_t n, uint32_t stride, int k, uint32_t s,
                                 uint32_t *common, uint32_t *denom, double *dist, int device_ptrs)
{
    try {
        return triangle_dense(rows, len, n, stride, k, s, common, denom, dist, device_ptrs);
    } catch (const std::bad_alloc &) {
        return fail(MHX_E_INTERNAL, "mhx_dist_triangle: out of host memory");
    } catch (const std::exception &e) {
        return fail(MHX_E_INTERNAL, "mhx_dist_triangle: %s", e.what());
    }
}

extern "C" int mhx_dist_triangle_edges(const uint64_t *rows, const uint32_t *len, uint32_t n, uint32_t stride, int k, uint32_t s,
                                       double max_dist, uint32_t *edge_i, uint32_t *edge_j, uint32_t *common, uint32_t *denom,
                                       double *dist, uint64_t cap, uint64_t *n_out, int device_ptrs)
{
    try {
        return triangle_edges(rows, len, n, stride, k, s, max_dist, edge_i, edge_j, common, denom, dist, cap, n_out, device_ptrs);
    } catch (const std::bad_alloc &) {
        return fail(MHX_E_INTERNAL, "mhx_dist_triangle_edges: out of host memory");
    } catch (const std::exception &e) {
        return fail(MHX_E_INTERNAL, "mhx_dist_triangle_edges: %s", e.what());
    }
}
