// mhx_engine_triangle.cpp -- host side of the all-pairs distance within one sketch set (mhx_dist_triangle,
// mhx_dist_triangle_edges and mhx_dist_cluster; the tree, mhx_dist_mst, is in mhx_engine_mst.cpp and takes its pairs from
// here, and so do the medoids, mhx_dist_medoids in mhx_engine_medoid.cpp, whose block mode run_medoid lies here): staging
// of a host-pointer call, the schedule of (query batch, reference slice) blocks over ONE offsets table of the whole set
// (what it shares with the query-by-reference calls -- route, workspace, clock, the passes of a block, the fallback of a
// flagged block to the generic pair kernel -- is BlockSchedule in mhx_engine_sets.h), one function per mode that rides the
// schedule, the exact distance rule and the order of the edge list on the host, the bound of the clustering as a table of
// integers.
// Rules: mhx_triangle.h, mhx_cluster.h, mhx_mst.h, mhx_medoid.h; kernels: mhx_triangle.hip, mhx_cluster.hip, mhx_mst.hip,
// mhx_medoid.hip and mhx_dist.hip.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "mhx_device.h"
#include "mhx_cluster.h"
#include "mhx_medoid.h"
#include "mhx_mst.h"
#include "mhx_triangle.h"
#include "mhx_engine_internal.h"
#include "mhx_engine_triangle.h"
#include "mhx_internal.h"

using namespace mhx;

namespace {

uint32_t tri_geometry(uint32_t longest)
{
    const char *geo = getenv("MHX_TRI_GEOMETRY");
    return geo && strcmp(geo, "dist") == 0 ? tri_ranges_dist(longest) : tri_ranges(longest);
}

// The schedule of an all-pairs call, what the modes below share: BlockSchedule (mhx_engine_sets.h: route, query batch, common
// workspace, clock, the passes of a block and the fallback of a flagged one) over ONE offsets table of the whole set, split
// into value ranges ONCE (offsets() over all n lists), with a block list that a mode may filter, block-local [queries][32]
// results that the finish pass and the generic pair kernel write and the mode's take-out kernel reads, and an edge counter.
// A mode goes as BlockSchedule says, with run_blocks() once or once per round.
struct TriSchedule : BlockSchedule {
    const TriCall c;
    uint32_t nblocks;
    std::vector<TriBlock> blocks;
    size_t o_lc, o_ld; // block-local common, denom, behind the common workspace
    uint32_t *loc_c = nullptr, *loc_d = nullptr;
    unsigned long long *counter = nullptr; // a mode's count of edges (words 2 and 3), zero after begin()
    DistArgs all{};

    explicit TriSchedule(const TriCall &call)
        : BlockSchedule((uint64_t)call.n * (call.n - 1) / 2, SetGeometry{tri_geometry(call.longest), call.s, "MHX_TRI_QBATCH", call.n, "triangle"}), c(call)
    {
        TriBlock b;
        for (bool more = tri_first_block(c.n, qbatch, b); more; more = tri_next_block(c.n, qbatch, b)) blocks.push_back(b);
        nblocks = (uint32_t)blocks.size();
        carve(c.n, 0, nblocks, 4);
        o_lc = extra((size_t)qbatch * kTriSlice * 4);
        o_ld = extra((size_t)qbatch * kTriSlice * 4);
    }
    // a mode that needs only some of the blocks drops the others (before place(); the workspace keeps its size)
    template <class Keep> void keep_blocks(Keep keep)
    {
        blocks.erase(std::remove_if(blocks.begin(), blocks.end(), [&](const TriBlock &b) { return !keep(b); }), blocks.end());
        nblocks = (uint32_t)blocks.size();
    }
    int place()
    {
        const int rc = BlockSchedule::place("the triangle workspace");
        if (rc) return rc;
        loc_c = (uint32_t *)at(o_lc); loc_d = (uint32_t *)at(o_ld);
        counter = (unsigned long long *)(words + 2);
        all.q = c.rows; all.q_len = c.len; all.nq = c.n; all.nr = 0; all.stride = c.stride; all.s = c.s; all.k = c.k;
        return MHX_OK;
    }
    void offsets()
    {
        if (fast && le == hipSuccess) le = launch_dist_offsets(all, offsets_work(offq, offq), g.stream);
    }
    DistArgs block_args(const TriBlock &b) const
    {
        DistArgs x = all;
        x.q = c.rows + (uint64_t)b.q0 * c.stride; x.q_len = c.len + b.q0; x.nq = b.nq;
        x.r = c.rows + (uint64_t)b.r0 * c.stride; x.r_len = c.len + b.r0; x.nr = b.nr;
        x.common = loc_c; x.denom = loc_d; x.dist = nullptr; x.out_stride = kTriSlice; x.out_off = 0;
        return x;
    }
    // what every take-out kernel (TriOut, ClusterOut, MstOut) reads of a block; the mode fills in where its pairs go
    template <class Out> Out out_of(const TriBlock &b, const uint32_t *flag) const
    {
        Out t{};
        t.loc_common = loc_c; t.loc_denom = loc_d; t.flag = flag;
        t.r0 = b.r0; t.nr = b.nr; t.q0 = b.q0; t.nq = b.nq;
        return t;
    }
    // Every block once: range, finish and take-out pass, the flagged ones again through the generic kernel.  first: the flag
    // words are still zero and the fallbacks are counted (the tree runs the blocks once per round).  slice_done() follows the
    // last block of every reference slice (and of every group) on the range route, never a block of the pair kernel.
    template <class TakeOut, class SliceDone> int run_blocks(TakeOut take_out, bool first, SliceDone slice_done)
    {
        return BlockSchedule::run_blocks(
            nblocks, !first, true, first,
            [&](uint64_t b, DistArgs &x) {
                x = block_args(blocks[b]);
                w.offs_q = offq + (uint64_t)blocks[b].q0 * per();
                w.offs_r = offq + (uint64_t)blocks[b].r0 * per();
            },
            [&](uint64_t, const DistArgs &x) { return launch_dist_pairs(x, g.stream); },
            [&](uint64_t, const DistArgs &x, const DistWork &wk) {
                return ranges < (uint32_t)kDistRanges ? launch_tri_finish_small(x, wk, g.stream) : launch_dist_finish(x, wk, g.stream);
            },
            [&](uint64_t b, const uint32_t *flag, bool generic) {
                const TriBlock &blk = blocks[b];
                hipError_t e = take_out(blk, flag);
                const bool last = (b + 1) % kBlockGroup == 0 || b + 1 == nblocks; // of its group
                if (e == hipSuccess && !generic && (last || blocks[b + 1].r0 != blk.r0)) e = slice_done();
                return e;
            });
    }
    template <class TakeOut> int run_blocks(TakeOut take_out, bool first)
    {
        return run_blocks(take_out, first, [] { return hipSuccess; });
    }
};

// where the pairs of the dense triangle and of the edge list go
struct PairsOut {
    uint32_t *common, *denom; // dense: packed triangle; edges: [cap]
    double *dist;             // may be null
    uint32_t *edge_i, *edge_j;
    uint64_t cap;
    double jmin;
    TriOut of(const TriSchedule &sch, const TriBlock &b, const uint32_t *flag) const
    {
        TriOut t = sch.out_of<TriOut>(b, flag);
        t.k = sch.c.k;
        t.common = common; t.denom = denom; t.dist = dist;
        t.edge_i = edge_i; t.edge_j = edge_j; t.count = sch.counter; t.cap = cap; t.jmin = jmin;
        return t;
    }
};

// the edge mode: the pairs that pass the prefilter, appended in the order of arrival; *found counts them all
int run_edges(const TriCall &c, const PairsOut &o, uint64_t *found)
{
    TriSchedule sch(c);
    int rc = sch.place();
    if (rc) return rc;
    sch.begin();
    sch.offsets();
    rc = sch.run_blocks([&](const TriBlock &b, const uint32_t *flag) { return launch_tri_edges(o.of(sch, b, flag), g.stream); }, true);
    if (rc == MHX_OK) rc = sch.end();
    if (rc) return rc;
    unsigned long long back = 0;
    rc = sch.wait(hipMemcpyAsync(&back, sch.counter, 8, hipMemcpyDeviceToHost, g.stream));
    if (rc == MHX_OK) *found = back;
    return rc;
}

// The cluster mode (mhx_cluster.h): the pairs feed a union-find over parent [n] instead of an output of pairs.  h_cmin: host,
// [s + 1]; degree may be null.
int run_cluster(const TriCall &c, const uint32_t *h_cmin, uint32_t *parent, uint32_t *degree, uint32_t *clusters, uint64_t *edges)
{
    TriSchedule sch(c);
    const size_t o_roots = sch.extra(8), o_cmin = sch.extra(((size_t)c.s + 1) * 4);
    int rc = sch.place();
    if (rc) return rc;
    unsigned long long *roots = (unsigned long long *)sch.at(o_roots);
    uint32_t *cmin = (uint32_t *)sch.at(o_cmin);
    hipError_t &le = sch.le;
    sch.begin();
    if (le == hipSuccess) le = hipMemsetAsync(roots, 0, 8, g.stream);
    if (le == hipSuccess) le = hipMemcpyAsync(cmin, h_cmin, ((size_t)c.s + 1) * 4, hipMemcpyHostToDevice, g.stream);
    if (le == hipSuccess) le = launch_cluster_init(parent, degree, c.n, g.stream);
    sch.offsets();
    rc = sch.run_blocks(
        [&](const TriBlock &b, const uint32_t *flag) {
            ClusterOut t = sch.out_of<ClusterOut>(b, flag);
            t.cmin = cmin; t.s = c.s; t.parent = parent; t.degree = degree; t.n_edges = sch.counter;
            return launch_tri_cluster(t, g.stream);
        },
        true, [&] { return launch_cluster_flatten(parent, c.n, nullptr, g.stream); }); // the trees stay shallow
    if (rc) return rc;
    if (le == hipSuccess) le = launch_cluster_flatten(parent, c.n, roots, g.stream); // behind the last block: the labels
    rc = sch.end();
    if (rc) return rc;
    unsigned long long found = 0, nroots = 0;
    hipError_t se = hipMemcpyAsync(&found, sch.counter, 8, hipMemcpyDeviceToHost, g.stream);
    if (se == hipSuccess) se = hipMemcpyAsync(&nroots, roots, 8, hipMemcpyDeviceToHost, g.stream);
    rc = sch.wait(se);
    if (rc) return rc;
    *edges = found;
    *clusters = (uint32_t)nroots;
    return MHX_OK;
}

} // namespace

namespace mhx {

// The medoid mode (mhx_medoid.h): the labels are known, and only the blocks that hold a pair of one cluster are run -- the
// schedule's blocks filtered by the exact predicate on the host, the offsets table built when one is left.  Their take-out
// pass adds the in-cluster distances to sum [n]; the pick and, on request, the pair kernel follow on the same stream.
int run_medoid(const TriCall &c, const MedoidRun &m)
{
    g.last_medoid_blocks = 0;
    const bool pairs = m.common != nullptr;
    const DistToArgs to{c.rows, c.len, c.n, c.stride, c.s, m.medoid, m.common, m.denom};
    auto reset = [&](hipError_t &le) { // sums at zero, no key yet
        if (le == hipSuccess) le = hipMemsetAsync(m.sum, 0, (size_t)c.n * 8, g.stream);
        if (le == hipSuccess) le = hipMemsetAsync(m.best, 0xFF, (size_t)c.n * 8, g.stream);
    };
    auto pick = [&](hipError_t &le) {
        if (le == hipSuccess) le = launch_medoid_pick(m.label, m.sum, m.best, m.medoid, c.n, g.stream);
        if (le == hipSuccess && pairs) le = launch_dist_to(to, g.stream);
    };
    if (c.n < 2) { // a list on its own: no triangle pass
        hipError_t le = hipSuccess;
        reset(le);
        pick(le);
        if (le == hipSuccess) le = hipStreamSynchronize(g.stream);
        g.last_dist_ms = 0.0;
        if (le != hipSuccess) return fail(MHX_E_HIP, "medoid kernel failed: %s", hipGetErrorString(le));
        return MHX_OK;
    }
    TriSchedule sch(c);
    const uint32_t scheduled = sch.nblocks;
    {
        std::vector<uint32_t> start((size_t)c.n + 1), member(c.n);
        medoid_members(m.h_label, c.n, start.data(), member.data());
        sch.keep_blocks([&](const TriBlock &b) { return medoid_block_runs(b, m.h_label, start.data(), member.data()); });
    }
    g.last_medoid_blocks = (uint64_t)sch.nblocks << 32 | scheduled;
    int rc = sch.place();
    if (rc) return rc;
    hipError_t &le = sch.le;
    sch.begin();
    reset(le);
    if (sch.nblocks) {
        sch.offsets();
        rc = sch.run_blocks(
            [&](const TriBlock &b, const uint32_t *flag) {
                MedoidOut t = sch.out_of<MedoidOut>(b, flag);
                t.label = m.label; t.sum = m.sum; t.k = c.k;
                return launch_tri_medoid(t, g.stream);
            },
            true);
        if (rc) return rc;
    }
    pick(le);
    rc = sch.end();
    return rc ? rc : sch.wait();
}

// the dense mode: every pair into the packed triangle
int run_dense(const TriCall &c, uint32_t *common, uint32_t *denom, double *dist)
{
    TriSchedule sch(c);
    int rc = sch.place();
    if (rc) return rc;
    const PairsOut o{common, denom, dist, nullptr, nullptr, 0, 0.0};
    sch.begin();
    sch.offsets();
    rc = sch.run_blocks([&](const TriBlock &b, const uint32_t *flag) { return launch_tri_scatter(o.of(sch, b, flag), g.stream); }, true);
    if (rc == MHX_OK) rc = sch.end();
    return rc ? rc : sch.wait();
}

// The tree (mhx_mst.h) from the recomputed pair source: the blocks run once per round and propose to m.best; the offsets
// table is built once.  The caller has run mst_begin.
int run_mst_recomputed(const TriCall &c, MstRun &m)
{
    TriSchedule sch(c);
    int rc = sch.place();
    if (rc) return rc;
    sch.begin();
    sch.offsets();
    auto propose = [&](const TriBlock &b, const uint32_t *flag) {
        MstOut t = sch.out_of<MstOut>(b, flag);
        t.comp = m.comp; t.best = m.best;
        return launch_tri_mst(t, g.stream);
    };
    rc = mst_rounds(m, sch.le, [&](uint32_t round) { return sch.run_blocks(propose, round == 0); });
    if (rc == MHX_OK) rc = sch.end();
    return rc ? rc : sch.wait(); // (a round's close has waited already: kept, the time of the call is read here)
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

// The inputs of a call, and the regions `in` of the staging area that the caller has declared, at *base (none declared in
// the device form: *base stays null).  Device form: rows and lengths are where they are -- the lengths too, so the row stride
// bounds them.  Host form: they are copied behind the caller's regions.
int stage_rows(const uint64_t *rows, const uint32_t *len, uint32_t n, uint32_t stride, int k, uint32_t s, int device_ptrs, Carve in, uint8_t **base, TriCall &c)
{
    *base = nullptr;
    c = TriCall{rows, len, n, stride, s, stride, k};
    if (device_ptrs) return in.bytes ? dist_stage(in.bytes, base) : MHX_OK;
    const size_t o_rows = in.take((size_t)n * stride * 8), o_len = in.take((size_t)n * 4);
    const int rc = dist_stage(in.bytes, base);
    if (rc) return rc;
    uint8_t *dr = *base + o_rows, *dl = *base + o_len;
    hipError_t ce = hipMemcpyAsync(dr, rows, (size_t)n * stride * 8, hipMemcpyHostToDevice, g.stream);
    if (ce == hipSuccess) ce = hipMemcpyAsync(dl, len, (size_t)n * 4, hipMemcpyHostToDevice, g.stream);
    if (ce != hipSuccess) return fail(MHX_E_HIP, "H2D copy failed in dist_triangle: %s", hipGetErrorString(ce));
    c.rows = (const uint64_t *)dr;
    c.len = (const uint32_t *)dl;
    c.longest = 0;
    for (uint32_t i = 0; i < n; ++i) c.longest = std::max(c.longest, len[i]);
    return MHX_OK;
}

} // namespace mhx

// Single-linkage clustering: the triangle's blocks feed the union-find of mhx_cluster.h.  The bound goes to the device as the
// cmin table, built here with host libm, so both forms are exact; nothing of the size of the pair count exists anywhere.
extern "C" int mhx_dist_cluster(const uint64_t *rows, const uint32_t *len, uint32_t n, uint32_t stride, int k, uint32_t s, double max_dist,
                                uint32_t *label, uint32_t *degree, uint32_t *n_clusters, uint64_t *n_edges, int device_ptrs)
{
    return guarded("mhx_dist_cluster", [&]() -> int {
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
        Carve in; // host form: [parent][degree], then rows and lengths
        const size_t o_parent = in.take(device_ptrs ? 0 : (size_t)n * 4), o_deg = in.take(device_ptrs ? 0 : (size_t)n * 4);
        TriCall c;
        uint8_t *base = nullptr;
        rc = stage_rows(rows, len, n, stride, k, s, device_ptrs, in, &base, c);
        if (rc) return rc;
        uint32_t *parent = device_ptrs ? label : (uint32_t *)(base + o_parent), *deg = device_ptrs || !degree ? degree : (uint32_t *)(base + o_deg);
        rc = run_cluster(c, cmin.data(), parent, deg, n_clusters, n_edges);
        if (rc || device_ptrs) return rc;
        return read_back("dist_cluster", {{label, parent, (size_t)n * 4}, {degree, deg, (size_t)n * 4, degree != nullptr}});
    });
}

extern "C" int mhx_dist_triangle(const uint64_t *rows, const uint32_t *len, uint32_t n, uint32_t stride, int k, uint32_t s, uint32_t *common,
                                 uint32_t *denom, double *dist, int device_ptrs)
{
    return guarded("mhx_dist_triangle", [&]() -> int {
        bool done;
        int rc = triangle_check(rows, len, n, stride, k, s, device_ptrs, &done);
        if (rc || done) return rc;
        if (!common || !denom) return fail(MHX_E_ARG, "null argument");
        const uint64_t pairs = (uint64_t)n * (n - 1) / 2;
        Carve in; // host form: [common][denom], then rows and lengths
        const size_t o_common = in.take(device_ptrs ? 0 : pairs * 4), o_denom = in.take(device_ptrs ? 0 : pairs * 4);
        TriCall c;
        uint8_t *base = nullptr;
        rc = stage_rows(rows, len, n, stride, k, s, device_ptrs, in, &base, c);
        if (rc) return rc;
        if (device_ptrs) return run_dense(c, common, denom, dist);
        uint32_t *d_common = (uint32_t *)(base + o_common), *d_denom = (uint32_t *)(base + o_denom);
        rc = run_dense(c, d_common, d_denom, nullptr); // distances in host libm below
        if (rc == MHX_OK) rc = read_back("dist_triangle", {{common, d_common, pairs * 4}, {denom, d_denom, pairs * 4}});
        if (rc) return rc;
        if (dist)
            for (uint64_t i = 0; i < pairs; ++i) dist[i] = tri_distance(common[i], denom[i], k);
        return MHX_OK;
    });
}

extern "C" int mhx_dist_triangle_edges(const uint64_t *rows, const uint32_t *len, uint32_t n, uint32_t stride, int k, uint32_t s, double max_dist,
                                       uint32_t *edge_i, uint32_t *edge_j, uint32_t *common, uint32_t *denom, double *dist, uint64_t cap, uint64_t *n_out,
                                       int device_ptrs)
{
    return guarded("mhx_dist_triangle_edges", [&]() -> int {
        if (n_out) *n_out = 0;
        bool done;
        int rc = triangle_check(rows, len, n, stride, k, s, device_ptrs, &done);
        if (rc || done) return rc;
        if (!n_out || (cap && (!edge_i || !edge_j || !common || !denom))) return fail(MHX_E_ARG, "null argument");
        if (!(max_dist == max_dist)) return fail(MHX_E_ARG, "max_dist is not a number");
        const uint64_t pairs = (uint64_t)n * (n - 1) / 2;
        const double jmin = tri_jmin(max_dist, k);
        TriCall c;
        uint8_t *base = nullptr;
        uint64_t found = 0;
        if (device_ptrs) { // the list stays where it is: prefiltered only, in the order of arrival
            rc = stage_rows(rows, len, n, stride, k, s, 1, Carve{}, &base, c);
            if (rc == MHX_OK) rc = run_edges(c, PairsOut{common, denom, dist, edge_i, edge_j, cap, jmin}, &found);
            if (rc) return rc;
            *n_out = found;
            if (found > cap) return fail(MHX_E_CAPACITY, "edge list too small (%llu needed)", (unsigned long long)found);
            return MHX_OK;
        }
        // The device list holds what passes the prefilter; its size is not known before the run.  A first run with room for
        // the caller's cap (at least 2^20 edges) counts them all; only when they did not fit does a second run follow.
        uint64_t room = std::min<uint64_t>(pairs, std::max<uint64_t>(cap, 1u << 20));
        PairsOut d{};
        for (int attempt = 0;; ++attempt) {
            Carve in; // [edge_i][edge_j][common][denom], then rows and lengths
            const size_t o_i = in.take(room * 4), o_j = in.take(room * 4), o_common = in.take(room * 4), o_denom = in.take(room * 4);
            rc = stage_rows(rows, len, n, stride, k, s, 0, in, &base, c);
            if (rc) return rc;
            d = PairsOut{(uint32_t *)(base + o_common), (uint32_t *)(base + o_denom), nullptr, (uint32_t *)(base + o_i), (uint32_t *)(base + o_j), room, jmin};
            rc = run_edges(c, d, &found);
            if (rc) return rc;
            if (found <= room) break;
            if (attempt) return fail(MHX_E_INTERNAL, "edge count changed between two runs");
            room = found;
        }
        const size_t m = (size_t)found;
        std::vector<uint32_t> ei(m), ej(m), ec(m), ed(m);
        rc = read_back("dist_triangle_edges", {{ei.data(), d.edge_i, m * 4, m != 0}, {ej.data(), d.edge_j, m * 4, m != 0}, {ec.data(), d.common, m * 4, m != 0}, {ed.data(), d.denom, m * 4, m != 0}});
        if (rc) return rc;
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
    });
}
