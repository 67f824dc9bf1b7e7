// mhx_engine_contain_within.cpp -- host side of the unbounded containment call (mhx_dist_contain_within: all references each
// query holds, as CSR): the containment search's schedule -- the containment's geometry, bounds, finish pass and pair kernel
// writing block-local, the need table of the bound (mhx_engine_contain_search.cpp) -- inside the super-batches of queries of
// mhx_dist_within, with its own take-out behind every block, and behind the last block of each super-batch the scan and the
// gather.  Rules: mhx_contain_within.h; kernels: mhx_contain_within.hip, mhx_within.hip, mhx_contain.hip and mhx_dist.hip.
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>

#include "mhx_device.h"
#include "mhx_contain_within.h"
#include "mhx_engine_sets.h"
#include "mhx_internal.h"

using namespace mhx;

namespace {

struct ContainWithinCall { // everything on the device but `need` and n_out
    const uint64_t *q, *r;
    const uint32_t *q_len, *r_len;
    uint32_t nq, nr, stride, s_q, s_r, longest;
    const uint32_t *need; // HOST: [need_limit + 1] (contain_need_build)
    uint32_t need_limit;
    uint64_t *row_off;                                      // [nq + 1]
    uint32_t *hit_ref, *hit_shared, *hit_n_ref, *hit_n_qry; // [cap]; hit_ref null: the counting form
    uint64_t cap;
    uint64_t *n_out;                                        // host
};

// Launches the whole call on the engine's stream and waits for it.  The queries go through in super-batches (mhx_within.h)
// whose cells live in g.within_ws: one run of the containment search's schedule per super-batch, and behind its last block and
// its last fallback the cells are scanned into row_off and the arrival list is gathered into the call's outputs.  A block
// that is redone later fills the same cells, so neither the order of the blocks nor the batch sizes show in the result.
// The passes of mhx_contain.hip index the rows, the bounds and the effective lengths of the CALL, so they get a block's
// first query counted from the call's first; the cells and row_off of a super-batch count from its own first query.
int contain_within_device(ContainWithinCall &c)
{
    uint64_t cells = kWithinCells;
    if (const char *e = getenv("MHX_WITHIN_CELLS")) { const long long v = atoll(e); if (v > 0 && (uint64_t)v < cells) cells = (uint64_t)v; }
    const uint32_t nslices = within_slices(c.nr), super = within_super_queries(c.nq, c.nr, cells);
    SetSchedule sch(c.nq, c.nr, c.stride, SetGeometry{contain_ranges(c.longest), c.longest, "MHX_SEARCH_QBATCH", super, "dist_contain_within"});
    sch.clear_first = sch.clear_later = sch.fast; // the flag words of the super-batch before are not this one's
    // the bounds and effective lengths of both sets, the block-local shared, n_qry, n_ref, the need table
    const size_t o_bq = sch.extra((size_t)c.nq * 8), o_br = sch.extra((size_t)c.nr * 8), o_eq = sch.extra((size_t)c.nq * 4), o_er = sch.extra((size_t)c.nr * 4);
    const size_t b_loc = (size_t)sch.qbatch * kTriSlice * 4;
    const size_t o_ls = sch.extra(b_loc), o_lq = sch.extra(b_loc), o_lr = sch.extra(b_loc), o_need = sch.extra(((size_t)c.need_limit + 1) * 4);
    int rc = sch.place("the workspace of dist_contain_within");
    if (rc) return rc;
    const bool store = c.hit_ref != nullptr && c.cap != 0;
    // the arrival list of a super-batch: its hits are at most its pairs (below 2^32: kWithinCells x 32, or one row of the
    // references), and what lies beyond the room the caller gave is only counted
    const uint32_t room = store ? (uint32_t)std::min<uint64_t>(c.cap, (uint64_t)super * c.nr) : 0;
    // the cells of a super-batch: [mask][base][arrival counter][arrival shared][arrival n_ref][arrival n_qry]
    Carve cw;
    const size_t o_mask = cw.take((size_t)super * nslices * 4), o_base = cw.take(store ? (size_t)super * nslices * 4 : 0), o_count = cw.take(256);
    const size_t o_arr_s = cw.take((size_t)room * 4), o_arr_r = cw.take((size_t)room * 4), o_arr_q = cw.take((size_t)room * 4);
    if (g.within_ws.grow(cw.bytes, g.stream) != hipSuccess) return fail(MHX_E_HIP, "hipMalloc failed for the cells of dist_contain_within (%zu bytes)", cw.bytes);
    uint32_t *mask = (uint32_t *)(g.within_ws + o_mask), *base = store ? (uint32_t *)(g.within_ws + o_base) : nullptr;
    uint32_t *count = (uint32_t *)(g.within_ws + o_count);
    hipError_t &le = sch.le;
    uint32_t *need = (uint32_t *)sch.at(o_need);
    // the table goes over before anything is queued, with a blocking copy, as in the containment search: it lies before the
    // first event, so mhx_last_dist_kernel_ms does not hold it
    if (hipMemcpy(need, c.need, ((size_t)c.need_limit + 1) * 4, hipMemcpyHostToDevice) != hipSuccess) return fail(MHX_E_HIP, "H2D copy of the need table failed");
    ContainArgs all{};
    all.q = c.q; all.q_len = c.q_len; all.nq = c.nq; all.r = c.r; all.r_len = c.r_len; all.nr = c.nr; all.stride = c.stride; all.s_q = c.s_q; all.s_r = c.s_r;
    all.q_bound = (uint64_t *)sch.at(o_bq); all.r_bound = (uint64_t *)sch.at(o_br);
    all.q_eff = (uint32_t *)sch.at(o_eq); all.r_eff = (uint32_t *)sch.at(o_er);
    all.shift = sch.words;
    all.shared = (uint32_t *)sch.at(o_ls); all.n_qry = (uint32_t *)sch.at(o_lq); all.n_ref = (uint32_t *)sch.at(o_lr); all.out_stride = kTriSlice;
    ContainWithinOut out{};
    out.loc_shared = all.shared; out.loc_n_qry = all.n_qry; out.loc_n_ref = all.n_ref; out.need = need; out.need_limit = c.need_limit; out.nslices = nslices;
    out.mask = mask; out.base = base; out.count = count; out.room = room;
    out.arr_shared = (uint32_t *)(g.within_ws + o_arr_s); out.arr_n_ref = (uint32_t *)(g.within_ws + o_arr_r); out.arr_n_qry = (uint32_t *)(g.within_ws + o_arr_q);
    // the passes of mhx_dist.hip see the effective lengths: what lies behind them in a row is not part of a list
    DistArgs lists{};
    lists.q = c.q; lists.q_len = all.q_eff; lists.nq = c.nq; lists.r = c.r; lists.r_len = all.r_eff; lists.nr = c.nr; lists.stride = c.stride;
    sch.begin();
    if (le == hipSuccess) le = hipMemsetAsync(c.row_off, 0, 8, g.stream);
    if (le == hipSuccess) le = launch_contain_bounds(all, g.stream);
    sch.offsets(lists);
    for (uint32_t s0 = 0; s0 < c.nq && le == hipSuccess; s0 += super) {
        const uint32_t snq = std::min(super, c.nq - s0);
        auto block_args = [&](const SearchBlock &b) { // cell (q, r) of the block lies at (q - q0) * 32 + (r - r0), q0 of the CALL
            ContainArgs x = all;
            x.q0 = s0 + b.q0; x.bnq = b.nq; x.r0 = b.r0; x.bnr = b.nr;
            x.out_base = (uint64_t)x.q0 * kTriSlice + b.r0;
            return x;
        };
        le = hipMemsetAsync(mask, 0, (size_t)snq * nslices * 4, g.stream);
        if (le == hipSuccess) le = hipMemsetAsync(count, 0, 4, g.stream);
        rc = sch.run(
            s0, snq, [&](const SearchBlock &b, const DistArgs &) { return launch_contain_pairs(block_args(b), g.stream); },
            [&](const SearchBlock &b, const DistArgs &, const DistWork &w) { return launch_contain_finish(block_args(b), w, g.stream); },
            [&](const SearchBlock &b, const uint32_t *flag) {
                ContainWithinOut t = out;
                t.flag = flag; t.r0 = b.r0; t.nr = b.nr; t.q0 = b.q0; t.nq = b.nq; // (the cells count from the super-batch's first query)
                return launch_contain_within_take(t, g.stream);
            });
        if (rc) return rc;
        if (le != hipSuccess) break;
        WithinRows scan{};
        scan.mask = mask; scan.nq = snq; scan.nslices = nslices; scan.row_off = c.row_off + s0;
        le = launch_within_scan(scan, g.stream);
        ContainWithinRows rows{};
        rows.mask = mask; rows.base = base; rows.nq = snq; rows.nslices = nslices; rows.row_off = c.row_off + s0;
        rows.arr_shared = out.arr_shared; rows.arr_n_ref = out.arr_n_ref; rows.arr_n_qry = out.arr_n_qry; rows.room = room;
        rows.hit_ref = c.hit_ref; rows.hit_shared = c.hit_shared; rows.hit_n_ref = c.hit_n_ref; rows.hit_n_qry = c.hit_n_qry; rows.cap = store ? c.cap : 0;
        if (le == hipSuccess) le = launch_contain_within_gather(rows, g.stream);
    }
    rc = sch.end();
    return rc ? rc : sch.wait(hipMemcpyAsync(c.n_out, c.row_off + c.nq, 8, hipMemcpyDeviceToHost, g.stream));
}

int too_small(uint64_t found) { return fail(MHX_E_CAPACITY, "hit list too small (%llu needed)", (unsigned long long)found); }

// Host queries against references that are on the device already (refs) or on the host (r / r_len, refs null).  The device's
// CSR is the result: the bound went there as integers, so nothing is filtered here.  Staging holds the rows, the lengths,
// row_off and min(cap, nq * nr) entries of the four hit arrays.
int contain_within_host(const uint64_t *q, const uint64_t *const *q_rows, const uint32_t *q_len, uint32_t nq, uint32_t s_q, const uint64_t *r,
                        const uint32_t *r_len, const SearchRefs *refs, uint32_t nr, uint32_t s_r, uint32_t stride, int k, double min_identity,
                        uint32_t min_shared, uint64_t *row_off, uint32_t *hit_ref, uint32_t *hit_shared, uint32_t *hit_n_ref, uint32_t *hit_n_qry, uint64_t cap,
                        uint64_t *n_out)
{
    const uint64_t room = hit_ref ? std::min<uint64_t>(cap, (uint64_t)nq * nr) : 0;
    Carve csr; // row_off and the four hit arrays
    const size_t o_off = csr.take(((size_t)nq + 1) * 8), o_ref = csr.take((size_t)room * 4), o_shared = csr.take((size_t)room * 4);
    const size_t o_nref = csr.take((size_t)room * 4), o_nqry = csr.take((size_t)room * 4);
    StagedSets in{};
    int rc = stage_sets("dist_contain_within", HostSet{q, q_rows, q_len, nq}, HostSet{r, nullptr, r_len, nr}, refs, stride, csr.bytes, in);
    if (rc) return rc;
    ContainWithinCall c{};
    c.q = in.q; c.q_len = in.q_len; c.r = in.r; c.r_len = in.r_len;
    c.nq = nq; c.nr = nr; c.stride = stride; c.s_q = s_q; c.s_r = s_r;
    c.longest = refs ? contain_eff_len(refs->longest, stride, s_r) : 0;
    for (uint32_t i = 0; i < nq; ++i) c.longest = std::max(c.longest, contain_eff_len(q_len[i], stride, s_q));
    if (!refs) for (uint32_t i = 0; i < nr; ++i) c.longest = std::max(c.longest, contain_eff_len(r_len[i], stride, s_r));
    c.need_limit = std::min(stride, s_r);
    c.need = contain_need_table(c.need_limit, k, min_identity, min_shared);
    c.row_off = (uint64_t *)(in.room + o_off);
    if (room) {
        c.hit_ref = (uint32_t *)(in.room + o_ref); c.hit_shared = (uint32_t *)(in.room + o_shared);
        c.hit_n_ref = (uint32_t *)(in.room + o_nref); c.hit_n_qry = (uint32_t *)(in.room + o_nqry);
    }
    c.cap = room;
    c.n_out = n_out;
    rc = contain_within_device(c);
    if (rc) return rc;
    rc = read_back("dist_contain_within", {{row_off, c.row_off, ((size_t)nq + 1) * 8}});
    if (rc) return rc;
    if (!hit_ref && cap == 0) return MHX_OK; // the counting form
    const uint64_t m = *n_out;
    if (m > cap) return too_small(m);
    return read_back("dist_contain_within", {{hit_ref, c.hit_ref, m * 4, m != 0}, {hit_shared, c.hit_shared, m * 4, m != 0}, {hit_n_ref, c.hit_n_ref, m * 4, m != 0},
                                             {hit_n_qry, c.hit_n_qry, m * 4, m != 0}});
}

} // namespace

namespace mhx {
int contain_within_rows(const uint64_t *const *q_rows, const uint32_t *q_len, uint32_t nq, uint32_t s_q, const SearchRefs &refs, uint32_t s_r, int k,
                        double min_identity, uint32_t min_shared, uint64_t *row_off, uint32_t *hit_ref, uint32_t *hit_shared, uint32_t *hit_n_ref,
                        uint32_t *hit_n_qry, uint64_t cap, uint64_t *n_out)
{
    *n_out = 0;
    int rc = contain_hit_check(s_q, s_r, refs.stride, k, min_identity, min_shared);
    if (rc || nq == 0) return rc;
    if (refs.nr == 0) { memset(row_off, 0, ((size_t)nq + 1) * 8); return MHX_OK; }
    return contain_within_host(nullptr, q_rows, q_len, nq, s_q, nullptr, nullptr, &refs, refs.nr, s_r, refs.stride, k, min_identity, min_shared, row_off,
                               hit_ref, hit_shared, hit_n_ref, hit_n_qry, cap, n_out);
}
} // namespace mhx

extern "C" int mhx_dist_contain_within(const uint64_t *q, const uint32_t *q_len, uint32_t nq, uint32_t s_q, const uint64_t *r, const uint32_t *r_len, uint32_t nr,
                                       uint32_t s_r, uint32_t stride, int k, double min_identity, uint32_t min_shared, uint64_t *row_off, uint32_t *hit_ref,
                                       uint32_t *hit_shared, uint32_t *hit_n_ref, uint32_t *hit_n_qry, uint64_t cap, uint64_t *n_out, int device_ptrs)
{
    return entry("mhx_dist_contain_within", [&]() -> int {
        int rc = contain_hit_check(s_q, s_r, stride, k, min_identity, min_shared);
        if (rc) return rc;
        if (nq == 0) { if (n_out) *n_out = 0; return MHX_OK; }
        if (!row_off || !n_out) return fail(MHX_E_ARG, "null argument");
        const bool counting = !hit_ref && !hit_shared && !hit_n_ref && !hit_n_qry && cap == 0;
        if (!counting && (!hit_ref || !hit_shared || !hit_n_ref || !hit_n_qry)) return fail(MHX_E_ARG, "null argument");
        *n_out = 0;
        if (nr == 0) {
            if (device_ptrs) { if (hipMemset(row_off, 0, ((size_t)nq + 1) * 8) != hipSuccess) return fail(MHX_E_HIP, "hipMemset failed in dist_contain_within"); }
            else memset(row_off, 0, ((size_t)nq + 1) * 8);
            return MHX_OK;
        }
        if (!q || !q_len || !r || !r_len) return fail(MHX_E_ARG, "null argument");
        if (!device_ptrs)
            return contain_within_host(q, nullptr, q_len, nq, s_q, r, r_len, nullptr, nr, s_r, stride, k, min_identity, min_shared, row_off, hit_ref, hit_shared,
                                       hit_n_ref, hit_n_qry, cap, n_out);
        ContainWithinCall c{}; // the lengths are on the device: the kernels clip them, the row stride and the sketch sizes bound them
        c.q = q; c.q_len = q_len; c.r = r; c.r_len = r_len; c.nq = nq; c.nr = nr; c.stride = stride; c.s_q = s_q; c.s_r = s_r;
        c.longest = std::min(stride, std::max(s_q, s_r));
        c.need_limit = std::min(stride, s_r);
        c.need = contain_need_table(c.need_limit, k, min_identity, min_shared);
        c.row_off = row_off; c.hit_ref = hit_ref; c.hit_shared = hit_shared; c.hit_n_ref = hit_n_ref; c.hit_n_qry = hit_n_qry; c.cap = cap; c.n_out = n_out;
        rc = contain_within_device(c);
        if (rc) return rc;
        return !counting && *n_out > cap ? too_small(*n_out) : MHX_OK;
    });
}
