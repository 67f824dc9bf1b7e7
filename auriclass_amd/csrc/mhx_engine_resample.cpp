// mhx_engine_resample.cpp -- host side of the jackknife over the hashes of a sketch set: one replicate of a set
// (mhx_resample_rows), the support values of the neighbour-joining tree (mhx_dist_nj_support: the main tree, then per replicate
// resample, cut, one 4-byte readback, dense triangle, init and joins, everything allocated once), and the exact count of the
// splits of the main tree among the replicates' on the host (mhx_nj_split_support).
// Rules: mhx_resample.h, mhx_nj.h; kernels: mhx_resample.hip, mhx_nj.hip and, through the triangle, mhx_triangle.hip and mhx_dist.hip.
#include <hip/hip_runtime.h>
#include <stdlib.h>

#include <algorithm>
#include <unordered_map>
#include <vector>

#include "mhx_device.h"
#include "mhx_nj.h"
#include "mhx_resample.h"
#include "mhx_triangle.h"
#include "mhx_engine_internal.h"
#include "mhx_engine_nj.h"
#include "mhx_engine_triangle.h"
#include "mhx_internal.h"

using namespace mhx;

namespace {

// ---- splits ---------------------------------------------------------------------------------------------------------------------
// The leaf set of the node of join t is the union of those of its two ids; canon(X) = X if leaf 0 is not in it, else its
// complement.  A split with 0, 1, n - 1 or n leaves on a side is in every tree.  Sets are bitsets of n bits, compared word by
// word; their 64-bit signature only finds the candidates.
using Bits = std::vector<uint64_t>;

uint64_t signature(const Bits &b)
{
    uint64_t h = 0x9E3779B97F4A7C15ull;
    for (uint64_t w : b) { h ^= w; h *= 0xBF58476D1CE4E5B9ull; h ^= h >> 29; }
    return h;
}

// Walks the joins of one tree in join order: visit(t, leaf set of join t made canonical, its leaves) for every join whose
// split is not in every tree, trivial(t) for the others.  False: the joins are no tree of n leaves (ids b < a < n, both
// nodes at the time of the join).
template <class Visit, class Trivial> bool walk_splits(const uint32_t *ja, const uint32_t *jb, uint32_t n, Visit visit, Trivial trivial)
{
    const size_t words = ((size_t)n + 63) / 64;
    std::vector<Bits> set(n);          // of the node with this id; empty: still the leaf alone
    std::vector<uint32_t> count(n, 1); // its leaves; 0: no node any more
    for (uint32_t t = 0; t + 1 < n; ++t) {
        const uint32_t a = ja[t], b = jb[t];
        if (a >= n || b >= a || count[a] == 0 || count[b] == 0) return false;
        Bits &into = set[b];
        if (into.empty()) { into.assign(words, 0); into[b >> 6] |= 1ull << (b & 63); }
        if (set[a].empty()) into[a >> 6] |= 1ull << (a & 63);
        else for (size_t w = 0; w < words; ++w) into[w] |= set[a][w];
        Bits().swap(set[a]); // a is no node any more: its set is let go
        count[b] += count[a];
        count[a] = 0;
        const uint32_t side = count[b];
        if (side <= 1 || side + 1 >= n) { trivial(t); continue; }
        if (into[0] & 1ull) { // leaf 0 is in it: the complement, within n bits
            Bits c(words);
            for (size_t w = 0; w < words; ++w) c[w] = ~into[w];
            if (n & 63) c[words - 1] &= (1ull << (n & 63)) - 1ull;
            visit(t, c);
        } else visit(t, into);
    }
    return true;
}

// the splits of the main tree, and how many replicates hold each
struct SplitCounter {
    uint32_t n;
    std::vector<Bits> split;                                  // of join t; empty: in every tree
    std::unordered_map<uint64_t, std::vector<uint32_t>> find; // signature -> joins
    std::vector<uint32_t> stamp;                              // the last replicate (1-based) that counted join t

    bool begin(const uint32_t *ja, const uint32_t *jb, uint32_t n_)
    {
        n = n_;
        split.assign(n - 1, Bits());
        stamp.assign(n - 1, 0);
        return walk_splits(ja, jb, n, [&](uint32_t t, const Bits &b) { split[t] = b; find[signature(b)].push_back(t); }, [](uint32_t) {});
    }
    // replicate `rep` (0-based): support[t] grows by one for every join t of the main tree whose split the replicate holds
    bool add(const uint32_t *ja, const uint32_t *jb, uint32_t rep, uint32_t *support)
    {
        return walk_splits(ja, jb, n,
                           [&](uint32_t, const Bits &b) {
                               const auto it = find.find(signature(b));
                               if (it == find.end()) return;
                               for (uint32_t t : it->second)
                                   if (stamp[t] != rep + 1 && split[t] == b) { stamp[t] = rep + 1; ++support[t]; }
                           },
                           [](uint32_t) {});
    }
    // the joins whose split is in every tree
    void finish(uint32_t replicates, uint32_t *support) const
    {
        for (uint32_t t = 0; t + 1 < n; ++t) if (split[t].empty()) support[t] = replicates;
    }
};

int check_resampling(double keep, uint32_t replicates, uint64_t *T)
{
    if (!resample_threshold(keep, T)) return fail(MHX_E_ARG, "keep must lie in (0, 1] (%g)", keep);
    if (replicates > kResampleMaxReplicates) return fail(MHX_E_ARG, "too many replicates (%u, at most %u)", replicates, kResampleMaxReplicates);
    return MHX_OK;
}

// one replicate on the stream and its s_r on the host; the device is done when this returns
int resample_once(const ResampleArgs &ra, double keep, uint32_t *s_r)
{
    hipError_t e = launch_resample(ra, g.stream);
    if (e == hipSuccess) e = launch_resample_clamp(ra, g.stream);
    if (e != hipSuccess) return fail(MHX_E_HIP, "resample kernel launch failed: %s", hipGetErrorString(e));
    uint32_t back = 0;
    e = hipMemcpyAsync(&back, ra.s_r, 4, hipMemcpyDeviceToHost, g.stream);
    if (e == hipSuccess) e = hipStreamSynchronize(g.stream);
    if (e != hipSuccess) return fail(MHX_E_HIP, "resample kernel failed: %s", hipGetErrorString(e));
    *s_r = back;
    if (back == 0) return fail(MHX_E_ARG, "replicate %u keeps no hash of a full list at keep = %g", ra.replicate, keep);
    return MHX_OK;
}

} // namespace

extern "C" int mhx_nj_split_support(const uint32_t *join_a, const uint32_t *join_b, const uint32_t *rep_join_a, const uint32_t *rep_join_b, uint32_t n,
                                    uint32_t replicates, uint32_t *support)
{
    return guarded("mhx_nj_split_support", [&]() -> int {
        clear_error();
        if (n <= 1) return MHX_OK;
        if (n > kTriMaxLists) return fail(MHX_E_ARG, "too many lists for one tree (%u, at most %u)", n, kTriMaxLists);
        if (!join_a || !join_b || !support || (replicates && (!rep_join_a || !rep_join_b))) return fail(MHX_E_ARG, "null argument");
        const size_t m = (size_t)n - 1;
        SplitCounter sc;
        if (!sc.begin(join_a, join_b, n)) return fail(MHX_E_ARG, "the joins of the main tree are no tree of %u leaves", n);
        std::vector<uint32_t> count(m, 0);
        for (uint32_t r = 0; r < replicates; ++r)
            if (!sc.add(rep_join_a + r * m, rep_join_b + r * m, r, count.data())) return fail(MHX_E_ARG, "the joins of replicate %u are no tree of %u leaves", r, n);
        sc.finish(replicates, count.data());
        std::copy(count.begin(), count.end(), support);
        return MHX_OK;
    });
}

extern "C" int mhx_resample_rows(const uint64_t *rows, const uint32_t *len, uint32_t n, uint32_t stride, uint32_t s, uint64_t seed, uint32_t replicate,
                                 double keep, uint64_t *out_rows, uint32_t *out_len, uint32_t *s_out, int device_ptrs)
{
    return guarded("mhx_resample_rows", [&]() -> int {
        clear_error();
        int rc = require_engine();
        if (rc) return rc;
        uint64_t T = 0;
        rc = check_resampling(keep, 0, &T);
        if (rc) return rc;
        if (n > kTriMaxLists) return fail(MHX_E_ARG, "too many lists for one set (%u, at most %u)", n, kTriMaxLists);
        if (s == 0 || stride == 0) return fail(MHX_E_ARG, "bad s / stride");
        if (!s_out || (n && (!rows || !len || !out_rows || !out_len))) return fail(MHX_E_ARG, "null argument");
        if (!device_ptrs)
            for (uint32_t i = 0; i < n; ++i) if (len[i] > stride) return fail(MHX_E_ARG, "len[%u] exceeds stride", i);
        if (n == 0) { *s_out = s; return MHX_OK; } // no list is full
        // staging: [s_r], host form: [out rows][out lengths][rows][lengths]
        const size_t rows_bytes = device_ptrs ? 0 : (size_t)n * stride * 8, len_bytes = device_ptrs ? 0 : (size_t)n * 4;
        Carve in;
        const size_t o_word = in.take(4), o_out = in.take(rows_bytes), o_olen = in.take(len_bytes), o_rows = in.take(rows_bytes), o_len = in.take(len_bytes);
        uint8_t *base = nullptr;
        rc = dist_stage(in.bytes, &base);
        if (rc) return rc;
        ResampleArgs ra{rows, len, n, stride, s, seed, T, replicate, out_rows, out_len, (uint32_t *)(base + o_word)};
        if (!device_ptrs) {
            uint8_t *d_out = base + o_out, *d_olen = base + o_olen, *d_rows = base + o_rows, *d_len = base + o_len;
            hipError_t ce = hipMemcpyAsync(d_rows, rows, (size_t)n * stride * 8, hipMemcpyHostToDevice, g.stream);
            if (ce == hipSuccess) ce = hipMemcpyAsync(d_len, len, (size_t)n * 4, hipMemcpyHostToDevice, g.stream);
            if (ce != hipSuccess) return fail(MHX_E_HIP, "H2D copy failed in resample_rows: %s", hipGetErrorString(ce));
            ra.rows = (const uint64_t *)d_rows; ra.len = (const uint32_t *)d_len;
            ra.out_rows = (uint64_t *)d_out; ra.out_len = (uint32_t *)d_olen;
        }
        uint32_t s_r = 0;
        rc = resample_once(ra, keep, &s_r);
        *s_out = s_r;
        if (rc || device_ptrs) return rc;
        return read_back("resample_rows", {{out_rows, ra.out_rows, rows_bytes}, {out_len, ra.out_len, len_bytes}});
    });
}

// The support values of the neighbour-joining tree.  The rows are staged once; the pair words, the triangle's two arrays, the
// state of the joins, one replicate row matrix and one set of replicate records are allocated once, before the main tree.  A
// replicate is resample, cut, a 4-byte readback of s_r (the triangle's geometry needs it on the host), dense triangle, init
// and joins, and the copy of its join_a / join_b to the host, where its splits are counted at once: nothing of the size of
// replicates x n is held unless the caller asks for the replicates' joins.  Device memory: 16 n (n - 1) / 2 bytes for the whole
// call (the triangle's arrays stay, unlike in mhx_dist_nj) and a second row matrix; the words must fit MHX_LINKAGE_STORE_MB.
extern "C" int mhx_dist_nj_support(const uint64_t *rows, const uint32_t *len, uint32_t n, uint32_t stride, int k, uint32_t s, uint32_t replicates, double keep,
                                   uint64_t seed, uint32_t *join_a, uint32_t *join_b, uint64_t *d, uint64_t *r_a, uint64_t *r_b, double *len_a, double *len_b,
                                   uint32_t *support, uint32_t *rep_join_a, uint32_t *rep_join_b, uint32_t *rep_s, int device_ptrs)
{
    return guarded("mhx_dist_nj_support", [&]() -> int {
        g.last_nj_clamps = 0;
        bool done;
        int rc = nj_check(rows, len, n, stride, k, s, device_ptrs, &done);
        if (rc) return rc;
        uint64_t T = 0;
        rc = check_resampling(keep, replicates, &T);
        if (rc) return rc;
        if (done) return MHX_OK; // no pair, no join
        if (!join_a || !join_b || !d || !r_a || !r_b || !len_a != !len_b || !rep_join_a != !rep_join_b || (replicates && !support))
            return fail(MHX_E_ARG, "null argument");
        rc = store_fits("MHX_LINKAGE_STORE_MB", n);
        if (rc) return rc;
        const size_t m = (size_t)n - 1;
        Carve in; // staging: [state][s_r][replicate rows][replicate lengths][replicate records], host form: [main records], then rows and lengths
        const NjStateAt state(in, n);
        const size_t o_word = in.take(4), o_rows = in.take((size_t)n * stride * 8), o_len = in.take((size_t)n * 4);
        const NjRecordsAt rep_records(in, n), main_records(in, n, !device_ptrs);
        TriCall c;
        uint8_t *base = nullptr;
        rc = stage_rows(rows, len, n, stride, k, s, device_ptrs, in, &base, c);
        if (rc) return rc;
        NjArgs a{};
        state.place(a, base, n, k);
        if (device_ptrs) { a.join_a = join_a; a.join_b = join_b; a.d = d; a.r_a = r_a; a.r_b = r_b; a.len_a = len_a; a.len_b = len_b; }
        else {
            main_records.place(a, base);
            a.len_a = a.len_b = nullptr; // lengths in host arithmetic below: the same doubles
        }
        StoredTriangle tri; // all of it released when the call returns
        rc = tri.alloc((uint64_t)n * (n - 1) / 2, "neighbour joining", true);
        if (rc) return rc;
        a.words = tri.words;
        // the main tree, exactly as mhx_dist_nj
        uint64_t main_clamps = 0;
        rc = nj_tree(c, a, tri, false, &main_clamps);
        g.last_nj_clamps = main_clamps;
        if (rc) return rc;
        double total_ms = g.last_dist_ms;
        std::vector<uint32_t> h_ja, h_jb; // device form: the main joins on the host, for the count
        const uint32_t *main_a = join_a, *main_b = join_b;
        if (!device_ptrs) {
            rc = read_back("dist_nj_support", {{join_a, a.join_a, m * 4}, {join_b, a.join_b, m * 4}, {d, a.d, m * 8}, {r_a, a.r_a, m * 8}, {r_b, a.r_b, m * 8}});
            if (rc) return rc;
            if (len_a)
                for (size_t t = 0; t < m; ++t) nj_lengths(NjRecord{join_a[t], join_b[t], d[t], r_a[t], r_b[t]}, n - (uint32_t)t, len_a[t], len_b[t]);
        } else if (replicates) {
            h_ja.resize(m); h_jb.resize(m);
            rc = read_back("dist_nj_support", {{h_ja.data(), a.join_a, m * 4}, {h_jb.data(), a.join_b, m * 4}});
            if (rc) return rc;
            main_a = h_ja.data(); main_b = h_jb.data();
        }
        if (replicates == 0) return MHX_OK; // the main tree only: support stays as it is
        SplitCounter sc;
        if (!sc.begin(main_a, main_b, n)) return fail(MHX_E_INTERNAL, "the joins of the main tree are no tree of %u leaves", n);
        std::vector<uint32_t> count(m, 0), one_a, one_b;
        if (!rep_join_a) { one_a.resize(m); one_b.resize(m); }
        // the replicates: no allocation from here on
        NjArgs ar = a;
        rep_records.place(ar, base);
        ar.len_a = ar.len_b = nullptr;
        ResampleArgs ra{c.rows, c.len, n, stride, s, seed, T, 0, (uint64_t *)(base + o_rows), (uint32_t *)(base + o_len), (uint32_t *)(base + o_word)};
        for (uint32_t r = 0; r < replicates; ++r) {
            ra.replicate = r;
            uint32_t s_r = 0;
            rc = resample_once(ra, keep, &s_r);
            if (rc) return rc;
            if (rep_s) rep_s[r] = s_r;
            const TriCall cr{ra.out_rows, ra.out_len, n, stride, s_r, std::min(c.longest, s_r), k}; // no list is longer than s_r now
            uint64_t clamps = 0;
            rc = nj_tree(cr, ar, tri, false, &clamps);
            if (rc) return rc;
            total_ms += g.last_dist_ms;
            uint32_t *to_a = rep_join_a ? rep_join_a + r * m : one_a.data(), *to_b = rep_join_a ? rep_join_b + r * m : one_b.data();
            rc = read_back("dist_nj_support", {{to_a, ar.join_a, m * 4}, {to_b, ar.join_b, m * 4}});
            if (rc) return rc;
            if (!sc.add(to_a, to_b, r, count.data())) return fail(MHX_E_INTERNAL, "the joins of replicate %u are no tree of %u leaves", r, n);
        }
        sc.finish(replicates, count.data());
        std::copy(count.begin(), count.end(), support);
        g.last_dist_ms = total_ms; // the main tree and every replicate's triangle and joins
        return MHX_OK;
    });
}
