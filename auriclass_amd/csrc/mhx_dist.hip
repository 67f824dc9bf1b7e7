// mhx_dist.hip -- mash distance on the device: one workgroup per (query, ref) pair (dist_pairs_kernel), and the
// all-vs-refs fast path (value-range partition + LDS hash probe) for batches against at most 32 references.  The rules
// the kernels share with the CPU emulator are in mhx_dist.h.
#include "mhx_device.h"
#include "mhx_dist.h"

namespace mhx {

// ---------------------------------------------------------------------------------------
// mash compareSketches for one (query, ref) pair per workgroup (Mash 2.x
// CommandDistance.cpp; invoked by /root/reference/auriclass/classes.py:92-104).
// The two ascending lists are merged along 256 merge-path diagonals.  In merged order
// (ties: ref copy first) the query copy of a shared hash directly follows the ref copy, so
//   common = #query copies whose distinct-rank (position - shared copies so far) <= s
//   denom  = min(s, |ref| + |qry| - shared)
// which is exactly what the sequential two-pointer loop with its tail completion yields.
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t merge_path(const uint64_t *A, uint32_t nA, const uint64_t *B, uint32_t nB, uint32_t diag)
{ // number of A elements among the first `diag` merged elements (A first on ties)
    uint32_t lo = diag > nB ? diag - nB : 0, hi = diag < nA ? diag : nA;
    while (lo < hi) {
        const uint32_t i = (lo + hi) >> 1, j = diag - 1 - i;
        if (A[i] <= B[j]) lo = i + 1; else hi = i;
    }
    return lo;
}

__global__ __launch_bounds__(256) void dist_pairs_kernel(const DistArgs a)
{
    __shared__ uint32_t part[256];
    __shared__ uint32_t total_common;
    const uint32_t pair = blockIdx.x;
    const uint32_t qi = pair / a.nr, ri = pair % a.nr;
    const uint64_t *A = a.r + (uint64_t)ri * a.stride; // ref
    const uint64_t *B = a.q + (uint64_t)qi * a.stride; // query
    const uint32_t nA = a.r_len[ri], nB = a.q_len[qi];
    const uint32_t total = nA + nB;
    const uint32_t t = threadIdx.x;
    const uint32_t per = (total + 255) / 256;
    const uint32_t d0 = min(t * per, total), d1 = min(d0 + per, total);
    const uint32_t i0 = merge_path(A, nA, B, nB, d0), i1 = merge_path(A, nA, B, nB, d1);
    const uint32_t j0 = d0 - i0, j1 = d1 - i1;
    // pass 1: shared copies in my segment (a query element equal to the ref element before it)
    uint32_t c = 0;
    {
        uint32_t i = i0, j = j0;
        while (i < i1 || j < j1) {
            if (i < i1 && (j >= j1 || A[i] <= B[j])) ++i;
            else { if (i > 0 && A[i - 1] == B[j]) ++c; ++j; }
        }
    }
    part[t] = c;
    if (t == 0) total_common = 0;
    __syncthreads();
    uint32_t before = 0, all = 0;
    for (uint32_t x = 0; x < 256; ++x) { const uint32_t v = part[x]; all += v; if (x < t) before += v; }
    // pass 2: count the shared copies whose distinct rank is within s
    uint32_t counted = 0;
    if (c) {
        uint32_t i = i0, j = j0, pos = d0, seen = before;
        while (i < i1 || j < j1) {
            ++pos;
            if (i < i1 && (j >= j1 || A[i] <= B[j])) ++i;
            else {
                if (i > 0 && A[i - 1] == B[j]) { ++seen; if (pos - seen <= a.s) ++counted; }
                ++j;
            }
        }
    }
    if (counted) atomicAdd(&total_common, counted);
    __syncthreads();
    if (t == 0) {
        const uint32_t uni = total - all;
        const uint32_t denom = uni < a.s ? uni : a.s;
        const uint32_t common = total_common;
        const uint64_t out = (uint64_t)qi * a.out_stride + a.out_off + ri; // the references may be a slice of a wider batch
        a.common[out] = common;
        a.denom[out] = denom;
        if (a.dist) {
            double d;
            if (common == denom) d = 0.0;
            else if (common == 0) d = 1.0;
            else {
                const double jac = (double)common / (double)denom;
                d = -log(2.0 * jac / (1.0 + jac)) / (double)a.k;
                if (d > 1.0) d = 1.0;
            }
            a.dist[out] = d;
        }
    }
}

hipError_t launch_dist_pairs(const DistArgs &a, hipStream_t st)
{
    const uint64_t pairs = (uint64_t)a.nq * a.nr;
    if (pairs == 0) return hipSuccess;
    hipLaunchKernelGGL(dist_pairs_kernel, dim3((unsigned)pairs), dim3(256), 0, st, a);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------
// All-vs-refs distance, fast path.  Hash values are uniform, so cutting the value space into
// R equal ranges cuts every sorted list into R short, aligned sub-lists (offsets by one pass
// over the list).  R = kDistRanges (1024) x W, W chosen on the host from the length of the
// call's longest list (mhx_dist.h: dist_windows; W = 1 up to 65 536 entries, 16 at 2^20), so
// that a slice holds at most 64 entries on average whatever the sketch size.  The scale is
// rounded to a power of two, so between R / 2 + 1 and R of the ranges are really in use.
// For one range, ALL references' hashes (<= 32 refs) go into one LDS hash
// table: key -> bit mask of the references that contain it.  Every query element is then
// probed ONCE and yields its shared-hash bits for all references at the same time (ballot +
// popcount per reference), instead of being merged 24 times.  A last kernel walks the
// per-range counts of each (query, ref) pair to the range where the union reaches s and
// finishes that one short range exactly with the sequential two-pointer rule.
// The shift, split and range kernels are templates with two instantiations: <false> is the
// base form (W = 1: kDistRanges is a compile-time constant -- the code of round 3, instruction
// for instruction), <true> the windowed form (R = w.ranges), which also has a level between
// pair and range in the finish pass (dist_window_kernel, dist_finish_wide_kernel).
// The rules themselves are the host+device functions of mhx_dist.h.
// ---------------------------------------------------------------------------------------
template <bool kWide> __device__ __forceinline__ uint32_t dist_ranges(const DistWork &w) { return kWide ? w.ranges : (uint32_t)kDistRanges; }

template <bool kWide> __global__ void dist_shift_kernel(const DistArgs a, DistWork w)
{
    __shared__ unsigned long long gmax;
    if (threadIdx.x == 0) gmax = 0;
    __syncthreads();
    unsigned long long m = 0;
    for (uint32_t i = threadIdx.x; i < a.nq + a.nr; i += blockDim.x) {
        const bool isq = i < a.nq;
        const uint32_t li = isq ? i : i - a.nq;
        const uint32_t n = isq ? a.q_len[li] : a.r_len[li];
        if (n) {
            const uint64_t v = (isq ? a.q : a.r)[(uint64_t)li * a.stride + n - 1];
            m = v > m ? v : m;
        }
    }
    atomicMax(&gmax, m);
    __syncthreads();
    if (threadIdx.x == 0) {
        w.params[0] = dist_shift_for(gmax, dist_ranges<kWide>(w)); // value >> shift is a range index < R
        w.params[1] = 0;
    }
}

// offs[list][p] = first element of the list whose range index (value >> shift) is >= p, for p = 0 .. R.
// One thread per ELEMENT: it compares its range index with its left neighbour's and writes the few offsets that fall
// between the two (none at all for 98 % of the elements: a range holds ~49 of them).  Every list is read once, coalesced --
// the per-offset binary searches of round 1 moved 709 MB per C5 call for 419 MB of lists and ran at the HBM limit.
template <bool kWide> __global__ __launch_bounds__(256) void dist_split_kernel(const DistArgs a, DistWork w, uint32_t list0)
{
    const uint32_t list = blockIdx.x + list0, per = dist_ranges<kWide>(w) + 1; // lists along x (no 65 535 limit), element blocks along y
    const bool isq = list < a.nq;
    const uint32_t li = isq ? list : list - a.nq;
    const uint32_t n = isq ? a.q_len[li] : a.r_len[li];
    const uint64_t *v = (isq ? a.q : a.r) + (uint64_t)li * a.stride;
    uint32_t *offs = (isq ? w.offs_q : w.offs_r) + li * per;
    const uint32_t shift = w.params[0];
    // two elements per thread: one 16-byte load where the row is 16-byte aligned (8-byte loads run at 0.55-0.7x the rate)
    const uint32_t i = 2 * (blockIdx.y * blockDim.x + threadIdx.x);
    if (n == 0) {
        if (blockIdx.y == 0) for (uint32_t p = threadIdx.x; p < per; p += blockDim.x) offs[p] = 0;
        return;
    }
    if (i >= n) return;
    uint64_t e0, e1 = 0;
    const bool two = i + 1 < n;
    if (two && (reinterpret_cast<uintptr_t>(v + i) & 15) == 0) {
        const uint4 q = *reinterpret_cast<const uint4 *>(v + i);
        e0 = ((uint64_t)q.y << 32) | q.x;
        e1 = ((uint64_t)q.w << 32) | q.z;
    } else {
        e0 = v[i];
        if (two) e1 = v[i + 1];
    }
    const uint32_t r0 = dist_range_of(e0, shift), r1 = two ? dist_range_of(e1, shift) : r0;
    // offsets p in (range of the left neighbour, range of this element] point at this element; the list's first element
    // also serves p = 0 .. its own range, the last one leaves everything above its range at n
    const uint32_t from = i == 0 ? 0u : dist_range_of(v[i - 1], shift) + 1u;
    dist_split_offsets(offs, per, i, n, two, from, r0, r1);
}

// Sum over the wave of a word of four byte counters (no carry between the bytes as long as every total stays < 256),
// by DPP row operations; lane 63 ends up with the totals.
__device__ __forceinline__ uint32_t wave_sum_bytes(uint32_t v)
{
    v += __builtin_amdgcn_update_dpp(0u, v, 0x111, 0xf, 0xf, false); // row_shr:1
    v += __builtin_amdgcn_update_dpp(0u, v, 0x112, 0xf, 0xf, false); // row_shr:2
    v += __builtin_amdgcn_update_dpp(0u, v, 0x114, 0xf, 0xf, false); // row_shr:4
    v += __builtin_amdgcn_update_dpp(0u, v, 0x118, 0xf, 0xf, false); // row_shr:8  -> lane 15 of every row holds the row's sum
    v += __builtin_amdgcn_update_dpp(0u, v, 0x142, 0xa, 0xf, false); // row_bcast:15 into rows 1 and 3
    v += __builtin_amdgcn_update_dpp(0u, v, 0x143, 0xc, 0xf, false); // row_bcast:31 into rows 2 and 3
    return v;
}

// One reference hash into the range's LDS table: key -> bit mask of the references that hold it.  `ndistinct` counts the
// keys (slots claimed).  Whether a range fits is decided by THAT number, not by the sum of the references' slice sizes:
// references of one clade share most of their hashes (AuriClass's 24 C. auris references do), so 24 slices of 65 hashes
// are 70 keys, not 1560 -- with the sum as the test every such reference set fell back to the generic kernel (0.48 ms
// instead of 0.05 for AuriClass's own 1 x 24 comparison, 62 ms instead of 0.4 for 1024 queries).  The probe sequence is
// bounded by the table size, so a table that does fill up (non-uniform values) ends the build instead of hanging it; the
// caller checks `ndistinct` against kDistTableLimit behind the barrier and gives the range up.
// returns the number of keys this call added (0 or 1; kDistTableSlots when the table had no room at all): the callers sum
// it per thread and add the wave totals to the shared count once, behind the build (dist_table_count).
// kEmptyKey (2^64 - 1, a legitimate hash) cannot be a slot's key: its references go into the mask word kept for it behind
// the slots (mhx_dist.h: kDistEmptyMask) and it adds no key.
__device__ __forceinline__ uint32_t dist_table_insert(unsigned long long *keys, uint32_t *masks, uint64_t v, uint32_t r)
{
    if (v == kEmptyKey) { atomicOr(&masks[kDistEmptyMask], 1u << r); return 0u; }
    uint32_t sl = dist_slot_of(v);
#pragma nounroll
    for (int probe = 0; probe < kDistTableSlots; ++probe) {
        const unsigned long long prev = atomicCAS(&keys[sl], (unsigned long long)kEmptyKey, (unsigned long long)v);
        if (prev == kEmptyKey || prev == v) { atomicOr(&masks[sl], 1u << r); return prev == kEmptyKey ? 1u : 0u; }
        sl = (sl + 1) & (kDistTableSlots - 1);
    }
    return (uint32_t)kDistTableSlots;
}
__device__ __forceinline__ void dist_table_count(uint32_t *ndistinct, uint32_t mine)
{ // all lanes of the wave call this
#pragma unroll
    for (int o = 32; o; o >>= 1) mine += __shfl_xor(mine, o);
    if ((threadIdx.x & 63) == 0 && mine) atomicAdd(ndistinct, mine);
}

template <bool kWide> __global__ __launch_bounds__(256) void dist_range_kernel(const DistArgs a, DistWork w)
{
    __shared__ unsigned long long keys[kDistTableSlots];
    __shared__ uint32_t masks[kDistMaskWords];
    __shared__ uint32_t too_big;
    // neighbouring ranges share the cache lines their slices begin and end in: consecutive workgroups go round the eight
    // XCDs, so this order puts ranges p, p + 1, ... of one eighth of the value space on ONE XCD (its L2), close in time
    const uint32_t R = dist_ranges<kWide>(w), p = dist_range_of_block(blockIdx.x, R), per = R + 1;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    dist_table_clear(keys, masks, tid, 256);
    if (tid == 0) too_big = 0; // number of distinct keys in the table
    __syncthreads();
    // build: wave w inserts references w, w+4, ...; a reference's slice of this range is a
    // few dozen hashes, so all slices of the wave are loaded first, then inserted
    {
        constexpr int G = 8; // 32 references / 4 waves
        uint64_t x[G];
        bool have[G];
        uint32_t added = 0;
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const uint32_t r = wave + 4 * g;
            have[g] = false;
            if (r < a.nr) {
                const uint32_t b = w.offs_r[r * per + p], e = w.offs_r[r * per + p + 1];
                if (b + lane < e) { x[g] = a.r[(uint64_t)r * a.stride + b + lane]; have[g] = true; }
            }
        }
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const uint32_t r = wave + 4 * g;
            if (r >= a.nr) continue;
            const uint32_t b = w.offs_r[r * per + p], e = w.offs_r[r * per + p + 1];
            // windowed form: a reference slice of more than 255 entries is no uniform input either -- it is not inserted
            // (a crowded range of a large sketch holds 10^5 entries and more, each of which would probe a full table from end
            // to end) and counts as a table overflow
            if (kWide && e - b > kDistSliceLimit) { added += (uint32_t)kDistTableSlots; continue; }
            for (uint32_t i = b + lane; i < e; i += 64) {
                const uint64_t v = (i == b + lane && have[g]) ? x[g] : a.r[(uint64_t)r * a.stride + i];
                added += dist_table_insert(keys, masks, v, r);
            }
        }
        dist_table_count(&too_big, added);
    }
    __syncthreads();
    if (too_big > kDistTableLimit) { // non-uniform input: the host reruns the generic kernel (uniform exit: the count is shared)
        if (tid == 0) atomicOr(&w.params[1], 1u);
        return;
    }
    // probe: wave w takes queries q0+w, q0+w+4, ... of this block's chunk, 8 at a time so that
    // eight global loads are in flight per lane; each query element is looked up once and its reference mask (one bit
    // per reference) is spread into byte counters, four references to a word; one DPP reduction per word and query
    // slice leaves the shared-hash counts of all references in lane 63, which stores them as bytes.
    const uint32_t qper = (a.nq + gridDim.y - 1) / gridDim.y;
    const uint32_t q0 = blockIdx.y * qper, q1 = min(a.nq, q0 + qper);
    const uint32_t nwords = (a.nr + 3) / 4;
    constexpr int G = 8;
    for (uint32_t qb = q0 + wave; qb < q1; qb += 4 * G) {
        uint64_t x[G];
        uint32_t bb[G], ee[G];
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const uint32_t q = qb + 4 * g;
            bb[g] = ee[g] = 0;
            if (q < q1) { bb[g] = w.offs_q[q * per + p]; ee[g] = w.offs_q[q * per + p + 1]; }
        }
#pragma unroll
        for (int g = 0; g < G; ++g) {
            x[g] = kEmptyKey;
            if (bb[g] + lane < ee[g]) x[g] = a.q[(uint64_t)(qb + 4 * g) * a.stride + bb[g] + lane];
        }
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const uint32_t q = qb + 4 * g;
            if (q >= q1) break;
            if (ee[g] - bb[g] > 255u) { // a byte counter could overflow: not a uniform input, the generic kernel takes over
                if (lane == 0) atomicOr(&w.params[1], 1u);
                continue;
            }
            uint32_t acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            for (uint32_t i0 = bb[g]; i0 < ee[g]; i0 += 64) {
                uint32_t m = 0;
                if (i0 + lane < ee[g]) {
                    const uint64_t v = i0 == bb[g] ? x[g] : a.q[(uint64_t)q * a.stride + i0 + lane];
                    m = dist_table_probe(keys, masks, v);
                }
#pragma unroll
                for (int j = 0; j < 8; ++j) // bits 4j .. 4j+3 of the mask -> the low bit of four bytes
                    if (j < (int)nwords) acc[j] += dist_spread4(m, j);
            }
            uint8_t *dst = w.cpart + ((uint64_t)q * R + p) * (4 * nwords);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                if (j >= (int)nwords) break;
                const uint32_t tot = wave_sum_bytes(acc[j]);
                if (lane == 63) reinterpret_cast<uint32_t *>(dst)[j] = tot;
            }
        }
    }
}

// The same pass with ONE QUERY PER LANE (round 3; used when a chunk holds enough queries to fill the lanes): lane t walks
// the slice of query q0 + t in this range element by element -- load, table probe, spread of the reference mask into
// byte counters -- so that nothing has to be reduced across lanes: the kernel above spends 60 of its ~170 VALU
// instructions per (query, range) slice on the wave-wide tally of a slice that fills 49 of 64 lanes once, this one spends
// ~40 per ELEMENT ROUND of 64 slices, i.e. a quarter of the instructions per element.  Each lane reads its own row
// (16-byte loads where the pair is aligned: a 64-byte line serves four loads of the same lane out of L1/L2), the rows
// of a workgroup's 256 queries are 256 concurrent streams.
#ifndef MHX_DIST_LANE_BLOCK
#define MHX_DIST_LANE_BLOCK 512
#endif
constexpr int kLaneBlock = MHX_DIST_LANE_BLOCK; // queries (= threads) per workgroup: they share one table build
template <bool kWide> __global__ __launch_bounds__(kLaneBlock) void dist_range_lane_kernel(const DistArgs a, DistWork w)
{
    __shared__ unsigned long long keys[kDistTableSlots];
    __shared__ uint32_t masks[kDistMaskWords];
    __shared__ uint32_t ndistinct; // keys in the table
    const uint32_t R = dist_ranges<kWide>(w), p = dist_range_of_block(blockIdx.x, R), per = R + 1;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // where range p begins and ends in every reference: lane r of EVERY wave holds reference r's pair (nr <= 32), so all
    // reference loads of the build are issued together -- two HBM round trips for the whole build instead of two per
    // reference and wave
    uint32_t rb = 0, re = 0;
    if ((uint32_t)lane < a.nr) { rb = w.offs_r[lane * per + p]; re = w.offs_r[lane * per + p + 1]; }
    dist_table_clear(keys, masks, tid, kLaneBlock);
    if (tid == 0) ndistinct = 0;
    uint32_t added = 0;
    auto insert = [&](uint64_t v, uint32_t r) { added += dist_table_insert(keys, masks, v, r); };
    constexpr int kWaves = kLaneBlock / 64, kPerWave = (32 + kWaves - 1) / kWaves;
    uint64_t rv[kPerWave];
    uint32_t have = 0;
#pragma unroll
    for (int t = 0; t < kPerWave; ++t) { // build: wave w inserts references w, w + #waves, ...; their first 64 elements
        const uint32_t r = (uint32_t)wave + (uint32_t)kWaves * t;
        const uint32_t b = __shfl(rb, (int)(r & 31u)), e = __shfl(re, (int)(r & 31u));
        rv[t] = 0;
        if (kWide && r < a.nr && e - b > kDistSliceLimit) { added += (uint32_t)kDistTableSlots; continue; } // (see dist_range_kernel: counts as a table overflow)
        if (r < a.nr && b + lane < e) { rv[t] = a.r[(uint64_t)r * a.stride + b + lane]; have |= 1u << t; }
    }
    __syncthreads(); // the table is clear
#pragma unroll
    for (int t = 0; t < kPerWave; ++t)
        if ((have >> t) & 1u) insert(rv[t], (uint32_t)wave + (uint32_t)kWaves * t);
    for (uint32_t r = wave; r < a.nr; r += kWaves) { // slices of more than 64 elements (rare with uniform hashes)
        const uint32_t b = __shfl(rb, (int)r), e = __shfl(re, (int)r);
        if (kWide && e - b > kDistSliceLimit) continue;
        for (uint32_t i = b + 64u + lane; i < e; i += 64) insert(a.r[(uint64_t)r * a.stride + i], r);
    }
    dist_table_count(&ndistinct, added);
    __syncthreads();
    if (ndistinct > kDistTableLimit) { // non-uniform input: the host reruns the generic kernel (uniform exit: the count is shared)
        if (tid == 0) atomicOr(&w.params[1], 1u);
        return;
    }
    const uint32_t q = blockIdx.y * kLaneBlock + tid;
    if (q >= a.nq) return;
    const uint32_t nwords = (a.nr + 3) / 4;
    const uint32_t b = w.offs_q[q * per + p], e = w.offs_q[q * per + p + 1];
    uint32_t *dst = reinterpret_cast<uint32_t *>(w.cpart + ((uint64_t)q * R + p) * (4 * nwords));
    if (e - b > 255u) { // a byte counter could overflow: not a uniform input, the generic kernel takes over
        atomicOr(&w.params[1], 1u);
        return;
    }
    const uint64_t *row = a.q + (uint64_t)q * a.stride;
    uint32_t acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    auto one = [&](uint64_t v) {
        const uint32_t m = dist_table_probe(keys, masks, v);
#pragma unroll
        for (int j = 0; j < 8; ++j) // bits 4j .. 4j+3 of the mask -> the low bit of four bytes
            if (j < (int)nwords) acc[j] += dist_spread4(m, j);
    };
#ifndef MHX_DIST_LINE64
    if ((reinterpret_cast<uintptr_t>(row) & 127) == 0 && (a.stride & 15u) == 0) {
        // whole 128-byte L2 lines, both halves consumed at once.  With one 64-byte half per step (the form below, round 3's
        // first) the lane kernel fetched exactly TWICE the rows' bytes: 65 k lanes per XCD each keep a line and the next in
        // flight, 8 MB against 4 MB of L2, so the other half of a 128-byte L2 line was gone again before its lane came
        // back for it.  C5: 830 -> 564 MB fetched by this kernel, 0.388 -> 0.399 ms (16 instead of 8 element slots per
        // step, more of them masked at the ends of a slice; -DMHX_DIST_LINE64 brings the old form back)
        for (uint32_t i0 = b & ~15u; i0 < e; i0 += 16) {
            uint4 x[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) x[u] = *reinterpret_cast<const uint4 *>(row + i0 + 2 * u);
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const uint32_t i = i0 + 2 * u;
                if (i >= b && i < e) one(((uint64_t)x[u].y << 32) | x[u].x);
                if (i + 1 >= b && i + 1 < e) one(((uint64_t)x[u].w << 32) | x[u].z);
            }
        }
    } else
#endif
    if ((reinterpret_cast<uintptr_t>(row) & 63) == 0 && (a.stride & 7u) == 0) { // (rows of whole lines: nothing is read beyond a row)
        // whole 64-byte lines, each fetched ONCE by the one lane that needs it (four 16-byte loads issued together; with
        // a load per pair of elements a line was fetched up to four times, and 1500 concurrent streams per CU do not fit
        // in its L1); the elements of the first and last line that lie outside the slice are skipped
        uint4 nx[4]; // the line after the one being worked on is already on its way
        const uint32_t first = b & ~7u;
        if (first < e) {
#pragma unroll
            for (int u = 0; u < 4; ++u) nx[u] = *reinterpret_cast<const uint4 *>(row + first + 2 * u);
        }
        for (uint32_t i0 = first; i0 < e; i0 += 8) {
            uint4 x[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) x[u] = nx[u];
            if (i0 + 8 < e) {
#pragma unroll
                for (int u = 0; u < 4; ++u) nx[u] = *reinterpret_cast<const uint4 *>(row + i0 + 8 + 2 * u);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const uint32_t i = i0 + 2 * u;
                if (i >= b && i < e) one(((uint64_t)x[u].y << 32) | x[u].x);
                if (i + 1 >= b && i + 1 < e) one(((uint64_t)x[u].w << 32) | x[u].z);
            }
        }
    } else {
        uint32_t i = b;
        if (i < e && ((reinterpret_cast<uintptr_t>(row + i) & 15) != 0)) { one(row[i]); ++i; }
        for (; i + 2 <= e; i += 2) {
            const uint4 x = *reinterpret_cast<const uint4 *>(row + i);
            one(((uint64_t)x.y << 32) | x.x);
            one(((uint64_t)x.w << 32) | x.z);
        }
        if (i < e) one(row[i]);
    }
#pragma unroll
    for (int j = 0; j < 8; ++j)
        if (j < (int)nwords) dst[j] = acc[j];
}

// ---- the same all-vs-refs pass without a split pass over the queries (round 3) ------------------------------------------
// dist_split_kernel reads every list once more just to find where the 1024 ranges begin: as much HBM traffic as the
// comparison itself.  Here a workgroup takes kDistWalk CONSECUTIVE ranges for its 256 queries, one query per lane: a lane
// only needs to know where its FIRST range begins (dist_segstart_kernel: one binary search per kDistWalk ranges), walks
// on from there -- the next range starts where the value's range index changes -- and leaves the range starts behind for
// the finish kernel (offs_q).  The line a range ends in is still in the lane's registers when the next range begins.
// Base form only: a windowed call (W > 1) is never sent here, whatever MHX_DIST_WALK_MIN says.
#ifndef MHX_DIST_WALK
#define MHX_DIST_WALK 4
#endif
constexpr uint32_t kDistWalk = MHX_DIST_WALK;

__global__ __launch_bounds__(256) void dist_segstart_kernel(const DistArgs a, DistWork w)
{
    constexpr uint32_t G = kDistRanges / kDistWalk, per = kDistRanges + 1;
    const uint32_t id = blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= a.nq * (G + 1)) return;
    const uint32_t q = id / (G + 1), g = id % (G + 1);
    const uint32_t n = a.q_len[q], shift = w.params[0];
    const uint64_t *v = a.q + (uint64_t)q * a.stride;
    uint32_t lo = 0, hi = n; // first index whose range index (value >> shift) is >= g * kDistWalk
    if (g == G) lo = n;
    else if (g != 0) {
        const uint64_t want = (uint64_t)g * kDistWalk;
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if ((v[mid] >> shift) < want) lo = mid + 1; else hi = mid;
        }
    }
    w.offs_q[q * per + g * kDistWalk] = lo;
}

__global__ __launch_bounds__(256) void dist_walk_kernel(const DistArgs a, DistWork w)
{
    __shared__ unsigned long long keys[kDistTableSlots];
    __shared__ uint32_t masks[kDistMaskWords];
    __shared__ uint32_t too_big;
    constexpr uint32_t G = kDistRanges / kDistWalk, per = kDistRanges + 1;
    // consecutive workgroups go round the eight XCDs: neighbouring segments of one eighth of the value space on one XCD
    const uint32_t g = (blockIdx.x & 7u) * (G / 8) + (blockIdx.x >> 3);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t shift = w.params[0];
    const uint32_t q = blockIdx.y * 256 + tid;
    const bool live = q < a.nq;
    const uint32_t nwords = (a.nr + 3) / 4;
    const uint32_t n = live ? a.q_len[q] : 0u;
    const uint64_t *row = a.q + (uint64_t)(live ? q : 0u) * a.stride;
    uint32_t i = live ? w.offs_q[q * per + g * kDistWalk] : 0u;
#ifndef MHX_DIST_LINE64
    constexpr uint32_t kLineElems = 16; // a whole 128-byte L2 line per step: both halves are used before it is evicted
#else
    constexpr uint32_t kLineElems = 8;
#endif
    uint4 x[kLineElems / 2] = {};
    uint32_t loaded = 0xFFFFFFFFu; // first element of the line held in x
    auto slot_of = [](uint64_t v) { return (uint32_t)((v * 0x9E3779B97F4A7C15ull) >> 40) & (kDistTableSlots - 1); };
#pragma nounroll
    for (uint32_t r = 0; r < kDistWalk; ++r) {
        const uint32_t p = g * kDistWalk + r;
        dist_table_clear(keys, masks, tid, 256);
        if (tid == 0) too_big = 0; // number of distinct keys in the table
        __syncthreads();
        uint32_t added = 0;
        for (uint32_t rr = wave; rr < a.nr; rr += 4) { // build: wave w inserts references w, w + 4, ...
            const uint32_t b = w.offs_r[rr * per + p], e = w.offs_r[rr * per + p + 1];
            for (uint32_t j = b + lane; j < e; j += 64) {
                added += dist_table_insert(keys, masks, a.r[(uint64_t)rr * a.stride + j], rr);
            }
        }
        dist_table_count(&too_big, added);
        __syncthreads();
        // non-uniform input (the table overflowed): the host reruns the generic kernel; this range is skipped.  (No return
        // here: an exit between the build and the walk makes hipcc keep 112 instead of 78 VGPRs, four waves per SIMD
        // instead of six, and the walk 15 % slower.)
        if (tid == 0 && too_big > kDistTableLimit) atomicOr(&w.params[1], 1u);
        if (live && too_big <= kDistTableLimit) {
            uint32_t acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            const uint32_t begin = i;
            bool more = true; // this lane's walk through range p
            while (more) {
                const uint32_t i0 = i & ~(kLineElems - 1u);
                if (i0 >= n) break;
                if (i0 != loaded) {
#pragma unroll
                    for (int u = 0; u < (int)kLineElems / 2; ++u) x[u] = *reinterpret_cast<const uint4 *>(row + i0 + 2 * u);
                    loaded = i0;
                }
#pragma unroll
                for (int u = 0; u < (int)kLineElems; ++u) {
                    const uint32_t idx = i0 + (uint32_t)u;
                    if (!more || idx < i) continue;
                    if (idx >= n) { i = n; more = false; continue; }
                    const uint4 xv = x[u >> 1];
                    const uint64_t v = (u & 1) ? (((uint64_t)xv.w << 32) | xv.z) : (((uint64_t)xv.y << 32) | xv.x);
                    if ((v >> shift) != p) { i = idx; more = false; continue; } // sorted rows: the next range begins here
                    uint32_t sl = slot_of(v), m = 0;
                    for (;;) {
                        const unsigned long long kx = keys[sl];
                        if (kx == v) { m = masks[kx == kEmptyKey ? (uint32_t)kDistEmptyMask : sl]; break; } // (dist_table_probe)
                        if (kx == kEmptyKey) break;
                        sl = (sl + 1) & (kDistTableSlots - 1);
                    }
#pragma unroll
                    for (int j = 0; j < 8; ++j) // bits 4j .. 4j+3 of the mask -> the low bit of four bytes
                        if (j < (int)nwords) acc[j] += (((m >> (4 * j)) & 0xFu) * 0x00204081u) & 0x01010101u;
                }
                if (more) i = i0 + kLineElems;
            }
            if (i > n) i = n;
            if (i - begin > 255u) atomicOr(&w.params[1], 1u); // a byte counter may have overflowed: not a uniform input
            uint32_t *dst = reinterpret_cast<uint32_t *>(w.cpart + ((uint64_t)q * kDistRanges + p) * (4 * nwords));
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (j < (int)nwords) dst[j] = acc[j];
            w.offs_q[q * per + p + 1] = i; // where the next range begins (the finish kernel reads these)
        }
        __syncthreads(); // nobody still probes the table that the next round clears
    }
}

// what the finish pass writes for one pair
__device__ __forceinline__ void dist_store(const DistArgs &a, uint32_t q, uint32_t r, uint32_t common, uint32_t denom)
{
    const uint64_t out = (uint64_t)q * a.out_stride + a.out_off + r; // the references may be a slice of a wider batch
    a.common[out] = common;
    a.denom[out] = denom;
    if (a.dist) {
        double d;
        if (common == denom) d = 0.0;
        else if (common == 0) d = 1.0;
        else {
            const double jac = (double)common / (double)denom;
            d = -log(2.0 * jac / (1.0 + jac)) / (double)a.k;
            if (d > 1.0) d = 1.0;
        }
        a.dist[out] = d;
    }
}

// 16 pairs per workgroup; thread (seg, pair) first sums its 64 ranges, then the 16 threads of
// segment 0 locate the cut segment, walk it range by range and finish the cut range with the
// sequential two-pointer rule.
__global__ __launch_bounds__(256) void dist_finish_kernel(const DistArgs a, DistWork w)
{
    __shared__ uint32_t seg_uni[kDistSegs][16], seg_com[kDistSegs][16];
    constexpr int RPS = kDistRanges / kDistSegs; // ranges per segment
    // the range kernel gave up on this slice (a value range too crowded for its table or for byte counters): cpart holds
    // cells it never wrote, the host discards this result and runs the generic kernel -- nothing to do here, and
    // nothing to be walked on the strength of stale counts
    if (w.params[1] != 0) return;
    const uint32_t pl = threadIdx.x & 15, seg = threadIdx.x >> 4;
    const uint32_t pair = blockIdx.x * 16 + pl;
    const bool live = pair < a.nq * a.nr;
    const uint32_t q = live ? pair / a.nr : 0, r = live ? pair % a.nr : 0, per = kDistRanges + 1;
    // shared hashes per range of this pair: bytes, [query][range][4 * ceil(nr / 4)], 24 bytes apart from range to range
    const uint32_t cstride = 4 * ((a.nr + 3) / 4);
    const DistPair x{w.cpart + (uint64_t)q * kDistRanges * cstride + r, cstride, w.offs_q + q * per, w.offs_r + r * per,
                     a.r + (uint64_t)r * a.stride, a.q + (uint64_t)q * a.stride, a.s};
    {
        uint32_t com = 0;
        for (uint32_t p = seg * RPS; p < (seg + 1) * RPS; ++p) com += x.cp[(uint64_t)p * cstride];
        seg_com[seg][pl] = com;
        seg_uni[seg][pl] = dist_range_union(x, seg * RPS, (seg + 1) * RPS, com);
    }
    __syncthreads();
    if (seg != 0 || !live) return;
    uint32_t uni = 0, common = 0, denom;
    const uint32_t sg = dist_scan_totals(&seg_uni[0][pl], &seg_com[0][pl], 16, 0, kDistSegs, a.s, uni, common);
    if (sg == kDistSegs) denom = uni; // union smaller than s: everything counts
    else {
        const uint32_t p = dist_scan_ranges(x, sg * RPS, (sg + 1) * RPS, uni, common); // the cut range is inside this segment
        dist_two_pointer(x, p, uni, common);
        denom = a.s; // this range holds enough further union elements by construction
    }
    dist_store(a, q, r, common, denom);
}

// ---- the finish pass of the windowed form ---------------------------------------------------------------------------------
// With R = 16 384 ranges the 16 threads of a pair would each sum 1024 byte cells.  A level between pair and range keeps
// the work per thread where it is in the base form: dist_window_kernel sums every window of kDistWindowRanges (64)
// ranges once, for the four references of a word at a time -- cpart is read once, word-wise, by neighbouring threads --
// and the finish kernel works on windows: thread (group, pair) sums the 16 window totals of its group of 1024 ranges,
// thread (0, pair) walks the <= 16 group totals to the cut group, its 16 windows to the cut window, that window's 64
// ranges to the cut range (dist_scan_* of mhx_dist.h) and finishes the cut range with the two-pointer rule.
__global__ __launch_bounds__(256) void dist_window_kernel(const DistArgs a, DistWork w)
{
    if (w.params[1] != 0) return; // (see dist_finish_kernel)
    const uint32_t nwords = (a.nr + 3) / 4, nwin = w.ranges / kDistWindowRanges;
    const uint32_t id = blockIdx.x * 256 + threadIdx.x; // (query, window, word), the word fastest
    if (id >= a.nq * nwin * nwords) return;
    const uint32_t j = id % nwords, qw = id / nwords; // qw = q * nwin + window
    uint32_t tot[4];
    dist_window_sum(reinterpret_cast<const uint32_t *>(w.cpart) + (uint64_t)qw * kDistWindowRanges * nwords + j, nwords, kDistWindowRanges, tot);
    *reinterpret_cast<uint4 *>(w.wtot + ((uint64_t)qw * nwords + j) * 4) = make_uint4(tot[0], tot[1], tot[2], tot[3]);
}

__global__ __launch_bounds__(256) void dist_finish_wide_kernel(const DistArgs a, DistWork w)
{
    constexpr uint32_t kGroupWindows = kDistRanges / kDistWindowRanges; // a group: 16 windows, kDistRanges ranges
    __shared__ uint32_t grp_uni[kDistMaxWindows][16], grp_com[kDistMaxWindows][16];
    if (w.params[1] != 0) return; // (see dist_finish_kernel)
    const uint32_t R = w.ranges, ngroups = R / kDistRanges, per = R + 1;
    const uint32_t pl = threadIdx.x & 15, grp = threadIdx.x >> 4;
    const uint32_t pair = blockIdx.x * 16 + pl;
    const bool live = pair < a.nq * a.nr;
    const uint32_t q = live ? pair / a.nr : 0, r = live ? pair % a.nr : 0;
    const uint32_t cstride = 4 * ((a.nr + 3) / 4);
    const DistPair x{w.cpart + (uint64_t)q * R * cstride + r, cstride, w.offs_q + q * per, w.offs_r + r * per,
                     a.r + (uint64_t)r * a.stride, a.q + (uint64_t)q * a.stride, a.s};
    const uint32_t *wt = w.wtot + (uint64_t)q * (R / kDistWindowRanges) * cstride + r; // this pair's window totals, cstride words apart
    if (grp < ngroups) {
        uint32_t com = 0;
        for (uint32_t t = grp * kGroupWindows; t < (grp + 1) * kGroupWindows; ++t) com += wt[(uint64_t)t * cstride];
        grp_com[grp][pl] = com;
        grp_uni[grp][pl] = dist_range_union(x, grp * kDistRanges, (grp + 1) * kDistRanges, com);
    }
    __syncthreads();
    if (grp != 0 || !live) return;
    uint32_t uni = 0, common = 0, denom;
    const uint32_t cg = dist_scan_totals(&grp_uni[0][pl], &grp_com[0][pl], 16, 0, ngroups, a.s, uni, common);
    if (cg == ngroups) denom = uni; // union smaller than s: everything counts
    else {
        const uint32_t cw = dist_scan_windows(x, wt, cstride, cg * kGroupWindows, (cg + 1) * kGroupWindows, uni, common);
        const uint32_t p = dist_scan_ranges(x, cw * kDistWindowRanges, (cw + 1) * kDistWindowRanges, uni, common);
        dist_two_pointer(x, p, uni, common);
        denom = a.s; // this range holds enough further union elements by construction
    }
    dist_store(a, q, r, common, denom);
}

size_t dist_work_bytes(uint32_t nq, uint32_t nr, uint32_t ranges, size_t *off_q, size_t *off_r, size_t *off_c, size_t *off_w, size_t *off_p)
{
    auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    const size_t cell = 4 * ((nr + 3) / 4);
    size_t o = 0;
    *off_q = o; o += up((size_t)nq * (ranges + 1) * 4);
    *off_r = o; o += up((size_t)nr * (ranges + 1) * 4);
    *off_c = o; o += up((size_t)ranges * nq * cell);
    *off_w = o; if (ranges != (uint32_t)kDistRanges) o += up((size_t)(ranges / kDistWindowRanges) * nq * cell * 4);
    *off_p = o; // behind it: two words per (query batch, reference slice) block, sized by the caller
    return o;
}

// the windowed form (w.ranges = kDistRanges * W, W > 1): the same passes with R as a launch parameter.  The caller bounds
// the batch (dist_work_bytes <= kDistWideWorkLimit), which keeps every q * (R + 1) product of the kernels below 2^32.
static hipError_t launch_dist_ranges_wide(const DistArgs &a, const DistWork &w, hipStream_t st)
{
    const uint32_t R = w.ranges;
    hipLaunchKernelGGL(dist_shift_kernel<true>, dim3(1), dim3(256), 0, st, a, w);
    hipLaunchKernelGGL(dist_split_kernel<true>, dim3(a.nq + a.nr, (a.stride + 511) / 512), dim3(256), 0, st, a, w, 0u);
    if (a.nq >= 128 && getenv("MHX_DIST_NO_LANE") == nullptr)
        hipLaunchKernelGGL(dist_range_lane_kernel<true>, dim3(R, (a.nq + kLaneBlock - 1) / kLaneBlock), dim3(kLaneBlock), 0, st, a, w);
    else { // a workgroup serves 32 queries per round: no more chunks than there are rounds (a chunk without queries only builds the table)
        const uint32_t chunks = std::min<uint32_t>(kDistQueryChunks, (a.nq + 31) / 32);
        hipLaunchKernelGGL(dist_range_kernel<true>, dim3(R, chunks), dim3(256), 0, st, a, w);
    }
    const uint32_t cells = a.nq * (R / kDistWindowRanges) * ((a.nr + 3) / 4), pairs = a.nq * a.nr;
    hipLaunchKernelGGL(dist_window_kernel, dim3((cells + 255) / 256), dim3(256), 0, st, a, w);
    hipLaunchKernelGGL(dist_finish_wide_kernel, dim3((pairs + 15) / 16), dim3(256), 0, st, a, w);
    return hipGetLastError();
}

hipError_t launch_dist_ranges(const DistArgs &a, const DistWork &w, hipStream_t st)
{
    if (w.ranges != (uint32_t)kDistRanges) return launch_dist_ranges_wide(a, w, st);
    hipLaunchKernelGGL(dist_shift_kernel<false>, dim3(1), dim3(256), 0, st, a, w);
    const bool no_lane = getenv("MHX_DIST_NO_LANE") != nullptr, no_walk = getenv("MHX_DIST_NO_WALK") != nullptr;
    // rows of whole 128-byte lines (the walk reads a row line by line), enough queries to fill the lanes.
    // Measured with 128-byte lines in both forms (C5 rows, profiles/r03_dist_line128_ab.txt): 1024 queries 0.40 ms lane
    // form / 0.49 walk (1024 workgroups of four ranges each leave the CUs a third empty), 4096: 1.30 / 1.37, 8192: 2.60 /
    // 2.52 -- the walk takes over there; it fetches 1.9x the algorithmic bytes against the lane form's 2.6x (no split
    // pass over the queries, but 257 binary searches per row).  MHX_DIST_WALK_MIN moves the switch.
    const uint32_t walk_min = getenv("MHX_DIST_WALK_MIN") ? (uint32_t)atol(getenv("MHX_DIST_WALK_MIN")) : 8192u;
    #ifndef MHX_DIST_LINE64
    const bool whole_lines = (a.stride & 15u) == 0 && (reinterpret_cast<uintptr_t>(a.q) & 127) == 0;
#else
    const bool whole_lines = (a.stride & 7u) == 0 && (reinterpret_cast<uintptr_t>(a.q) & 63) == 0;
#endif
    const bool walk = !no_lane && !no_walk && a.nq >= walk_min && whole_lines;
    if (walk) {
        hipLaunchKernelGGL(dist_split_kernel<false>, dim3(a.nr, (a.stride + 511) / 512), dim3(256), 0, st, a, w, a.nq); // the references only
        constexpr uint32_t G = kDistRanges / kDistWalk;
        hipLaunchKernelGGL(dist_segstart_kernel, dim3((a.nq * (G + 1) + 255) / 256), dim3(256), 0, st, a, w);
        hipLaunchKernelGGL(dist_walk_kernel, dim3(G, (a.nq + 255) / 256), dim3(256), 0, st, a, w);
    } else {
        hipLaunchKernelGGL(dist_split_kernel<false>, dim3(a.nq + a.nr, (a.stride + 511) / 512), dim3(256), 0, st, a, w, 0u);
        if (a.nq >= 128 && !no_lane) hipLaunchKernelGGL(dist_range_lane_kernel<false>, dim3(kDistRanges, (a.nq + kLaneBlock - 1) / kLaneBlock), dim3(kLaneBlock), 0, st, a, w);
        else hipLaunchKernelGGL(dist_range_kernel<false>, dim3(kDistRanges, kDistQueryChunks), dim3(256), 0, st, a, w);
    }
    const uint32_t pairs = a.nq * a.nr;
    hipLaunchKernelGGL(dist_finish_kernel, dim3((pairs + 15) / 16), dim3(256), 0, st, a, w);
    return hipGetLastError();
}

// ---- the passes one by one, for a caller that keeps ONE offsets table for a whole set (mhx_triangle.hip) ------------------
// The windowed kernels take R = w.ranges as a launch parameter and work for any power of two R >= 16 when offs_q and offs_r
// point into the same [list][R + 1] table.  The entry points above do not come through here.
hipError_t launch_dist_offsets(const DistArgs &a, const DistWork &w, hipStream_t st)
{ // shift (w.params[0]; [1] = 0) and offsets of the a.nq lists of a.q into w.offs_q; a.nr must be 0
    if (a.nq == 0) return hipSuccess;
    hipLaunchKernelGGL(dist_shift_kernel<true>, dim3(1), dim3(256), 0, st, a, w);
    const uint64_t per = (uint64_t)w.ranges + 1;
    const uint32_t chunk = (uint32_t)std::min<uint64_t>(a.nq, 0xFFFFFFFFull / per); // list * (R + 1) stays below 2^32 in the kernel
    for (uint32_t c0 = 0; c0 < a.nq; c0 += chunk) {
        DistArgs x = a;
        DistWork y = w;
        x.q = a.q + (uint64_t)c0 * a.stride;
        x.q_len = a.q_len + c0;
        x.nq = std::min(chunk, a.nq - c0);
        y.offs_q = w.offs_q + (uint64_t)c0 * per;
        hipLaunchKernelGGL(dist_split_kernel<true>, dim3(x.nq, (a.stride + 511) / 512), dim3(256), 0, st, x, y, 0u);
    }
    return hipGetLastError();
}

hipError_t launch_dist_offsets_both(const DistArgs &a, const DistWork &w, hipStream_t st)
{ // ONE shift over the a.nq lists of a.q and the a.nr lists of a.r (w.params[0]; [1] = 0), then the offsets of the queries
  // into w.offs_q and of the references into w.offs_r, [list][R + 1] each: the two sets of a search share their ranges
    if (a.nq == 0 && a.nr == 0) return hipSuccess;
    hipLaunchKernelGGL(dist_shift_kernel<true>, dim3(1), dim3(1024), 0, st, a, w); // a reference set is 10^5 lists: 1024 threads share them
    const uint64_t per = (uint64_t)w.ranges + 1;
    for (int side = 0; side < 2; ++side) {
        const uint32_t n = side ? a.nr : a.nq;
        const uint32_t chunk = (uint32_t)std::min<uint64_t>(n, 0xFFFFFFFFull / per); // list * (R + 1) stays below 2^32 in the kernel
        for (uint32_t c0 = 0; c0 < n; c0 += chunk) {
            DistArgs x = a;
            DistWork y = w;
            x.q = (side ? a.r : a.q) + (uint64_t)c0 * a.stride;
            x.q_len = (side ? a.r_len : a.q_len) + c0;
            x.nq = std::min(chunk, n - c0);
            x.nr = 0;
            y.offs_q = (side ? w.offs_r : w.offs_q) + (uint64_t)c0 * per;
            hipLaunchKernelGGL(dist_split_kernel<true>, dim3(x.nq, (a.stride + 511) / 512), dim3(256), 0, st, x, y, 0u);
        }
    }
    return hipGetLastError();
}

hipError_t launch_dist_range_pass(const DistArgs &a, const DistWork &w, hipStream_t st)
{ // the range pass of one block (a.nr <= 32): byte counters into w.cpart, the overflow flag into w.params[1]
    const uint32_t R = w.ranges;
    if (a.nq >= 128 && getenv("MHX_DIST_NO_LANE") == nullptr)
        hipLaunchKernelGGL(dist_range_lane_kernel<true>, dim3(R, (a.nq + kLaneBlock - 1) / kLaneBlock), dim3(kLaneBlock), 0, st, a, w);
    else {
        const uint32_t chunks = std::min<uint32_t>(kDistQueryChunks, (a.nq + 31) / 32);
        hipLaunchKernelGGL(dist_range_kernel<true>, dim3(R, chunks), dim3(256), 0, st, a, w);
    }
    return hipGetLastError();
}

hipError_t launch_dist_finish(const DistArgs &a, const DistWork &w, hipStream_t st)
{ // the finish pass of one block with R >= 1024: the base kernel at 1024 (it does not read w.wtot), window totals + wide above
    const uint32_t R = w.ranges, pairs = a.nq * a.nr;
    if (R == (uint32_t)kDistRanges) hipLaunchKernelGGL(dist_finish_kernel, dim3((pairs + 15) / 16), dim3(256), 0, st, a, w);
    else {
        const uint32_t cells = a.nq * (R / kDistWindowRanges) * ((a.nr + 3) / 4);
        hipLaunchKernelGGL(dist_window_kernel, dim3((cells + 255) / 256), dim3(256), 0, st, a, w);
        hipLaunchKernelGGL(dist_finish_wide_kernel, dim3((pairs + 15) / 16), dim3(256), 0, st, a, w);
    }
    return hipGetLastError();
}

} // namespace mhx
