// mhx_table.hip -- passes over the candidate table: the tighten pass that lowers the admission threshold, the cap of
// that threshold, the FASTQ phase-chain check, reset, extraction of the entries below a limit, and the hash-order pass
// that finish() runs over a large extracted block.
#include "mhx_block.h"
#include "mhx_device.h"
#include "mhx_tile.h"
#include "mhx_tighten.h"

namespace mhx {

// ---------------------------------------------------------------------------------------
// Threshold tightening.  T only ever decreases, and only to a value below which at least
// s entries with count >= m already exist, so every hash of the final sketch stays admitted
// (and therefore fully counted) for the whole run.
// ---------------------------------------------------------------------------------------
// One kernel: every workgroup histograms its share of the table in LDS and flushes it with global atomics; the
// workgroup that finishes LAST (ticket) turns the histogram into the new threshold.  All cross-workgroup data moves
// through memory-side atomics (the flush, the ticket) and agent-scope loads / stores in the last workgroup (which also
// clear the bins for the next pass), with an agent-scope release in front of the ticket, so no cache of another XCD is
// ever trusted.
// Geometry (launch_tighten): at most one workgroup per CU, each with kTightenLoads independent key loads in flight per
// thread -- the pass costs a launch, the stream of the key array, one ticket per workgroup and the last workgroup's tail;
// a grid of several workgroups per CU only adds arrivals at the ticket word (10-20 ns each, one after the other) and
// release fences.  A workgroup that counted nothing below T -- the usual case from the second pass of a push on, when
// qualifying entries are one slot in thousands -- has nothing to flush.
// TableArgs::verify_rec: the pass that push_span launches last also checks the FASTQ phase chain of the push
// (phase_verify_kernel's work, one launch and one kernel boundary less).
#ifndef MHX_TIGHTEN_LOADS
#define MHX_TIGHTEN_LOADS 16
#endif
#ifndef MHX_TIGHTEN_PER_CU
#define MHX_TIGHTEN_PER_CU 1
#endif
constexpr int kTightenLoads = MHX_TIGHTEN_LOADS;
#ifdef MHX_TIGHTEN_STAMPS // diagnostic builds: wall-clock ticks (10 ns) per phase of the pass, summed over workgroups
#define MHX_TSTAMP(IDX_)                                                                                                   \
    do {                                                                                                                   \
        if (threadIdx.x == 0) {                                                                                            \
            const uint64_t now_ = wall_clock64();                                                                          \
            atomicAdd(reinterpret_cast<unsigned long long *>(a.stats) + (1 + blockIdx.x % (kStatReplicas - 1)) * kStatCount + kStatStamp0 + (IDX_), \
                      (unsigned long long)(now_ - tstamp_prev));                                                           \
            tstamp_prev = now_;                                                                                            \
        }                                                                                                                  \
    } while (0)
#else
#define MHX_TSTAMP(IDX_) do { } while (0)
#endif
__global__ __launch_bounds__(256) void table_tighten_kernel(const TableArgs a)
{
    __shared__ uint32_t h[kHistBins];
    __shared__ uint32_t occ_s, solid_s, last_s, cut_s;
    __shared__ uint32_t wave_sums[4];
    __shared__ unsigned long long tot_s[2];
#ifdef MHX_TIGHTEN_STAMPS
    uint64_t tstamp_prev = wall_clock64();
#endif
    for (int i = threadIdx.x; i < kHistBins; i += blockDim.x) h[i] = 0;
    if (threadIdx.x == 0) { occ_s = 0; solid_s = 0; cut_s = kNoCut; tot_s[0] = 0; tot_s[1] = 0; }
    __syncthreads();
    const uint64_t T = *a.thresh;
    const int lz = tighten_lz(T);
    // FASTQ, self-synchronising form: do the line phases the tiles of the push found form one chain?
    if (a.verify_rec)
        for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x + 1u; i < a.verify_ntiles; i += gridDim.x * blockDim.x)
            if (phase_chain_broken(a.verify_rec[i - 1], a.verify_rec[i]))
                atomicOr(reinterpret_cast<unsigned long long *>(a.stats) + kStatFlags, (unsigned long long)kFlagBadFastq);
    MHX_TSTAMP(0); // 0: LDS clear, T, phase chain
    uint32_t occ = 0, solid = 0;
    // sample = 1: every slot; sample = 8: one 256-slot block in eight (slots are hash-addressed, so
    // any fixed subset of blocks is a uniform sample of the entries)
    const uint64_t nblocks256 = a.nslots / 256;
    const uint64_t step = a.sample > 1 ? a.sample : 1;
    // kTightenLoads independent key loads in flight per thread: with one, the pass is a chain of L2/HBM round trips
    const uint64_t stride = (uint64_t)gridDim.x * step;
    for (uint64_t b0 = (uint64_t)blockIdx.x * step; b0 < nblocks256; b0 += kTightenLoads * stride) {
        uint64_t key[kTightenLoads];
#pragma unroll
        for (int u = 0; u < kTightenLoads; ++u) {
            const uint64_t b = b0 + u * stride;
            key[u] = b < nblocks256 ? a.keys[b * 256 + threadIdx.x] : kEmptyKey;
        }
        // ... and the counts of the entries <= T likewise, all of them issued before the first is looked at: behind the
        // first launch of a sketch every entry qualifies, and a count fetched inside the branch that tests it made that
        // pass a chain of one round trip per key.  m = 1: an occupied slot has been counted at least once, nothing to fetch.
        uint32_t cnt[kTightenLoads];
#pragma unroll
        for (int u = 0; u < kTightenLoads; ++u) {
            const bool fetch = a.min_mult > 1 && key[u] != kEmptyKey && key[u] <= T;
            cnt[u] = fetch ? a.cnts[(b0 + u * stride) * 256 + threadIdx.x] : 1u;
        }
#pragma unroll
        for (int u = 0; u < kTightenLoads; ++u) {
            if (key[u] == kEmptyKey) continue;
            ++occ;
            if (key[u] <= T && cnt[u] >= a.min_mult) {
                ++solid;
                atomicAdd(&h[tighten_bin(key[u], lz)], 1u);
            }
        }
    }
    if (occ) atomicAdd(&occ_s, occ);
    if (solid) atomicAdd(&solid_s, solid);
    __syncthreads();
    MHX_TSTAMP(1); // 1: key loop
    if (solid_s) { // (workgroup-uniform) nothing counted: every bin is zero
        // two neighbouring bins per 64-bit atomic: half the atomics of the first pass of a sketch, when every entry
        // qualifies and every workgroup has something in every bin (a bin's total is at most nslots < 2^32: no carry)
        unsigned long long *hist2 = reinterpret_cast<unsigned long long *>(a.hist);
        for (int i = threadIdx.x; i < kHistBins / 2; i += blockDim.x) {
            const uint32_t lo = h[2 * i], hi = h[2 * i + 1];
            if (lo | hi) atomicAdd(&hist2[i], (unsigned long long)lo | ((unsigned long long)hi << 32));
        }
    }
    if (threadIdx.x == 0) {
        // 64 replicas, 64 bytes apart: a thousand workgroups adding to ONE word serialise at ~10-20 ns each
        unsigned long long *acc = reinterpret_cast<unsigned long long *>(a.acc) + (blockIdx.x % kAccReplicas) * 8;
        if (occ_s) atomicAdd(&acc[0], (unsigned long long)occ_s);
        if (solid_s) atomicAdd(&acc[1], (unsigned long long)solid_s);
    }
    // every wave waits for its own atomics, the barrier collects the waves, ONE lane fences and takes the ticket
    // (256 threads fencing cost 60 us per pass)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    MHX_TSTAMP(2); // 2: flushes
    if (threadIdx.x == 0) {
        __threadfence();
        last_s = atomicAdd(a.done, 1u) == gridDim.x - 1;
    }
    __syncthreads();
    MHX_TSTAMP(3); // 3: release + ticket
#ifdef MHX_TIGHTEN_STAMPS
    if (threadIdx.x == 0) atomicAdd(reinterpret_cast<unsigned long long *>(a.stats) + (1 + blockIdx.x % (kStatReplicas - 1)) * kStatCount + kStatStamp0 + 5, 1ull); // 5: workgroups
#endif
    if (!last_s) return;

    // ---- last workgroup: first bin where the cumulative count reaches s (mhx_tighten.h) ------------------------
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    constexpr int kPer = kHistBins / 256; // bins per thread, in value order
    uint32_t c[kPer], mine = 0;
    // agent-scope loads + stores: served past the caches, like the look-back words.  All loads first -- the eight bins
    // and this pass's totals in one round trip --, then the stores that clear the words for the next pass.
#pragma unroll
    for (int j = 0; j < kPer; ++j) c[j] = __hip_atomic_load(&a.hist[kPer * t + j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    uint64_t o = 0, so = 0;
    if (t < kAccReplicas) {
        o = __hip_atomic_load(&a.acc[t * 8], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        so = __hip_atomic_load(&a.acc[t * 8 + 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
        if (c[j]) __hip_atomic_store(&a.hist[kPer * t + j], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        mine += c[j];
    }
    if (t < kAccReplicas) {
        if (o) __hip_atomic_store(&a.acc[t * 8], (uint64_t)0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (so) __hip_atomic_store(&a.acc[t * 8 + 1], (uint64_t)0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (o) atomicAdd(&tot_s[0], (unsigned long long)o);
        if (so) atomicAdd(&tot_s[1], (unsigned long long)so);
    }
    // (block_scan_excl of mhx_block.h without the total: only the waves in front of a thread's own are summed, which is
    // other code than that function's predicated sum over all four)
    uint32_t incl = mine;
#pragma unroll
    for (int o2 = 1; o2 < 64; o2 <<= 1) {
        const uint32_t v = __shfl_up(incl, o2);
        if (lane >= o2) incl += v;
    }
    if (lane == 63) wave_sums[wave] = incl;
    __syncthreads();
    uint32_t before = incl - mine;
    for (int w = 0; w < wave; ++w) before += wave_sums[w];
    const uint32_t s = tighten_target(a.sketch_size, a.sample);
    if (before < s && before + mine >= s) cut_s = tighten_cut_among(c, kPer, (uint32_t)(kPer * t), before, s); // exactly one thread gets here
    __syncthreads();
    if (t == 0) {
        const uint64_t occupied = tot_s[0] * (a.sample > 1 ? a.sample : 1), solid = tot_s[1] * (a.sample > 1 ? a.sample : 1);
        a.stats[kStatOccupied] = occupied;
        a.stats[kStatSolid] = solid;
        *a.done = 0;
        const bool was_established = a.min_mult > 1 && a.stats[kStatEstablished];
        bool established = was_established, bounded = false;
        const uint64_t now = tighten_threshold(T, lz, cut_s, a.min_mult, a.next_cap, occupied, solid, established, bounded);
        if (established && !was_established) a.stats[kStatEstablished] = 1; // from now on T follows the solid hashes: no more caps
        if (bounded) a.stats[kStatBounded] = 1;
        // (atomic: a pass between two launches of a push runs beside the next launch's cap_threshold_kernel, and T must
        // never rise -- a hash that is admitted now must have been admitted on every earlier occurrence)
        if (now < T) atomicMin(reinterpret_cast<unsigned long long *>(a.thresh), (unsigned long long)now);
    }
    MHX_TSTAMP(4); // 4: the last workgroup's tail
}

// Cap of the admission threshold that follows the bytes seen (multiplicity filter, before s solid hashes exist):
// T = min(T, cap) -- decided on the device from what the last tighten pass left in the counters, so that the host never
// waits for a round trip: no cap once a pass has lowered T from solid hashes, and none while the table looks like a
// small genome sequenced deeply (a fifth of its entries solid, yet fewer than s of them: such a sketch may need every
// solid hash there is).
__global__ void cap_threshold_kernel(uint64_t *thresh, uint64_t cap, uint64_t *stats)
{
    if (stats[kStatEstablished]) return;
    const uint64_t occupied = stats[kStatOccupied], solid = stats[kStatSolid];
    if (occupied > 0 && solid * 5 >= occupied) return;
    if (atomicMin(reinterpret_cast<unsigned long long *>(thresh), (unsigned long long)cap) > cap) stats[kStatBounded] = 1;
}

// FASTQ, self-synchronising form: do the line phases the tiles found (HashArgs::phase_rec) form one chain?
__global__ void phase_verify_kernel(const uint8_t *rec, uint32_t ntiles, uint64_t *stats)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x + 1u;
    if (i < ntiles && phase_chain_broken(rec[i - 1], rec[i]))
        atomicOr(reinterpret_cast<unsigned long long *>(stats) + kStatFlags, (unsigned long long)kFlagBadFastq);
}

hipError_t launch_phase_verify(const uint8_t *rec, uint32_t ntiles, uint64_t *stats, hipStream_t st)
{
    if (ntiles < 2) return hipSuccess;
    hipLaunchKernelGGL(phase_verify_kernel, dim3((ntiles - 1 + 255) / 256), dim3(256), 0, st, rec, ntiles, stats);
    return hipGetLastError();
}

hipError_t launch_cap_threshold(uint64_t *thresh, uint64_t cap, uint64_t *stats, hipStream_t st)
{
    hipLaunchKernelGGL(cap_threshold_kernel, dim3(1), dim3(1), 0, st, thresh, cap, stats);
    return hipGetLastError();
}

hipError_t launch_tighten(const TableArgs &a, uint32_t cus, hipStream_t st)
{
    // few, long-running workgroups (see table_tighten_kernel): no more than the device has CUs, and none with less than one
    // full round of loads
    const uint64_t step = a.sample > 1 ? a.sample : 1;
    uint64_t blocks = a.nslots / 256 / step / kTightenLoads;
    const uint64_t most = (uint64_t)(cus ? cus : 256) * MHX_TIGHTEN_PER_CU;
    if (blocks > most) blocks = most;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(table_tighten_kernel, dim3((unsigned)blocks), dim3(256), 0, st, a);
    return hipGetLastError();
}

// One launch instead of five memsets and a copy: vacates the table and clears every small control buffer.
__global__ __launch_bounds__(256) void table_reset_kernel(const TableArgs a, uint64_t t_init, uint32_t *tickets, uint32_t ntickets, uint32_t *out_n)
{
    const uint64_t n2 = a.nslots / 2, n4 = a.nslots / 4; // nslots is a power of two >= 2^16
    uint4 *k4 = reinterpret_cast<uint4 *>(a.keys), *c4 = reinterpret_cast<uint4 *>(a.cnts);
    const uint4 ones = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, zero = {0, 0, 0, 0};
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n2; i += (uint64_t)gridDim.x * blockDim.x) {
        k4[i] = ones;
        if (i < n4) c4[i] = zero;
    }
    if (blockIdx.x == 0) {
        for (uint32_t i = threadIdx.x; i < (uint32_t)kHistBins; i += blockDim.x) a.hist[i] = 0;
        for (uint32_t i = threadIdx.x; i < (uint32_t)kAccReplicas * 8; i += blockDim.x) a.acc[i] = 0;
        for (uint32_t i = threadIdx.x; i < (uint32_t)(kStatReplicas * kStatCount); i += blockDim.x) a.stats[i] = 0;
        for (uint32_t i = threadIdx.x; i < ntickets; i += blockDim.x) tickets[i] = 0;
        if (threadIdx.x == 0) { *a.thresh = t_init; *a.done = 0; *out_n = 0; if (a.need_lookback) *a.need_lookback = 0; }
    }
}

hipError_t launch_reset(const TableArgs &a, uint64_t t_init, uint32_t *tickets, uint32_t ntickets, uint32_t *out_n, hipStream_t st)
{
    uint64_t blocks = a.nslots / 2 / 256 / 4;
    if (blocks > 2048) blocks = 2048;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(table_reset_kernel, dim3((unsigned)blocks), dim3(256), 0, st, a, t_init, tickets, ntickets, out_n);
    return hipGetLastError();
}

__device__ __forceinline__ int order_shift(uint64_t T, uint32_t log2_buckets)
{ // finish(), large sketches (see launch_order_block): the bucket of a hash is its leading log2_buckets bits below T's top bit
    const int bits = 64 - __clzll((long long)(T | 1ull)); // T < 2^bits
    return bits > (int)log2_buckets ? bits - (int)log2_buckets : 0;
}

__global__ __launch_bounds__(256) void table_extract_kernel(const TableArgs a, uint64_t limit, uint32_t min_count,
                                                            uint64_t *out_keys, uint32_t *out_cnts, uint32_t cap,
                                                            uint32_t *out_n, uint64_t *flags_out, const uint64_t *limit_dev,
                                                            uint64_t *limit_out, uint64_t *maxkey_out,
                                                            uint32_t *order_cursor, uint32_t order_log2,
                                                            uint64_t *hdr_dev, uint64_t *hdr_host, uint32_t *ticket,
                                                            uint64_t *occ_out, uint32_t nhdr, uint64_t *hdr_copy)
{
    if (limit_dev) limit = *limit_dev; // the admission threshold as it stands on the device
    const int bucket_shift = order_shift(limit, order_log2);
    if (blockIdx.x == 0 && threadIdx.x == 0 && limit_out) *limit_out = limit;
    // optional: occurrences of the one hash value the table cannot hold (2^64 - 1), summed over the replicas
    if (maxkey_out && blockIdx.x == 0 && threadIdx.x < kStatReplicas) {
        const uint64_t c = a.stats[threadIdx.x * kStatCount + kStatMaxKey];
        if (c) atomicAdd(reinterpret_cast<unsigned long long *>(maxkey_out), (unsigned long long)c);
    }
    // optional: OR of the replicated device flags, so that a caller that never reads the stats block
    // (the multi-GPU slab export) still learns about a full table or a malformed FASTQ
    if (flags_out && blockIdx.x == 0 && threadIdx.x < kStatReplicas) {
        uint64_t f = a.stats[threadIdx.x * kStatCount + kStatFlags];
        if (threadIdx.x == 0) // plus the state of the m > 1 phase and the "repair pass due" word of the FASTQ parser
            f |= (a.stats[kStatBounded] ? kFlagStateBounded : 0) | (a.stats[kStatEstablished] ? kFlagStateEstablished : 0) |
                 (a.need_lookback && *a.need_lookback ? kFlagNeedLookback : 0);
        if (f) atomicOr(reinterpret_cast<unsigned long long *>(flags_out), (unsigned long long)f);
    }
    // Qualifying entries are sparse (about one per few hundred slots), so they are collected per
    // workgroup in LDS and appended to the output with ONE global atomic per flush instead of one
    // per entry (a single counter word serialises at ~10 ns per atomic).
    constexpr uint32_t kBuf = 1024;
    __shared__ unsigned long long bkeys[kBuf];
    __shared__ uint32_t bcnts[kBuf];
    __shared__ uint32_t nbuf, base, occ_s;
    if (threadIdx.x == 0) { nbuf = 0; occ_s = 0; }
    __syncthreads();
    uint32_t occ = 0; // occupied slots seen by this thread (reported when occ_out is given: the shard export)
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    const uint64_t rounds = (a.nslots + stride - 1) / stride; // same trip count for every thread (barriers inside)
    for (uint64_t rd = 0; rd <= rounds; ++rd) {
        if (rd < rounds) {
            const uint64_t i = rd * stride + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
            if (i < a.nslots) {
                const uint64_t key = a.keys[i];
                occ += key != kEmptyKey ? 1u : 0u;
                if (key != kEmptyKey && key <= limit) {
                    const uint32_t c = a.cnts[i];
                    if (c >= min_count) {
                        const uint32_t p = atomicAdd(&nbuf, 1u); // at most 256 per round, flushed below before it can overflow
                        bkeys[p] = key;
                        bcnts[p] = c;
                    }
                }
            }
        }
        __syncthreads();
        const uint32_t n = nbuf;
        if (n > kBuf - 256 || (rd == rounds && n)) { // flush
            if (threadIdx.x == 0) base = atomicAdd(out_n, n);
            __syncthreads();
            for (uint32_t j = threadIdx.x; j < n; j += blockDim.x)
                if (base + j < cap) {
                    out_keys[base + j] = bkeys[j];
                    out_cnts[base + j] = bcnts[j];
                    if (order_cursor) atomicAdd(&order_cursor[bkeys[j] >> bucket_shift], 1u); // bucket sizes for launch_order_block
                }
            __syncthreads();
            if (threadIdx.x == 0) nbuf = 0;
            __syncthreads();
        }
    }
    // finish(): the four header words [n, T, flags, max-key count] at hdr_dev go to the pinned block (whose payload the
    // flushes above have written directly) and are cleared for the next call, by the workgroup that finishes last --
    // no header memset in front of the kernel, no copy command behind it.  Same hand-over as the tighten pass: every
    // wave waits for its own memory operations, one lane releases and takes the ticket, the last workgroup reads the
    // words with agent-scope loads.
    if (occ_out) { // table occupancy (the sharded merge sizes its insertions against it), one global atomic per workgroup
        if (occ) atomicAdd(&occ_s, occ);
        __syncthreads();
        if (threadIdx.x == 0 && occ_s) atomicAdd(reinterpret_cast<unsigned long long *>(occ_out), (unsigned long long)occ_s);
    }
    if (!hdr_host) return;
    __shared__ uint32_t last_s;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        __threadfence();
        last_s = atomicAdd(ticket, 1u) == gridDim.x - 1;
    }
    __syncthreads();
    if (!last_s) return;
    if (threadIdx.x < nhdr) {
        const uint64_t v = __hip_atomic_load(&hdr_dev[threadIdx.x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        hdr_host[threadIdx.x] = v;
        if (hdr_copy) hdr_copy[threadIdx.x] = v; // the shard export: the header also rides in front of the slab
        __hip_atomic_store(&hdr_dev[threadIdx.x], (uint64_t)0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (threadIdx.x == 0) *ticket = 0;
}

hipError_t launch_extract(const TableArgs &a, uint64_t limit, uint32_t min_count, uint64_t *out_keys,
                          uint32_t *out_cnts, uint32_t cap, uint32_t *out_n, uint64_t *flags_out, const uint64_t *limit_dev,
                          uint64_t *limit_out, uint64_t *maxkey_out, hipStream_t st, uint32_t *order_cursor, uint32_t order_log2,
                          uint64_t *hdr_dev, uint64_t *hdr_host, uint32_t *ticket, uint64_t *occ_out, uint32_t nhdr, uint64_t *hdr_copy)
{
    uint64_t blocks = (a.nslots + 256 * 16 - 1) / (256 * 16);
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(table_extract_kernel, dim3((unsigned)blocks), dim3(256), 0, st, a, limit, min_count, out_keys,
                       out_cnts, cap, out_n, flags_out, limit_dev, limit_out, maxkey_out, order_cursor, order_log2,
                       hdr_dev, hdr_host, ticket, occ_out, nhdr, hdr_copy);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------
// finish(), large sketches: the result block in hash order, written straight into the pinned host block.  The
// extracted hashes are close to uniform below the threshold T (block word [1]), so a counting sort on their leading
// log2(nbuckets) bits below T's top bit puts all but a few neighbours in place: the extract kernel counts the buckets as
// it appends (order_cursor), order_scan_kernel turns counts into start positions (per group of 1024 buckets; the group
// totals are summed by whoever needs them), order_scatter_kernel places the
// entries, order_place_kernel -- one thread per bucket -- ranks the handful of entries of its bucket, stores them at
// their final position in host memory (neighbouring threads, neighbouring addresses) and clears its counter for the
// next finish().  Nothing is read back in between and no copy follows; the host checks the order of what it received
// (buckets beyond kOrderMaxBucket entries are passed through unranked) and sorts itself if it has to.
// Block layout as written by table_extract_kernel: [0] n  [1] T  [2] flags  [3] max-key count  [4 .. 4+cap) hashes
// [4+cap ..) counts.
// ---------------------------------------------------------------------------------------
constexpr uint32_t kOrderMaxBucket = 48;
constexpr uint32_t kScanChunk = 1024;    // counters per workgroup of the scan (256 threads x one uint4)
constexpr uint32_t kMaxScanGroups = 1024; // -> at most 2^20 buckets

// counts -> start positions WITHIN each group of kScanChunk buckets (coalesced, one uint4 per thread), group totals aside;
// the consumers add the groups in front themselves (group_bases)
__global__ __launch_bounds__(256) void order_scan_kernel(uint32_t *cursor, uint32_t *starts, uint32_t *group_total)
{
    __shared__ uint32_t wave_sums[4];
    const size_t v = (size_t)blockIdx.x * 256 + threadIdx.x;
    const uint4 c = reinterpret_cast<const uint4 *>(cursor)[v];
    uint32_t total;
    uint32_t run = block_scan_excl<256>(c.x + c.y + c.z + c.w, wave_sums, total);
    uint4 o;
    o.x = run; run += c.x;
    o.y = run; run += c.y;
    o.z = run; run += c.z;
    o.w = run;
    reinterpret_cast<uint4 *>(cursor)[v] = o;
    reinterpret_cast<uint4 *>(starts)[v] = o;
    if (threadIdx.x == 0) group_total[blockIdx.x] = total;
}

// sbase[g] = entries in the groups in front of group g, sbase[ngroups] = all of them (256 threads, ngroups <= 1024)
__device__ __forceinline__ void group_bases(const uint32_t *group_total, uint32_t ngroups, uint32_t *sbase, uint32_t *wave_sums)
{
    uint32_t c[4], sum = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint32_t g = 4u * threadIdx.x + j;
        c[j] = g < ngroups ? group_total[g] : 0u;
        sum += c[j];
    }
    uint32_t total;
    uint32_t run = block_scan_excl<256>(sum, wave_sums, total);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint32_t g = 4u * threadIdx.x + j;
        if (g < ngroups) sbase[g] = run;
        run += c[j];
    }
    if (threadIdx.x == 0) sbase[ngroups] = total;
    __syncthreads();
}

__global__ __launch_bounds__(256) void order_scatter_kernel(const uint64_t *blk, uint32_t cap, uint32_t log2_buckets, uint32_t *cursor,
                                                            const uint32_t *group_total, uint64_t *out)
{
    __shared__ uint32_t sbase[kMaxScanGroups + 1], wave_sums[4];
    group_bases(group_total, (1u << log2_buckets) / kScanChunk, sbase, wave_sums);
    const uint32_t n = blk[0] < cap ? (uint32_t)blk[0] : cap;
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t key = blk[4 + i];
    const uint32_t b = (uint32_t)(key >> order_shift(blk[1], log2_buckets));
    const uint32_t d = sbase[b / kScanChunk] + atomicAdd(&cursor[b], 1u);
    if (d >= cap) return; // cannot happen with counters that start from zero
    out[4 + d] = key;
    reinterpret_cast<uint32_t *>(out + 4 + cap)[d] = reinterpret_cast<const uint32_t *>(blk + 4 + cap)[i];
}

__global__ __launch_bounds__(256) void order_place_kernel(const uint64_t *blk, const uint64_t *grouped, uint32_t cap, uint32_t nbuckets,
                                                          uint32_t *cursor, const uint32_t *starts, const uint32_t *group_total, uint64_t *host_blk)
{
    __shared__ uint32_t sbase[kMaxScanGroups + 1], wave_sums[4];
    group_bases(group_total, nbuckets / kScanChunk, sbase, wave_sums);
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < 4) host_blk[b] = blk[b];
    if (b >= nbuckets) return;
    cursor[b] = 0;
    const uint32_t n = blk[0] < cap ? (uint32_t)blk[0] : cap;
    uint32_t lo = sbase[b / kScanChunk] + starts[b], hi = sbase[(b + 1) / kScanChunk] + starts[b + 1]; // starts[nbuckets] = 0 for good
    lo = lo < n ? lo : n;
    hi = hi < n ? hi : n;
    const uint32_t *gc = reinterpret_cast<const uint32_t *>(grouped + 4 + cap);
    uint32_t *hc = reinterpret_cast<uint32_t *>(host_blk + 4 + cap);
    const bool rank_them = hi - lo <= kOrderMaxBucket;
    for (uint32_t i = lo; i < hi; ++i) {
        const uint64_t key = grouped[4 + i];
        uint32_t rank = i - lo;
        if (rank_them && hi - lo > 1) {
            rank = 0;
            for (uint32_t j = lo; j < hi; ++j) rank += grouped[4 + j] < key ? 1u : 0u; // hashes of one table are distinct
        }
        host_blk[4 + lo + rank] = key;
        hc[lo + rank] = gc[i];
    }
}

hipError_t launch_order_block(const uint64_t *blk, uint32_t cap, uint32_t log2_buckets, uint32_t *cursor, uint32_t *starts,
                              uint32_t *group_total, uint64_t *grouped, uint64_t *host_blk, hipStream_t st)
{
    const uint32_t nb = 1u << log2_buckets; // 2^10 .. 2^20
    if (nb < kScanChunk || nb / kScanChunk > kMaxScanGroups) return hipErrorInvalidValue;
    const unsigned blocks = (cap + 255) / 256;
    hipLaunchKernelGGL(order_scan_kernel, dim3(nb / kScanChunk), dim3(256), 0, st, cursor, starts, group_total);
    hipLaunchKernelGGL(order_scatter_kernel, dim3(blocks), dim3(256), 0, st, blk, cap, log2_buckets, cursor, group_total, grouped);
    hipLaunchKernelGGL(order_place_kernel, dim3(nb / 256), dim3(256), 0, st, blk, grouped, cap, nb, cursor, starts, group_total, host_blk);
    return hipGetLastError();
}

} // namespace mhx
