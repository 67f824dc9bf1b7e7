// mhx_fasta.hip -- FASTA on the device: the raw (inflated) file bytes go to HBM as they are and three small
// kernels turn them into the dense sequence stream (MHX_FMT_SEQ) the sketch kernel hashes:
//
//   fasta_scan_kernel     per 16 KiB tile: which bytes would be kept, for either state the tile may start in
//   fasta_offsets_kernel  one workgroup: resolves every tile's start state and output offset (scan over tiles)
//   fasta_compact_kernel  per tile: writes the kept bytes to their place, notes where every record starts
//
// The bit logic of a chunk and the partition of the offsets pass live in mhx_fasta.h (host+device, run thread by thread by
// tests/emul/fasta_emul.cpp); here are the kernels, the wave shuffles, the barriers and the launches.
//
// What is kept is exactly what kseq + mash keep (mash `sketch` without -r, Sketch.cpp sketchFile; AuriClass hands the
// FASTA paths over untouched, /root/reference/auriclass/classes.py:696-713): a line that starts with '>' is a header,
// everything up to the next header is the record's sequence with every byte <= ' ' (line breaks, CR, blanks) and DEL
// squeezed out, so k-mers span the line breaks of a record; the header's own newline stays as the one separator byte in
// front of each record, so no k-mer spans two records.  A line that starts with '@' or '+' (FASTQ syntax) raises a flag and
// the host falls back to its record parser, as it does when the file does not start with '>'.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mhx_block.h"
#include "mhx_device.h"
#include "mhx_fasta.h"

namespace mhx {

static_assert(kFaTile == kFastaTile, "the host sizes its tile count by kFastaTile");

namespace {

// exclusive scan of per-thread states with `combine`; one barrier (the counters go through block_scan_excl, mhx_block.h)
__device__ __forceinline__ uint32_t block_scan_state(uint32_t s, uint32_t *tmp, uint32_t &total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t incl = s;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t v = __shfl_up(incl, o);
        if (lane >= o) incl = combine(v, incl);
    }
    uint32_t excl = __shfl_up(incl, 1);
    if (lane == 0) excl = kPass;
    if (lane == 63) tmp[wave] = incl;
    __syncthreads();
    uint32_t before = kPass, all = kPass;
    for (int w = 0; w < kFaThreads / 64; ++w) {
        if (w < wave) before = combine(before, tmp[w]);
        all = combine(all, tmp[w]);
    }
    total = all;
    return combine(before, excl);
}

} // namespace

// summary of tile t: [0] state at its end (kPass: no line starts inside), [1] kept bytes if it starts inside a sequence
// line, [2] kept bytes if it starts inside a header line
__global__ __launch_bounds__(kFaThreads) void fasta_scan_kernel(const uint8_t *base, uint64_t n, uint32_t *summary, uint32_t *flags)
{
    __shared__ uint32_t tmp[8];
    const uint64_t off = (uint64_t)blockIdx.x * kFaTile + (uint64_t)threadIdx.x * kFaBytesPerThread;
    uint32_t d[16];
    const ChunkMasks c = load_chunk(base, off, n, d);
    if (c.ls & c.fq) atomicOr(flags, 1u); // a line that starts with '@' or '+': FASTQ syntax, not for this path
    uint32_t tile_state;
    const uint32_t st_in = block_scan_state(chunk_state(c), tmp, tile_state);
    // threads whose start state is known count once; the others (in front of the tile's first line start) count twice
    uint32_t known = 0, if_seq = 0, if_hdr = 0;
    if (st_in != kPass) known = (uint32_t)__builtin_popcountll(kept_mask(c, st_in));
    else {
        if_seq = (uint32_t)__builtin_popcountll(kept_mask(c, kSeq));
        if_hdr = (uint32_t)__builtin_popcountll(kept_mask(c, kHdr));
    }
    __syncthreads();
    uint32_t t_known, t_seq, t_hdr;
    block_scan_excl<kFaThreads>(known, tmp, t_known);
    __syncthreads();
    block_scan_excl<kFaThreads>(if_seq, tmp, t_seq);
    __syncthreads();
    block_scan_excl<kFaThreads>(if_hdr, tmp, t_hdr);
    if (threadIdx.x == 0) {
        summary[3 * blockIdx.x] = tile_state;
        summary[3 * blockIdx.x + 1] = t_known + t_seq;
        summary[3 * blockIdx.x + 2] = t_known + t_hdr;
    }
}

// One workgroup: start state and output offset of every tile.  tile_in[t] = state tile t starts in, tile_off[t] = its first
// output byte; tile_off[ntiles] = total output size.
__global__ __launch_bounds__(kFaOffsetThreads) void fasta_offsets_kernel(const uint32_t *summary, uint32_t ntiles, uint32_t *tile_in, uint64_t *tile_off)
{
    __shared__ uint32_t st[kFaOffsetThreads];
    __shared__ unsigned long long sums[kFaOffsetThreads];
    const uint32_t t = threadIdx.x;
    const FaSpan sp = fa_span(t, ntiles);
    st[t] = fa_span_state(summary, sp);
    __syncthreads();
    const uint32_t in = fa_state_before(st, t);
    sums[t] = fa_walk_states(summary, sp, in, tile_in);
    __syncthreads();
    unsigned long long before = 0;
    for (uint32_t i = 0; i < t; ++i) before += sums[i];
    before = fa_walk_offsets(summary, sp, in, before, tile_off);
    if (t == kFaOffsetThreads - 1) tile_off[ntiles] = before;
}

// writes the kept bytes of tile t at out + tile_off[t]; every record separator (the newline that ends a header line) is
// also noted in seps[] (output position; unordered, at most seps_cap of them are stored, *nseps counts all)
__global__ __launch_bounds__(kFaThreads) void fasta_compact_kernel(const uint8_t *base, uint64_t n, const uint32_t *tile_in, const uint64_t *tile_off,
                                                                    uint8_t *out, uint64_t *seps, uint32_t seps_cap, uint32_t *nseps)
{
    __shared__ uint32_t tmp[8];
    const uint64_t off = (uint64_t)blockIdx.x * kFaTile + (uint64_t)threadIdx.x * kFaBytesPerThread;
    uint32_t d[16];
    const ChunkMasks c = load_chunk(base, off, n, d);
    uint32_t tile_state;
    uint32_t st_in = block_scan_state(chunk_state(c), tmp, tile_state);
    if (st_in == kPass) st_in = tile_in[blockIdx.x];
    const uint64_t hdr = header_mask(c, st_in);
    uint64_t keep = (~hdr & c.keepc) | (hdr & c.nl);
    __syncthreads();
    uint32_t total;
    const uint32_t before = block_scan_excl<kFaThreads>((uint32_t)__builtin_popcountll(keep), tmp, total);
    uint64_t pos = tile_off[blockIdx.x] + before;
    const uint64_t sepbits = hdr & c.nl;
    while (keep) {
        const int q = __builtin_ctzll(keep);
        out[pos] = base[off + q]; // from the cache: a register array indexed at run time would live in scratch
        if ((sepbits >> q) & 1ull) {
            const uint32_t i = atomicAdd(nseps, 1u);
            if (i < seps_cap) seps[i] = pos;
        }
        ++pos;
        keep &= keep - 1ull;
    }
}

size_t fasta_workspace_bytes(uint64_t n, size_t *o_summary, size_t *o_in, size_t *o_off, size_t *o_flags)
{
    const uint64_t ntiles = (n + kFaTile - 1) / kFaTile;
    auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    size_t o = 0;
    *o_summary = o; o += up((size_t)ntiles * 3 * 4);
    *o_in = o; o += up((size_t)ntiles * 4);
    *o_off = o; o += up((size_t)(ntiles + 1) * 8);
    *o_flags = o; o += 256; // [0] format flags, [1] separator count
    return o;
}

hipError_t launch_fasta_compact(const uint8_t *base, uint64_t n, uint8_t *ws, uint8_t *out, uint64_t *seps, uint32_t seps_cap, hipStream_t st)
{
    size_t os, oi, oo, of;
    fasta_workspace_bytes(n, &os, &oi, &oo, &of);
    const uint32_t ntiles = (uint32_t)((n + kFaTile - 1) / kFaTile);
    uint32_t *summary = (uint32_t *)(ws + os), *tin = (uint32_t *)(ws + oi), *flags = (uint32_t *)(ws + of);
    uint64_t *toff = (uint64_t *)(ws + oo);
    hipError_t e = hipMemsetAsync(flags, 0, 256, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(fasta_scan_kernel, dim3(ntiles), dim3(kFaThreads), 0, st, base, n, summary, flags);
    hipLaunchKernelGGL(fasta_offsets_kernel, dim3(1), dim3(kFaOffsetThreads), 0, st, summary, ntiles, tin, toff);
    hipLaunchKernelGGL(fasta_compact_kernel, dim3(ntiles), dim3(kFaThreads), 0, st, base, n, tin, toff, out, seps, seps_cap, flags + 1);
    return hipGetLastError();
}

} // namespace mhx
