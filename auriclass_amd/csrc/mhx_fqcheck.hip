// mhx_fqcheck.hip -- record check of a 4-line FASTQ span (rules and method: mhx_fqcheck.h).  Two launches on the
// engine stream, apart from the sketch kernel (which stays as it is):
//   fq_block_kernel   one workgroup per 256 KiB of the span: eight steps of 32 KiB staged in LDS, 16 B per lane,
//                     coalesced; each lane summarises its 128 contiguous bytes (read from padded
//                     LDS rows, free of bank conflicts), an in-order tree over the 256 lanes
//                     gives the step's summary, the steps are joined in order -> one summary per workgroup
//   fq_final_kernel   one workgroup: each lane joins a contiguous run of workgroup summaries, an in-order tree
//                     joins the lanes, lane 0 raises kFlagBadFastq in the sketcher's stats if the span fails
#include "mhx_device.h"
#include "mhx_fqcheck.h"

namespace mhx {

// in-order tree over the block's summaries in sm.red: red[0] = red[0] . red[1] . ... . red[kFqBlock - 1]
template <class I> __device__ __forceinline__ void fq_tree(FqSum<I> *red, int tid)
{
    for (int stride = 1; stride < kFqBlock; stride <<= 1) {
        __syncthreads();
        if ((tid & (2 * stride - 1)) == 0) red[tid] = fq_combine(red[tid], red[tid + stride]);
    }
    __syncthreads();
}

__global__ __launch_bounds__(kFqBlock) void fq_block_kernel(const uint8_t *base, uint64_t begin, uint64_t end, FqSum<int32_t> *out)
{
    __shared__ FqSmem sm;
    const int tid = threadIdx.x;
    const uint64_t lim = (end + 15) & ~(uint64_t)15;
    FqSum<int32_t> run = fq_identity<int32_t>();
    for (int step = 0; step < kFqTilesPerBlock; ++step) {
        const uint64_t tile_off = (uint64_t)blockIdx.x * kFqBlockBytes + (uint64_t)step * kFqTileBytes;
        if (tile_off >= end) break; // block-uniform
        fq_stage(sm, tid, base, tile_off, lim);
        __syncthreads();
        sm.red[tid] = fq_thread(sm, tid, tile_off, begin, end);
        fq_tree(sm.red, tid);
        if (tid == 0) run = fq_combine(run, sm.red[0]);
        // (the next step's staging writes sm.bytes only after every lane has passed fq_tree's last barrier)
    }
    if (tid == 0) out[blockIdx.x] = run;
}

__global__ __launch_bounds__(kFqBlock) void fq_final_kernel(const FqSum<int32_t> *in, uint32_t n, uint64_t *stats)
{
    __shared__ FqSum<int64_t> red[kFqBlock];
    const int tid = threadIdx.x;
    const uint32_t per = (n + kFqBlock - 1) / kFqBlock;
    const uint32_t lo = (uint32_t)tid * per, hi = lo + per < n ? lo + per : n;
    FqSum<int64_t> acc = fq_identity<int64_t>();
    uint32_t i = lo;
    for (; i + 4 <= hi; i += 4) { // four independent loads in flight, then the in-order joins
        const FqSum<int32_t> x0 = in[i], x1 = in[i + 1], x2 = in[i + 2], x3 = in[i + 3];
        acc = fq_combine(fq_combine(fq_combine(fq_combine(acc, x0), x1), x2), x3);
    }
    for (; i < hi; ++i) acc = fq_combine(acc, in[i]);
    red[tid] = acc;
    fq_tree(red, tid);
    if (tid == 0 && fq_span_bad(red[0]))
        atomicOr(reinterpret_cast<unsigned long long *>(stats) + kStatFlags, (unsigned long long)kFlagBadFastq);
}

uint32_t fastq_check_blocks(uint64_t begin, uint64_t end)
{
    (void)begin;
    return (uint32_t)((end + kFqBlockBytes - 1) / kFqBlockBytes);
}

hipError_t launch_fastq_check(const uint8_t *base, uint64_t begin, uint64_t end, void *scratch, uint64_t *stats, hipStream_t st)
{
    const uint32_t nblocks = fastq_check_blocks(begin, end);
    if (nblocks == 0) return hipSuccess;
    FqSum<int32_t> *sums = reinterpret_cast<FqSum<int32_t> *>(scratch);
    hipLaunchKernelGGL(fq_block_kernel, dim3(nblocks), dim3(kFqBlock), 0, st, base, begin, end, sums);
    hipLaunchKernelGGL(fq_final_kernel, dim3(1), dim3(kFqBlock), 0, st, (const FqSum<int32_t> *)sums, nblocks, stats);
    return hipGetLastError();
}

size_t fastq_check_scratch_bytes(uint64_t begin, uint64_t end) { return (size_t)fastq_check_blocks(begin, end) * sizeof(FqSum<int32_t>); }

} // namespace mhx
