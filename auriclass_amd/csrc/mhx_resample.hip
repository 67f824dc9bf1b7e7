// mhx_resample.hip -- one jackknife replicate of a sketch set on the device (mhx_resample_rows, mhx_dist_nj_support): the kept
// hashes of every row, compacted in order, and the cut of all rows to the smallest kept count of the full ones.  The rule and
// the steps of the compaction are the host+device functions of mhx_resample.h.  One workgroup per row; a row is taken in
// chunks of the workgroup's width -- coalesced 8-byte loads, a wave ballot of the keep flags, the set bits below a lane as its
// place in the wave, the waves' totals through LDS -- and the kept hashes of a chunk go out as one contiguous run of 8-byte
// stores.  The hand-off from the counts to the cut crosses a kernel boundary.  Next to the joins the work is nothing: not tuned.
#include "mhx_device.h"
#include "mhx_resample.h"

namespace mhx {

__global__ __launch_bounds__(kResampleThreads) void resample_kernel(const ResampleArgs a)
{
    __shared__ uint32_t wave_total[kResampleWaves];
    const uint32_t i = blockIdx.x, lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t full_len = a.len[i], len = full_len < a.stride ? full_len : a.stride; // a row ends at its stride, whatever len says
    const uint64_t *row = a.rows + (uint64_t)i * a.stride;
    uint64_t *out = a.out_rows + (uint64_t)i * a.stride;
    uint32_t kept = 0; // of the chunks so far (uniform)
    for (uint32_t c0 = 0; c0 < len; c0 += kResampleThreads) {
        const uint32_t j = c0 + threadIdx.x;
        const uint64_t h = j < len ? row[j] : 0;
        const bool keep = j < len && resample_keeps(h, a.seed, a.replicate, a.threshold);
        const uint64_t ballot = __ballot(keep);
        if (lane == 0) wave_total[wave] = resample_popcount(ballot);
        __syncthreads();
        uint32_t total;
        const uint32_t before = resample_wave_base(wave_total, wave, &total);
        if (keep) out[kept + before + resample_lane_rank(ballot, lane)] = h; // kept + before + rank < kept of the row <= len <= stride
        kept += total;
        __syncthreads(); // the totals are read before the next chunk writes them
    }
    if (threadIdx.x != 0) return;
    a.out_len[i] = kept;
    if (resample_full(full_len, a.s)) atomicMin(a.s_r, kept);
}

__global__ __launch_bounds__(kResampleThreads) void resample_clamp_kernel(const ResampleArgs a)
{
    const uint32_t i = blockIdx.x, s_r = *a.s_r, kept = a.out_len[i]; // every thread reads the length before thread 0 writes it:
    __syncthreads();                                                   // the barrier stands between the two
    const uint32_t len = kept < s_r ? kept : s_r;
    uint64_t *out = a.out_rows + (uint64_t)i * a.stride;
    for (uint32_t j = len + threadIdx.x; j < a.stride; j += kResampleThreads) out[j] = 0;
    if (threadIdx.x == 0) a.out_len[i] = len;
}

hipError_t launch_resample(const ResampleArgs &a, hipStream_t st)
{
    const hipError_t e = hipMemsetD32Async((hipDeviceptr_t)a.s_r, (int)a.s, 1, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(resample_kernel, dim3(a.n), dim3(kResampleThreads), 0, st, a);
    return hipGetLastError();
}
hipError_t launch_resample_clamp(const ResampleArgs &a, hipStream_t st)
{
    hipLaunchKernelGGL(resample_clamp_kernel, dim3(a.n), dim3(kResampleThreads), 0, st, a);
    return hipGetLastError();
}

} // namespace mhx
