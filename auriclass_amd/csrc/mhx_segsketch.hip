// mhx_segsketch.hip -- the segmented sketch kernel: one workgroup per segment of an MHX_FMT_SEQ stream, the segment's
// windows hashed, sorted and selected in LDS (phases and rules: mhx_segsketch.h).  Segments of more than kSegCut windows
// are left to the host (mhx_engine_segments.cpp), which runs them through the sketcher.
#include <hip/hip_runtime.h>

#include "mhx_device.h"
#include "mhx_segsketch.h"

namespace mhx {

template <int K>
__global__ __launch_bounds__(kSegBlock) void segsketch_kernel(const uint8_t *bytes, const uint64_t *seg_off, uint32_t s,
                                                              uint64_t *rows, uint32_t *len, uint32_t stride)
{
    __shared__ SegSmem sm;
    const uint32_t seg = blockIdx.x, tid = threadIdx.x;
    const uint64_t b = seg_off[seg], e = seg_off[seg + 1];
    const uint64_t windows64 = seg_windows(b, e, K);
    if (!seg_is_small(windows64)) return; // the host's share
    if (windows64 == 0) {
        if (tid == 0) len[seg] = 0;
        return;
    }
    const uint32_t windows = (uint32_t)windows64, nsort = seg_sort_size(windows);
    const uint8_t *first = bytes + b;
    seg_phase_stage(sm, tid, first, (uint32_t)(e - b));
    __syncthreads();
    seg_phase_hash<K>(sm, tid, seg_misalign(first), windows, nsort);
    __syncthreads();
    for (uint32_t size = 2; size <= nsort; size <<= 1)
        for (uint32_t step = size >> 1; step > 0; step >>= 1) {
            seg_sort_step(sm, tid, nsort, size, step);
            __syncthreads();
        }
    seg_phase_count(sm, tid, nsort);
    __syncthreads();
    seg_phase_write(sm, tid, nsort, s < stride ? s : stride, rows + (uint64_t)seg * stride, len + seg);
}

#ifdef MHX_ONLY_K   // experiment / ISA-study builds: one k-mer size
#define MHX_K_LIST(X) X(MHX_ONLY_K)
#else
#define MHX_K_LIST(X) X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10) X(11) X(12) X(13) X(14) X(15) X(16) \
    X(17) X(18) X(19) X(20) X(21) X(22) X(23) X(24) X(25) X(26) X(27) X(28) X(29) X(30) X(31) X(32)
#endif

hipError_t launch_segsketch(int k, const uint8_t *bytes, const uint64_t *seg_off, uint32_t n_seg, uint32_t s, uint64_t *rows,
                            uint32_t *len, uint32_t stride, hipStream_t st)
{
    if (n_seg == 0) return hipSuccess;
    if (n_seg > 0x7FFFFFFFu) return hipErrorInvalidValue;
    switch (k) {
#define X(KK) case KK: hipLaunchKernelGGL((segsketch_kernel<KK>), dim3(n_seg), dim3(kSegBlock), 0, st, bytes, seg_off, s, rows, len, stride); break;
        MHX_K_LIST(X)
#undef X
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

} // namespace mhx
