// mhx_screen.hip -- kernels of the containment screen: the screen table of a reference set is built and cleared here,
// and what the reads left in it is tallied per reference.  The rules (probe sequence, count, winner, median selection
// steps) are the host+device functions of mhx_screen.h; the kernels that probe the table while reading are the PROBE
// forms of the sketch tile kernel (mhx_sketch.hip).
#include "mhx_device.h"
#include "mhx_screen.h"

namespace mhx {

// ---------------------------------------------------------------------------------------
// Containment screen (mhx_screen.h).  Build: the table is vacated by one kernel and filled by the next (a CAS claims a slot,
// duplicates across references meet the key they share); T_screen = the largest reference hash, one atomic per thread.
// Clear: counters and control words to zero, keys kept.  Tally: one workgroup per reference looks every entry up, writes
// its count, counts the non-zero ones and selects their median by four histogram passes over the counts it has written.
// Winner-take-all: a grid-stride pass over the entries raises a winner word per key, then the tally in its winner form.
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void screen_vacate_kernel(const ScreenArgs a)
{
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.nslots; i += (uint64_t)gridDim.x * blockDim.x) a.keys[i] = kEmptyKey;
    if (blockIdx.x == 0 && threadIdx.x == 0) *a.thresh = 0;
}

__global__ __launch_bounds__(256) void screen_clear_kernel(const ScreenArgs a, uint32_t *tickets, uint32_t ntickets, uint32_t *need_lookback)
{
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.nslots; i += (uint64_t)gridDim.x * blockDim.x) a.cnts[i] = 0;
    if (blockIdx.x == 0) {
        for (uint32_t i = threadIdx.x; i < (uint32_t)(kStatReplicas * kStatCount); i += blockDim.x) a.stats[i] = 0;
        for (uint32_t i = threadIdx.x; i < ntickets; i += blockDim.x) tickets[i] = 0;
        if (threadIdx.x == 0) *need_lookback = 0;
    }
}

__global__ __launch_bounds__(256) void screen_build_kernel(const ScreenArgs a)
{
    unsigned long long *keys = reinterpret_cast<unsigned long long *>(a.keys);
    auto claim = [keys](uint64_t slot, uint64_t h) { return (uint64_t)atomicCAS(&keys[slot], (unsigned long long)kEmptyKey, (unsigned long long)h); };
    const uint64_t total = (uint64_t)a.nr * a.stride;
    uint64_t top = 0;
    bool any = false;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t r = (uint32_t)(i / a.stride), j = (uint32_t)(i % a.stride);
        if (j >= a.len[r]) continue;
        const uint64_t h = a.rows[i];
        any = true;
        top = h > top ? h : top;
        if (h != kEmptyKey && screen_insert(a.nslots - 1, h, claim) == kScreenAbsent)
            atomicOr(reinterpret_cast<unsigned long long *>(a.stats) + kStatFlags, (unsigned long long)kFlagTableFull);
    }
    if (any) atomicMax(reinterpret_cast<unsigned long long *>(a.thresh), (unsigned long long)top);
}

__global__ __launch_bounds__(256) void screen_tally_kernel(const ScreenArgs a)
{
    __shared__ uint32_t hist[kScreenSelectBins];
    __shared__ unsigned long long maxkey_s;
    __shared__ uint32_t shared_s, prefix_s, rank_s;
    const uint32_t r = blockIdx.x, n = a.len[r] < a.stride ? a.len[r] : a.stride, tid = threadIdx.x;
    const uint64_t *row = a.rows + (uint64_t)r * a.stride;
    uint32_t *out = a.counts + (uint64_t)r * a.stride;
    if (tid == 0) { maxkey_s = 0; shared_s = 0; }
    __syncthreads();
    if (tid < kStatReplicas) {
        const uint64_t c = a.stats[tid * kStatCount + kStatMaxKey];
        if (c) atomicAdd(&maxkey_s, (unsigned long long)c);
    }
    __syncthreads();
    const uint64_t maxkey = maxkey_s;
    uint32_t nz = 0;
    for (uint32_t i = tid; i < n; i += blockDim.x) {
        const uint32_t c = screen_count_of(a.keys, a.cnts, a.nslots - 1, row[i], maxkey);
        out[i] = c;
        nz += c != 0u ? 1u : 0u;
    }
    if (nz) atomicAdd(&shared_s, nz);
    __syncthreads(); // (also: every count of this row is written and visible to the workgroup)
    const uint32_t shared = shared_s;
    if (tid == 0) { a.shared[r] = shared; prefix_s = 0; rank_s = shared / 2; }
    if (shared == 0) {
        if (tid == 0) a.median[r] = 0;
        return;
    }
    for (int shift = 24; shift >= 0; shift -= 8) {
        for (uint32_t i = tid; i < (uint32_t)kScreenSelectBins; i += blockDim.x) hist[i] = 0;
        __syncthreads();
        const uint32_t prefix = prefix_s;
        for (uint32_t i = tid; i < n; i += blockDim.x) {
            const uint32_t c = out[i];
            if (screen_select_match(c, prefix, shift)) atomicAdd(&hist[screen_select_digit(c, shift)], 1u);
        }
        __syncthreads();
        if (tid == 0) {
            uint32_t rank = rank_s;
            const uint32_t d = screen_select_step(hist, rank);
            rank_s = rank;
            prefix_s = (prefix << 8) | d;
        }
        __syncthreads();
    }
    if (tid == 0) a.median[r] = prefix_s;
}

// The tally's winner-take-all form: a count is kept only where this reference won the key (win / prio: mhx_screen.h,
// screen_count_won); everything else -- one workgroup per reference, the four selection passes -- is screen_tally_kernel's
// text.  A kernel of its own and not a template parameter of that one, so that the plain tally stays, instruction for
// instruction, the code it was (as one template body its register allocation moved: profiles/screen_winner.txt).  The
// same holds for sharing less than the whole body: with the selection passes -- with or without the early-out in front of
// them, with the caller's LDS words or its own -- in one forced-inline function, and with one forced-inline body that
// takes the count rule as a functor, the plain tally went from 1153 to 1213 instructions and from 47 to 48 SGPRs (20
// VGPRs, 1048 bytes of LDS and no scratch either way; the winner form from 52 to 53 SGPRs): profiles/tu_split_isa.txt.
// So the median selection is written twice; a change to one is a change to both.
__global__ __launch_bounds__(256) void screen_tally_winner_kernel(const ScreenArgs a, const uint32_t *win, const uint32_t *prio)
{
    __shared__ uint32_t hist[kScreenSelectBins];
    __shared__ unsigned long long maxkey_s;
    __shared__ uint32_t shared_s, prefix_s, rank_s;
    const uint32_t r = blockIdx.x, n = a.len[r] < a.stride ? a.len[r] : a.stride, tid = threadIdx.x;
    const uint64_t *row = a.rows + (uint64_t)r * a.stride;
    uint32_t *out = a.counts + (uint64_t)r * a.stride;
    if (tid == 0) { maxkey_s = 0; shared_s = 0; }
    __syncthreads();
    if (tid < kStatReplicas) {
        const uint64_t c = a.stats[tid * kStatCount + kStatMaxKey];
        if (c) atomicAdd(&maxkey_s, (unsigned long long)c);
    }
    __syncthreads();
    const uint64_t maxkey = maxkey_s;
    const uint32_t mine = prio[r];
    uint32_t nz = 0;
    for (uint32_t i = tid; i < n; i += blockDim.x) {
        const uint32_t c = screen_count_won(a.keys, a.cnts, win, a.nslots - 1, row[i], maxkey, mine);
        out[i] = c;
        nz += c != 0u ? 1u : 0u;
    }
    if (nz) atomicAdd(&shared_s, nz);
    __syncthreads(); // (also: every count of this row is written and visible to the workgroup)
    const uint32_t shared = shared_s;
    if (tid == 0) { a.shared[r] = shared; prefix_s = 0; rank_s = shared / 2; }
    if (shared == 0) {
        if (tid == 0) a.median[r] = 0;
        return;
    }
    for (int shift = 24; shift >= 0; shift -= 8) {
        for (uint32_t i = tid; i < (uint32_t)kScreenSelectBins; i += blockDim.x) hist[i] = 0;
        __syncthreads();
        const uint32_t prefix = prefix_s;
        for (uint32_t i = tid; i < n; i += blockDim.x) {
            const uint32_t c = out[i];
            if (screen_select_match(c, prefix, shift)) atomicAdd(&hist[screen_select_digit(c, shift)], 1u);
        }
        __syncthreads();
        if (tid == 0) {
            uint32_t rank = rank_s;
            const uint32_t d = screen_select_step(hist, rank);
            rank_s = rank;
            prefix_s = (prefix << 8) | d;
        }
        __syncthreads();
    }
    if (tid == 0) a.median[r] = prefix_s;
}

// Winner pass: every valid reference entry whose key was seen raises the key's winner word to its reference's priority.
// win is at kScreenNobody when the kernel starts; the tally that reads it is the next kernel on the stream.
__global__ __launch_bounds__(256) void screen_winner_kernel(const ScreenArgs a, uint32_t *win, const uint32_t *prio, uint64_t maxkey)
{
    auto raise = [win](uint64_t w, uint32_t p) { atomicMax(&win[w], p); };
    const uint64_t total = (uint64_t)a.nr * a.stride;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t r = (uint32_t)(i / a.stride), j = (uint32_t)(i % a.stride);
        if (j >= a.len[r]) continue;
        screen_claim(a.keys, a.cnts, a.nslots - 1, a.rows[i], maxkey, prio[r], raise);
    }
}

static unsigned screen_blocks(uint64_t items)
{
    uint64_t blocks = (items + 256 * 8 - 1) / (256 * 8);
    return (unsigned)(blocks > 2048 ? 2048 : blocks < 1 ? 1 : blocks);
}

hipError_t launch_screen_clear(const ScreenArgs &a, uint32_t *tickets, uint32_t ntickets, uint32_t *need_lookback, hipStream_t st)
{
    hipLaunchKernelGGL(screen_clear_kernel, dim3(screen_blocks(a.nslots)), dim3(256), 0, st, a, tickets, ntickets, need_lookback);
    return hipGetLastError();
}

hipError_t launch_screen_build(const ScreenArgs &a, hipStream_t st)
{
    hipLaunchKernelGGL(screen_vacate_kernel, dim3(screen_blocks(a.nslots)), dim3(256), 0, st, a);
    if ((uint64_t)a.nr * a.stride) hipLaunchKernelGGL(screen_build_kernel, dim3(screen_blocks((uint64_t)a.nr * a.stride)), dim3(256), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_screen_tally(const ScreenArgs &a, hipStream_t st)
{
    if (a.nr) hipLaunchKernelGGL(screen_tally_kernel, dim3(a.nr), dim3(256), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_screen_winner(const ScreenArgs &a, uint32_t *win, const uint32_t *prio, uint64_t maxkey, hipStream_t st)
{
    const uint64_t total = (uint64_t)a.nr * a.stride;
    if (total) hipLaunchKernelGGL(screen_winner_kernel, dim3(screen_blocks(total)), dim3(256), 0, st, a, win, prio, maxkey);
    return hipGetLastError();
}

hipError_t launch_screen_tally_winner(const ScreenArgs &a, const uint32_t *win, const uint32_t *prio, hipStream_t st)
{
    if (a.nr) hipLaunchKernelGGL(screen_tally_winner_kernel, dim3(a.nr), dim3(256), 0, st, a, win, prio);
    return hipGetLastError();
}

} // namespace mhx
