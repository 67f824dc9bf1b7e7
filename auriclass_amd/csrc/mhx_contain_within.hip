// mhx_contain_within.hip -- all references a query holds on the device (mhx_dist_contain_within): the pass that takes a
// block's three counts per pair out of its block-local arrays into one cell per (query, slice) and an arrival list, and the
// gather that puts every hit in its final place.  The bounds, the finish pass and the pair kernel are those of
// mhx_contain.hip, writing block-local; the range pass is that of mhx_dist.hip; the scan of the cells into row_off is that of
// mhx_within.hip (launch_within_scan); the rules are the host+device functions of mhx_contain_within.h.
// Nothing is handed from one workgroup to another inside a kernel: the cells, the arrival list and row_off are written by one
// launch and read by a later one of the same stream, and the only word several waves touch at once is the arrival counter,
// through a device-scope atomicAdd whose return value is all a wave uses of it.
#include "mhx_device.h"
#include "mhx_block.h"
#include "mhx_contain_within.h"

namespace mhx {

// The thread mapping of within_take_kernel: thread id = (query ql, reference rl) of the block, so a half-wave is one (query,
// slice) and its half of the wave's ballot is the cell's mask (contain_within_ballot).  The keepers of both halves are
// appended with ONE atomic per wave, the lower half first, each in reference order (within_rank); a wave without keepers
// adds nothing.  Every cell of the block is written, an empty one too: a block that is redone later fills exactly the cells
// its first run left out.
__global__ __launch_bounds__(256) void contain_within_take_kernel(const ContainWithinOut o)
{
    if (*o.flag != 0) return; // the range pass gave this block up: the pair kernel redoes it, its take-out runs then
    const uint32_t id = blockIdx.x * 256 + threadIdx.x;
    const uint32_t ql = id / kTriSlice, rl = id % kTriSlice, lane = threadIdx.x & 63u;
    const bool live = ql < o.nq;
    uint32_t c = 0, b = 0;
    bool keep = false;
    if (live && rl < o.nr) {
        c = o.loc_shared[id];
        b = o.loc_n_ref[id];
        keep = contain_keep(c, b, o.need, o.need_limit);
    }
    const unsigned long long votes = __ballot(keep);
    const uint32_t word = (uint32_t)(votes >> (lane & 32u));
    uint32_t start = 0;
    if (o.base) { // (the same in every thread of the launch)
        uint32_t first = 0;
        if (lane == 0 && votes != 0) first = atomicAdd(o.count, (uint32_t)__popcll(votes));
        first = (uint32_t)__shfl((int)first, 0);
        start = first + ((lane & 32u) ? within_popc((uint32_t)votes) : 0u);
        if (keep) {
            const uint32_t at = start + within_rank(word, rl);
            if (at < o.room) { o.arr_shared[at] = c; o.arr_n_ref[at] = b; o.arr_n_qry[at] = o.loc_n_qry[id]; }
        }
    }
    if (live && rl == 0) within_cell_record(o.mask, o.base, within_cell(o.q0 + ql, o.r0, o.nslices), word, start);
}

// one workgroup per query, one thread per cell: the set bits of the cells before it (a workgroup scan, chunk by chunk) give
// within_dest, and the thread copies its up to 32 keepers from the arrival list, the reference from the bit's position
__global__ __launch_bounds__(256) void contain_within_gather_kernel(const ContainWithinRows o)
{
    __shared__ uint32_t wave_n[256 / 64];
    const uint32_t q = blockIdx.x;
    const uint64_t row_start = o.row_off[q];
    uint64_t carry = 0;
    for (uint32_t s0 = 0; s0 < o.nslices; s0 += 256) {
        const uint32_t sl = s0 + threadIdx.x;
        const uint64_t cell = (uint64_t)q * o.nslices + sl;
        uint32_t word = sl < o.nslices ? o.mask[cell] : 0u;
        const uint32_t n = within_popc(word);
        uint32_t total;
        const uint64_t before = carry + block_scan_excl<256>(n, wave_n, total);
        if (n) {
            const uint32_t start = o.base[cell];
            for (uint32_t rank = 0; rank < n; ++rank, word &= word - 1u) {
                const uint64_t to = within_dest(row_start, before, rank);
                const uint32_t from = start + rank;
                if (to >= o.cap || from >= o.room) continue;
                o.hit_ref[to] = sl * kTriSlice + (uint32_t)(__ffs((int)word) - 1);
                o.hit_shared[to] = o.arr_shared[from];
                o.hit_n_ref[to] = o.arr_n_ref[from];
                o.hit_n_qry[to] = o.arr_n_qry[from];
            }
        }
        carry += total;
        __syncthreads(); // the next chunk's scan writes wave_n again
    }
}

hipError_t launch_contain_within_take(const ContainWithinOut &o, hipStream_t st)
{
    if (o.nq == 0) return hipSuccess;
    hipLaunchKernelGGL(contain_within_take_kernel, dim3((o.nq * kTriSlice + 255) / 256), dim3(256), 0, st, o);
    return hipGetLastError();
}

hipError_t launch_contain_within_gather(const ContainWithinRows &o, hipStream_t st)
{
    if (o.nq == 0 || o.cap == 0 || !o.base) return hipSuccess;
    hipLaunchKernelGGL(contain_within_gather_kernel, dim3(o.nq), dim3(256), 0, st, o);
    return hipGetLastError();
}

} // namespace mhx
