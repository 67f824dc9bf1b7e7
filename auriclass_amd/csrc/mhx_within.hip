// mhx_within.hip -- all references within a distance of each query on the device (mhx_dist_within): the pass that takes a
// block's results out of its block-local arrays into one cell per (query, slice) and an arrival list, the scan of the cells
// into row_off, and the gather that puts every hit in its final place.  The range pass and the finish passes are those of
// mhx_dist.hip and mhx_triangle.hip; the rules are the host+device functions of mhx_within.h.
// Nothing is handed from one workgroup to another inside a kernel: the cells, the arrival list and row_off are written by one
// launch and read by a later one of the same stream, and the only word several waves touch at once is the arrival counter,
// through a device-scope atomicAdd whose return value is all a wave uses of it.
#include "mhx_device.h"
#include "mhx_within.h"

namespace mhx {

// The cells of tri_cluster_kernel: thread id = (query ql, reference rl) of the block, so a half-wave is one (query, slice)
// and its half of the wave's ballot is the cell's mask (within_ballot).  The keepers of both halves are appended with ONE
// atomic per wave, the lower half first, each in reference order (within_rank); a wave without keepers adds nothing.  Every
// cell of the block is written, an empty one too: a block that is redone later fills exactly the cells its first run left out.
__global__ __launch_bounds__(256) void within_take_kernel(const WithinOut o)
{
    if (*o.flag != 0) return; // the range pass gave this block up: the generic kernel redoes it, its take-out runs then
    const uint32_t id = blockIdx.x * 256 + threadIdx.x;
    const uint32_t ql = id / kTriSlice, rl = id % kTriSlice, lane = threadIdx.x & 63u;
    const bool live = ql < o.nq;
    uint32_t c = 0, d = 0;
    bool keep = false;
    if (live && rl < o.nr) {
        c = o.loc_common[id];
        d = o.loc_denom[id];
        keep = cluster_keep(c, d, o.cmin, o.s);
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
            if (at < o.room) { o.arr_common[at] = c; o.arr_denom[at] = d; }
        }
    }
    if (live && rl == 0) within_cell_record(o.mask, o.base, within_cell(o.q0 + ql, o.r0, o.nslices), word, start);
}

// inclusive scan over the 256 threads of a workgroup; buf [256] may be used again after the call
template <class T> __device__ __forceinline__ T block_scan(T v, T *buf, T &total)
{
    const uint32_t t = threadIdx.x;
    buf[t] = v;
    __syncthreads();
    for (uint32_t off = 1; off < 256; off <<= 1) {
        const T x = t >= off ? buf[t - off] : (T)0;
        __syncthreads();
        buf[t] += x;
        __syncthreads();
    }
    const T mine = buf[t];
    total = buf[255];
    __syncthreads();
    return mine;
}

// one workgroup per query: within_row_count of its cells into row_off[q + 1]
__global__ __launch_bounds__(256) void within_count_kernel(const WithinRows o)
{
    __shared__ uint64_t buf[256];
    const uint32_t q = blockIdx.x;
    const uint32_t *row = o.mask + (uint64_t)q * o.nslices;
    uint64_t n = 0;
    for (uint32_t i = threadIdx.x; i < o.nslices; i += 256) n += within_popc(row[i]);
    uint64_t total;
    block_scan(n, buf, total);
    if (threadIdx.x == 0) o.row_off[q + 1] = total;
}

// ONE workgroup: the counts of the super-batch's queries, in index order, become the running sum on top of row_off[0]
__global__ __launch_bounds__(256) void within_offsets_kernel(const WithinRows o)
{
    __shared__ uint64_t buf[256];
    uint64_t carry = o.row_off[0];
    for (uint32_t q0 = 0; q0 < o.nq; q0 += 256) {
        const uint32_t q = q0 + threadIdx.x;
        uint64_t total;
        const uint64_t incl = block_scan(q < o.nq ? o.row_off[q + 1] : (uint64_t)0, buf, total);
        if (q < o.nq) o.row_off[q + 1] = carry + incl;
        carry += total;
    }
}

// one workgroup per query, one thread per cell: the set bits of the cells before it (a scan, chunk by chunk) give
// within_dest, and the thread copies its up to 32 keepers from the arrival list, the reference from the bit's position
__global__ __launch_bounds__(256) void within_gather_kernel(const WithinRows o)
{
    __shared__ uint32_t buf[256];
    const uint32_t q = blockIdx.x;
    const uint64_t row_start = o.row_off[q];
    uint64_t carry = 0;
    for (uint32_t s0 = 0; s0 < o.nslices; s0 += 256) {
        const uint32_t sl = s0 + threadIdx.x;
        const uint64_t cell = (uint64_t)q * o.nslices + sl;
        uint32_t word = sl < o.nslices ? o.mask[cell] : 0u;
        const uint32_t n = within_popc(word);
        uint32_t total;
        const uint32_t incl = block_scan(n, buf, total);
        if (n) {
            const uint64_t before = carry + incl - n;
            const uint32_t start = o.base[cell];
            for (uint32_t rank = 0; rank < n; ++rank, word &= word - 1u) {
                const uint64_t to = within_dest(row_start, before, rank);
                const uint32_t from = start + rank;
                if (to >= o.cap || from >= o.room) continue;
                const uint32_t c = o.arr_common[from], d = o.arr_denom[from];
                o.hit_ref[to] = sl * kTriSlice + (uint32_t)(__ffs((int)word) - 1);
                o.hit_common[to] = c;
                o.hit_denom[to] = d;
                if (o.hit_dist) o.hit_dist[to] = tri_distance(c, d, o.k);
            }
        }
        carry += total;
    }
}

hipError_t launch_within_take(const WithinOut &o, hipStream_t st)
{
    if (o.nq == 0) return hipSuccess;
    hipLaunchKernelGGL(within_take_kernel, dim3((o.nq * kTriSlice + 255) / 256), dim3(256), 0, st, o);
    return hipGetLastError();
}

hipError_t launch_within_scan(const WithinRows &o, hipStream_t st)
{
    if (o.nq == 0) return hipSuccess;
    hipLaunchKernelGGL(within_count_kernel, dim3(o.nq), dim3(256), 0, st, o);
    hipLaunchKernelGGL(within_offsets_kernel, dim3(1), dim3(256), 0, st, o);
    return hipGetLastError();
}

hipError_t launch_within_gather(const WithinRows &o, hipStream_t st)
{
    if (o.nq == 0 || o.cap == 0 || !o.base) return hipSuccess;
    hipLaunchKernelGGL(within_gather_kernel, dim3(o.nq), dim3(256), 0, st, o);
    return hipGetLastError();
}

} // namespace mhx
