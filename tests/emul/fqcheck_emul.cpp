// tests/emul/fqcheck_emul.cpp -- CPU emulator of the FASTQ record check (mhx_fqcheck.hip, test tool).
// Runs the host+device functions of auriclass_amd/csrc/mhx_fqcheck.h in the kernels' order: per workgroup, the steps
// of 32 KiB, each staged lane by lane (both forms of fq_stage), summarised lane by lane and joined by the same in-order
// tree; then the final kernel's per-lane runs of workgroup summaries and its tree.  Not part of the product; built by
// tests/test_fastq_check_emulation.py with g++.
#include <cstdint>
#include <cstring>
#include <vector>
#include "../../auriclass_amd/csrc/mhx_fqcheck.h"

using namespace mhx;

template <class I> static void tree(FqSum<I> *red)
{
    for (int stride = 1; stride < kFqBlock; stride <<= 1)
        for (int tid = 0; tid < kFqBlock; tid += 2 * stride) red[tid] = fq_combine(red[tid], red[tid + stride]);
}

// 1: the span [begin, end) of base fails the check (kFlagBadFastq), 0: it passes.  base must be readable up to end
// rounded up to 16 bytes, as on the device.
extern "C" int emul_fqcheck(const uint8_t *base, uint64_t begin, uint64_t end)
{
    static FqSmem sm;
    const uint64_t lim = (end + 15) & ~(uint64_t)15;
    const uint32_t nblocks = (uint32_t)((end + kFqBlockBytes - 1) / kFqBlockBytes);
    std::vector<FqSum<int32_t>> sums(nblocks);
    for (uint32_t b = 0; b < nblocks; ++b) {
        FqSum<int32_t> run = fq_identity<int32_t>();
        for (int step = 0; step < kFqTilesPerBlock; ++step) {
            const uint64_t tile_off = (uint64_t)b * kFqBlockBytes + (uint64_t)step * kFqTileBytes;
            if (tile_off >= end) break;
            for (int tid = 0; tid < kFqBlock; ++tid) fq_stage(sm, tid, base, tile_off, lim);
            for (int tid = 0; tid < kFqBlock; ++tid) sm.red[tid] = fq_thread(sm, tid, tile_off, begin, end);
            tree(sm.red);
            run = fq_combine(run, sm.red[0]);
        }
        sums[b] = run;
    }
    static FqSum<int64_t> red[kFqBlock];
    const uint32_t per = (nblocks + kFqBlock - 1) / kFqBlock;
    for (int tid = 0; tid < kFqBlock; ++tid) {
        const uint32_t lo = (uint32_t)tid * per, hi = lo + per < nblocks ? lo + per : nblocks;
        FqSum<int64_t> acc = fq_identity<int64_t>();
        uint32_t i = lo;
        for (; i + 4 <= hi; i += 4)
            acc = fq_combine(fq_combine(fq_combine(fq_combine(acc, sums[i]), sums[i + 1]), sums[i + 2]), sums[i + 3]);
        for (; i < hi; ++i) acc = fq_combine(acc, sums[i]);
        red[tid] = acc;
    }
    tree(red);
    return nblocks && fq_span_bad(red[0]) ? 1 : 0;
}
