// tests/emul/segsketch_emul.cpp -- the segmented sketch kernel (auriclass_amd/csrc/mhx_segsketch.hip) run on the CPU: the
// very phase functions of mhx_segsketch.h, thread by thread, a loop over the threads standing for every __syncthreads().
// Segments above the cut are the host's share there and here: their len comes back as 0xFFFFFFFF.
// Not part of the product; built by tests/test_segsketch_emulation.py with g++.
#include <cstdint>
#include <cstring>
#include <memory>

#include "../../auriclass_amd/csrc/mhx_segsketch.h"

using namespace mhx;

template <int K>
static void run_segment(SegSmem &sm, const uint8_t *bytes, const uint64_t *seg_off, uint32_t seg, uint32_t s, uint64_t *rows, uint32_t *len,
                        uint32_t stride)
{
    const uint64_t b = seg_off[seg], e = seg_off[seg + 1];
    const uint64_t windows64 = seg_windows(b, e, K);
    if (!seg_is_small(windows64)) { len[seg] = 0xFFFFFFFFu; return; }
    if (windows64 == 0) { len[seg] = 0; return; }
    const uint32_t windows = (uint32_t)windows64, nsort = seg_sort_size(windows);
    const uint8_t *first = bytes + b;
    for (uint32_t tid = 0; tid < kSegBlock; ++tid) seg_phase_stage(sm, tid, first, (uint32_t)(e - b));
    for (uint32_t tid = 0; tid < kSegBlock; ++tid) seg_phase_hash<K>(sm, tid, seg_misalign(first), windows, nsort);
    for (uint32_t size = 2; size <= nsort; size <<= 1)
        for (uint32_t step = size >> 1; step > 0; step >>= 1)
            for (uint32_t tid = 0; tid < kSegBlock; ++tid) seg_sort_step(sm, tid, nsort, size, step);
    for (uint32_t tid = 0; tid < kSegBlock; ++tid) seg_phase_count(sm, tid, nsort);
    for (uint32_t tid = 0; tid < kSegBlock; ++tid) seg_phase_write(sm, tid, nsort, s < stride ? s : stride, rows + (uint64_t)seg * stride, len + seg);
}

extern "C" uint32_t emul_seg_cut(void) { return kSegCut; }
extern "C" uint32_t emul_seg_sort_size(uint32_t windows) { return seg_sort_size(windows); }

// bytes: the stream, with at least 4 readable bytes in front of it and behind it (the kernel stages whole aligned dwords)
extern "C" int emul_segsketch(int k, const uint8_t *bytes, const uint64_t *seg_off, uint32_t n_seg, uint32_t s, uint64_t *rows, uint32_t *len,
                              uint32_t stride)
{
    std::unique_ptr<SegSmem> sm(new SegSmem);
    for (uint32_t seg = 0; seg < n_seg; ++seg) {
        memset(sm.get(), 0xA5, sizeof(SegSmem)); // LDS is not cleared between workgroups
        switch (k) {
#define X(KK) case KK: run_segment<KK>(*sm, bytes, seg_off, seg, s, rows, len, stride); break;
            X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10) X(11) X(12) X(13) X(14) X(15) X(16)
            X(17) X(18) X(19) X(20) X(21) X(22) X(23) X(24) X(25) X(26) X(27) X(28) X(29) X(30) X(31) X(32)
#undef X
        default: return -1;
        }
    }
    return 0;
}
