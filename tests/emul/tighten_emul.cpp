// tests/emul/tighten_emul.cpp -- CPU emulator of the tighten pass's last workgroup (mhx_table.hip: table_tighten_kernel;
// test tool).  emul_tighten runs the host+device functions of auriclass_amd/csrc/mhx_tighten.h in the kernel's order:
// 256 threads of eight bins each, a prefix over the threads, the search inside the one thread that holds the cut, then
// thread 0's decision.  emul_tighten_former is the arithmetic the kernel carried inline before that header existed, kept
// here word for word as the statement of the rule.  Not part of the product; built by tests/test_tighten_emulation.py.
#include <cmath>
#include <cstdint>
#include "../../auriclass_amd/csrc/mhx_tighten.h"

using namespace mhx;

// state[0] = established, state[1] = bounded (in: before the pass, out: after it); returns the threshold after the pass
extern "C" uint64_t emul_tighten(const uint32_t *hist, uint64_t T, uint32_t sketch_size, uint32_t sample, uint32_t min_mult,
                                 uint64_t next_cap, uint64_t occupied, uint64_t solid, int *state)
{
    constexpr int kThreads = 256, kPer = kHistBins / kThreads;
    const int lz = tighten_lz(T);
    const uint32_t s = tighten_target(sketch_size, sample);
    uint32_t cut = kNoCut, before = 0;
    for (int t = 0; t < kThreads; ++t) {
        uint32_t mine = 0;
        for (int j = 0; j < kPer; ++j) mine += hist[kPer * t + j];
        if (before < s && before + mine >= s) cut = tighten_cut_among(hist + kPer * t, kPer, (uint32_t)(kPer * t), before, s);
        before += mine;
    }
    bool established = min_mult > 1 && state[0], bounded = false;
    const uint64_t now = tighten_threshold(T, lz, cut, min_mult, next_cap, occupied, solid, established, bounded);
    if (established) state[0] = 1;
    if (bounded) state[1] = 1;
    return now < T ? now : T;
}

extern "C" uint64_t emul_tighten_former(const uint32_t *hist, uint64_t T, uint32_t sketch_size, uint32_t sample, uint32_t min_mult,
                                        uint64_t next_cap, uint64_t occupied, uint64_t solid, int *state)
{
    const int lz = T ? __builtin_clzll(T) : 63;
    uint32_t s = sketch_size;
    if (sample > 1) {
        const float mean = (float)sketch_size / (float)sample;
        s = (uint32_t)(mean + 6.0f * sqrtf(mean)) + 16u;
    }
    uint32_t cut = 0xFFFFFFFFu, run = 0;
    for (int i = 0; i < kHistBins; ++i) { // first bin where the cumulative count reaches s
        if (run < s && run + hist[i] >= s) cut = (uint32_t)i;
        run += hist[i];
    }
    uint64_t now = T;
    bool established = min_mult > 1 && state[0];
    if (cut != 0xFFFFFFFFu && lz <= 52) {
        const uint64_t edge = (((uint64_t)cut + 1) << (53 - lz)) - 1; // last value of bin `cut`
        if (edge < T) {
            now = edge;
            if (min_mult > 1) { state[0] = 1; established = true; }
        }
    }
    if (next_cap && !established && !(occupied > 0 && solid * 5 >= occupied) && now > next_cap) {
        now = next_cap;
        state[1] = 1;
    }
    return now < T ? now : T;
}

// the bin of a hash <= T (the kernel's LDS histogram index) and its former spelling
extern "C" uint32_t emul_tighten_bin(uint64_t key, uint64_t T) { return tighten_bin(key, tighten_lz(T)); }
extern "C" uint32_t emul_tighten_bin_former(uint64_t key, uint64_t T)
{
    const int lz = T ? __builtin_clzll(T) : 63;
    return (uint32_t)((key << lz) >> (64 - 11));
}
