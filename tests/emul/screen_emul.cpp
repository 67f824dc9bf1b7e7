// tests/emul/screen_emul.cpp -- CPU emulator of the containment screen's table (mhx_screen.hip: screen_build_kernel,
// ScreenProber, screen_tally_kernel; test tool).  Runs the host+device functions of auriclass_amd/csrc/mhx_screen.h
// sequentially, in the kernels' order: vacate and build (claim = a compare-and-swap done by one agent), one probe per
// input hash, then per reference the look-up of every entry and the four selection passes over the counts.  Not part of
// the product; built by tests/test_screen_emulation.py with g++.
#include <cstdint>
#include <vector>
#include "../../auriclass_amd/csrc/mhx_screen.h"

using namespace mhx;

// rows [nr][stride] / len [nr]: the reference hash lists; probes [nprobes]: the hash of every admitted window.
// slots: 0 = sized by screen_table_slots(nr * stride), else the table size to use (a power of two that holds the keys).
// Out: counts [nr][stride], shared [nr], median [nr], t_screen.  Returns the number of occupied slots, or -1 when the
// build found no room, -2 when a counter reached its limit.
extern "C" int64_t emul_screen(const uint64_t *rows, const uint32_t *len, uint32_t nr, uint32_t stride, const uint64_t *probes,
                               uint64_t nprobes, uint64_t slots, uint32_t *counts, uint32_t *shared, uint32_t *median, uint64_t *t_screen)
{
    const uint64_t nslots = slots ? slots : screen_table_slots((uint64_t)nr * stride);
    const uint64_t mask = nslots - 1;
    std::vector<uint64_t> keys(nslots, kEmptyKey);
    std::vector<uint32_t> cnts(nslots, 0);
    uint64_t *kp = keys.data();
    auto claim = [kp](uint64_t slot, uint64_t h) {
        const uint64_t prev = kp[slot];
        if (prev == kEmptyKey) kp[slot] = h;
        return prev;
    };
    uint64_t top = 0;
    for (uint32_t r = 0; r < nr; ++r)
        for (uint32_t j = 0; j < len[r]; ++j) {
            const uint64_t h = rows[(uint64_t)r * stride + j];
            top = h > top ? h : top;
            if (h != kEmptyKey && screen_insert(mask, h, claim) == kScreenAbsent) return -1;
        }
    *t_screen = top;
    // the prober: the kernel hands it every window whose hash is <= T_screen
    uint64_t maxkey = 0;
    bool wrapped = false;
    for (uint64_t i = 0; i < nprobes; ++i) {
        const uint64_t h = probes[i];
        if (h > top) continue;
        if (h == kEmptyKey) { ++maxkey; continue; }
        const uint64_t at = screen_find(kp, mask, h);
        if (at == kScreenAbsent) continue;
        if (screen_count_stands(cnts[at])) ++cnts[at]; else wrapped = true;
    }
    // the tally, one reference after the other
    for (uint32_t r = 0; r < nr; ++r) {
        uint32_t *out = counts + (uint64_t)r * stride;
        uint32_t nz = 0;
        for (uint32_t j = 0; j < len[r]; ++j) {
            out[j] = screen_count_of(kp, cnts.data(), mask, rows[(uint64_t)r * stride + j], maxkey);
            nz += out[j] != 0u;
        }
        shared[r] = nz;
        median[r] = 0;
        if (!nz) continue;
        uint32_t prefix = 0, rank = nz / 2;
        for (int shift = 24; shift >= 0; shift -= 8) {
            uint32_t hist[kScreenSelectBins] = {0};
            for (uint32_t j = 0; j < len[r]; ++j)
                if (screen_select_match(out[j], prefix, shift)) ++hist[screen_select_digit(out[j], shift)];
            prefix = (prefix << 8) | screen_select_step(hist, rank);
        }
        median[r] = prefix;
    }
    if (wrapped) return -2;
    int64_t occupied = 0;
    for (uint64_t i = 0; i < nslots; ++i) occupied += keys[i] != kEmptyKey;
    return occupied;
}

extern "C" uint64_t emul_screen_table_slots(uint64_t entries) { return screen_table_slots(entries); }
