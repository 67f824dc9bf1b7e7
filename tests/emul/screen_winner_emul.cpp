// tests/emul/screen_winner_emul.cpp -- CPU emulator of the winner-take-all form of the containment screen (mhx_screen.hip:
// screen_winner_kernel, screen_tally_winner_kernel; mhx_engine.cpp: screener_winner_passes; test tool).  Runs the host+device
// functions of auriclass_amd/csrc/mhx_screen.h sequentially, in the engine's order: build, one probe per input hash, the plain
// tally's shared, the priority order, the claim of every entry (raise = a maximum taken by one agent), then per reference the
// winner form of the look-up and the four selection passes.  Not part of the product; built by
// tests/test_screen_winner_emulation.py with g++.
#include <cstdint>
#include <vector>
#include "../../auriclass_amd/csrc/mhx_screen.h"

using namespace mhx;

// rows [nr][stride] / len [nr] / length [nr] (may be null: all equal): the references; probes [nprobes]: the hash of every
// window.  Out: counts [nr][stride], shared [nr], median [nr] under winner-take-all, shared0 [nr] the plain shared, prio [nr].
// Returns the number of winner words that are not kScreenNobody (= distinct reference hashes found), or -1 when the build
// found no room.
extern "C" int64_t emul_screen_winner(const uint64_t *rows, const uint32_t *len, const uint64_t *length, uint32_t nr, uint32_t stride,
                                      const uint64_t *probes, uint64_t nprobes, uint32_t *counts, uint32_t *shared, uint32_t *median,
                                      uint32_t *shared0, uint32_t *prio)
{
    const uint64_t nslots = screen_table_slots((uint64_t)nr * stride);
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
    uint64_t maxkey = 0;
    for (uint64_t i = 0; i < nprobes; ++i) {
        const uint64_t h = probes[i];
        if (h > top) continue;
        if (h == kEmptyKey) { ++maxkey; continue; }
        const uint64_t at = screen_find(kp, mask, h);
        if (at != kScreenAbsent && screen_count_stands(cnts[at])) ++cnts[at];
    }
    // the plain tally's shared, the order it gives
    for (uint32_t r = 0; r < nr; ++r) {
        shared0[r] = 0;
        for (uint32_t j = 0; j < len[r]; ++j) shared0[r] += screen_count_of(kp, cnts.data(), mask, rows[(uint64_t)r * stride + j], maxkey) != 0u;
    }
    screen_priorities(shared0, len, length, nr, prio);
    // the winner pass
    std::vector<uint32_t> win(nslots + 1, kScreenNobody);
    uint32_t *wp = win.data();
    auto raise = [wp](uint64_t w, uint32_t p) { if (wp[w] < p) wp[w] = p; };
    for (uint32_t r = 0; r < nr; ++r)
        for (uint32_t j = 0; j < len[r]; ++j) screen_claim(kp, cnts.data(), mask, rows[(uint64_t)r * stride + j], maxkey, prio[r], raise);
    // the winner tally, one reference after the other
    for (uint32_t r = 0; r < nr; ++r) {
        uint32_t *out = counts + (uint64_t)r * stride;
        uint32_t nz = 0;
        for (uint32_t j = 0; j < len[r]; ++j) {
            out[j] = screen_count_won(kp, cnts.data(), wp, mask, rows[(uint64_t)r * stride + j], maxkey, prio[r]);
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
    int64_t claimed = 0;
    for (uint64_t i = 0; i <= nslots; ++i) claimed += win[i] != kScreenNobody;
    return claimed;
}
