// push_plan_emul.cpp -- the schedule of a sketcher push (auriclass_amd/csrc/mhx_push_plan.h, the very header push_span steps
// through) run on the host: a sequence of pushes on one sketcher's counters, every launch a row.  As a shared library for
// tests/test_push_plan.py (against tests/push_rule.py); with -DPUSH_PLAN_MAIN a program of its own for the sanitizer build.
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "../../auriclass_amd/csrc/mhx_push_plan.h"

using namespace mhx;

constexpr int kRowWords = 11; // push, tile0, ntiles, split, queue, cap_before, next_cap, verify_chain, bytes after, next chunk after, tiles of the push

extern "C" {

uint64_t emul_push_constant(int which)
{
    const uint64_t v[] = {(uint64_t)kMaxLaunchesPerPush, kChunkGrowth, kUncappedBytes, kDeviceOrderMinSketch, (uint64_t)kTileBytes, (uint64_t)kRowWords};
    return v[which];
}

uint64_t emul_first_chunk(uint32_t s, uint32_t m, uint64_t nslots) { return first_chunk_bytes(s, m, nslots); }

// (the rate as the screen-mode push forms it: T_screen / hash_max)
uint32_t emul_queue_form(int kfmt, uint32_t s, uint64_t num, uint64_t den, int forced) { return queue_form(kfmt, s, (long double)num / (long double)den, forced); }

// counters: {bytes_pushed, next_chunk_bytes, repair_bytes, repair_next_chunk_bytes}, as mhx_sketcher_reset leaves them or as
// earlier pushes did; push i is `n[i]` bytes that begin `begin[i]` (<= 15) bytes behind an aligned base, in kernel format
// kfmt[i], as a repair pass where repair[i].  Returns the launches (rows written, at most cap_rows), -1: out of rows.
int64_t emul_push_rows(uint32_t s, uint32_t m, uint64_t nslots, uint64_t hash_max, uint64_t admit_scale, int cu_count, const int32_t *kfmt,
                       const int32_t *repair, const uint64_t *begin, const uint64_t *n, uint64_t n_pushes, int force_queue, uint32_t force_split,
                       uint64_t *counters, uint64_t *rows, uint64_t cap_rows)
{
    const PushConsts c{s, m, nslots, hash_max, admit_scale};
    uint64_t at = 0;
    for (uint64_t i = 0; i < n_pushes; ++i) {
        const bool rep = repair[i] != 0;
        PushPlan plan(c, cu_count, kfmt[i], rep, begin[i], begin[i] + n[i], counters[rep ? 2 : 0], counters[rep ? 3 : 1], force_queue, force_split);
        for (PushStep st; plan.next(st); ++at) {
            if (at >= cap_rows) return -1;
            counters[rep ? 2 : 0] = st.bytes_pushed; // (what push_span does once the launch is on the stream)
            counters[rep ? 3 : 1] = st.next_chunk_bytes;
            uint64_t *r = rows + at * kRowWords;
            r[0] = i; r[1] = st.tile0; r[2] = st.ntiles; r[3] = st.split; r[4] = st.queue_candidates; r[5] = st.cap_before; r[6] = st.next_cap;
            r[7] = st.verify_chain; r[8] = counters[rep ? 2 : 0]; r[9] = counters[rep ? 3 : 1]; r[10] = span_tiles(begin[i] + n[i]);
        }
    }
    return (int64_t)at;
}

} // extern "C"

#ifdef PUSH_PLAN_MAIN
// The two long cases under the sanitizers: one 3 GB span, and a span of 70 tiles in 10-byte pushes; for m = 1 and 3, the
// three kernel formats and a repair pass.  Checks only what memory safety needs a witness for: the tiles add up.
static int run(uint32_t m, int kfmt, bool repair, uint64_t total, uint64_t piece)
{
    const uint32_t s = 1000;
    const uint64_t nslots = 1ull << 21;
    uint64_t counters[4] = {0, first_chunk_bytes(s, m, nslots), 0, first_chunk_bytes(s, m, nslots)};
    std::vector<uint64_t> rows((size_t)kMaxLaunchesPerPush * kRowWords);
    uint64_t tiles = 0, want_tiles = 0;
    for (uint64_t off = 0; off < total; off += piece) {
        const int32_t f = kfmt, r = repair;
        const uint64_t begin = off & 15, n = total - off < piece ? total - off : piece;
        const int64_t got = emul_push_rows(s, m, nslots, ~0ull, 1, 256, &f, &r, &begin, &n, 1, -1, 0, counters, rows.data(), kMaxLaunchesPerPush);
        if (got < 1 || got > kMaxLaunchesPerPush) { printf("m %u fmt %d: %lld launches in one push\n", m, kfmt, (long long)got); return 1; }
        for (int64_t i = 0; i < got; ++i) tiles += rows[(size_t)i * kRowWords + 2];
        want_tiles += span_tiles(begin + n);
    }
    if (tiles != want_tiles || counters[repair ? 2 : 0] != total) { printf("m %u fmt %d: %llu of %llu tiles\n", m, kfmt, (unsigned long long)tiles, (unsigned long long)want_tiles); return 1; }
    return 0;
}

int main()
{
    int bad = 0, cases = 0;
    for (uint32_t m : {1u, 3u, 5u})
        for (int kfmt = 0; kfmt < 3; ++kfmt)
            for (int repair = 0; repair < (kfmt == 1 ? 2 : 1); ++repair) {
                bad += run(m, kfmt, repair != 0, 3000000000ull, 3000000000ull);
                bad += run(m, kfmt, repair != 0, 70ull * kTileBytes - 3, 10);
                cases += 2;
            }
    if (bad) return 1;
    printf("ok %d\n", cases);
    return 0;
}
#endif
