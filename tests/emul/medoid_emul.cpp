// tests/emul/medoid_emul.cpp -- CPU emulator of the medoid kernels (mhx_medoid.hip, test tool).  Runs the host+device functions
// of auriclass_amd/csrc/mhx_medoid.h themselves: the key, the label check, the block predicate next to a brute force over
// every cell, the sum pass cell by cell in the kernel's order with the wave's combine on arrays of 64 lanes, the pick, and
// the pair walk share by share as a workgroup of `shares` threads runs it.  The lanes and shares of a phase run in descending
// order: nothing in a phase may depend on the order.  Not part of the product; built by tests/test_medoid_emulation.py with g++.
#include <cstdint>
#include <vector>
#include "../../auriclass_amd/csrc/mhx_medoid.h"

using namespace mhx;

extern "C" uint64_t emul_medoid_key(uint64_t sum, uint32_t index) { return medoid_key(sum, index); }
extern "C" uint64_t emul_medoid_key_sum(uint64_t key) { return medoid_key_sum(key); }
extern "C" uint32_t emul_medoid_key_index(uint64_t key) { return medoid_key_index(key); }
extern "C" uint64_t emul_medoid_max_sum() { return kMedoidMaxSum; }
extern "C" uint32_t emul_medoid_pair_threads() { return kMedoidPairThreads; }
extern "C" uint32_t emul_medoid_first_bad_label(const uint32_t *label, uint32_t n) { return medoid_first_bad_label(label, n); }

// every block of the schedule at `qbatch`: runs[b] by the predicate, brute[b] by a look at every cell; returns their number
extern "C" uint32_t emul_medoid_blocks(const uint32_t *label, uint32_t n, uint32_t qbatch, uint8_t *runs, uint8_t *brute, uint32_t cap)
{
    std::vector<uint32_t> start((size_t)n + 1), member(n);
    medoid_members(label, n, start.data(), member.data());
    uint32_t nb = 0;
    TriBlock b;
    for (bool more = tri_first_block(n, qbatch, b); more; more = tri_next_block(n, qbatch, b), ++nb) {
        if (nb >= cap) continue;
        runs[nb] = medoid_block_runs(b, label, start.data(), member.data()) ? 1 : 0;
        bool any = false;
        for (uint32_t ql = 0; ql < b.nq && !any; ++ql)
            for (uint32_t rl = 0; rl < kTriSlice && !any; ++rl) any = medoid_cell_counts(b, ql, rl, label);
        brute[nb] = any ? 1 : 0;
    }
    return nb;
}

// The combine of one wave of tri_medoid_kernel: v [64] what the lanes hold (0 where their cell does not contribute), votes
// the ballot.  The exchanges run in lockstep over the arrays.  row [2] and ref [32] receive what the adders add (untouched
// where nothing is added); returns the number of adds.
static uint32_t wave_combine(const uint64_t *v, uint64_t votes, uint64_t *row, uint64_t *ref)
{
    uint64_t r[64], t[64];
    for (uint32_t l = 0; l < 64; ++l) r[l] = v[l];
    for (uint32_t x = kMedoidRowLanes / 2; x >= 1; x >>= 1) {
        for (uint32_t l = 0; l < 64; ++l) t[l] = r[l ^ x];
        for (uint32_t l = 64; l-- > 0;) r[l] += t[l];
    }
    uint32_t adds = 0;
    for (uint32_t l = 64; l-- > 0;) {
        const uint64_t both = v[l] + v[l ^ kMedoidRowLanes];
        if (medoid_row_adder(l) && medoid_row_any(votes, l) && r[l]) { row[l / kMedoidRowLanes] = r[l]; ++adds; }
        if (medoid_ref_adder(l) && medoid_ref_any(votes, l) && both) { ref[l] = both; ++adds; }
    }
    return adds;
}
extern "C" uint32_t emul_medoid_wave(const uint64_t *v, uint64_t votes, uint64_t *row, uint64_t *ref) { return wave_combine(v, votes, row, ref); }

// The sum pass over the blocks the predicate keeps, from the packed triangle (common, denom at tri_index): every wave of
// every launch in the kernel's cell order.  sum [n] zero on entry.  *adds: the adds of all waves, *most: of one wave.
extern "C" uint32_t emul_medoid_sums(const uint32_t *common, const uint32_t *denom, uint32_t n, int k, uint32_t qbatch, const uint32_t *label, uint64_t *sum,
                                     uint64_t *adds, uint32_t *most)
{
    std::vector<uint32_t> start((size_t)n + 1), member(n);
    medoid_members(label, n, start.data(), member.data());
    uint32_t run = 0;
    *adds = 0;
    *most = 0;
    TriBlock b;
    for (bool more = tri_first_block(n, qbatch, b); more; more = tri_next_block(n, qbatch, b)) {
        if (!medoid_block_runs(b, label, start.data(), member.data())) continue;
        ++run;
        const uint32_t cells = (b.nq * kTriSlice + 255) / 256 * 256;
        for (uint32_t w0 = 0; w0 < cells; w0 += 64) {
            uint64_t v[64], votes = 0, row[2] = {0, 0}, ref[32] = {};
            for (uint32_t l = 0; l < 64; ++l) {
                const uint32_t id = w0 + l, ql = id / kTriSlice, rl = id % kTriSlice;
                v[l] = 0;
                if (!medoid_cell_counts(b, ql, rl, label)) continue;
                votes |= 1ull << l;
                const uint64_t at = tri_index(b.q0 + ql, b.r0 + rl);
                v[l] = medoid_cell_value(common[at], denom[at], k);
            }
            if (votes == 0) continue;
            const uint32_t a = wave_combine(v, votes, row, ref);
            *adds += a;
            if (a > *most) *most = a;
            const uint32_t ql0 = w0 / kTriSlice;
            for (uint32_t h = 0; h < 2; ++h)
                if (row[h]) sum[b.q0 + ql0 + h] += row[h];
            for (uint32_t rl = 0; rl < kMedoidRowLanes; ++rl)
                if (ref[rl]) sum[b.r0 + rl] += ref[rl];
        }
    }
    return run;
}

// medoid_pick_kernel and medoid_write_kernel, the lists in descending order
extern "C" void emul_medoid_pick(const uint32_t *label, const uint64_t *sum, uint32_t n, uint32_t *medoid)
{
    std::vector<uint64_t> best(n, kMedoidNoKey);
    for (uint32_t i = n; i-- > 0;) {
        const uint64_t key = medoid_key(sum[i], i);
        if (key < best[label[i]]) best[label[i]] = key;
    }
    for (uint32_t i = n; i-- > 0;) medoid[i] = medoid_key_index(best[label[i]]);
}

// dist_to_kernel for one pair with a workgroup of `shares` threads: A the target's list, B the list itself
extern "C" void emul_medoid_pair(const uint64_t *A, uint32_t nA, const uint64_t *B, uint32_t nB, uint32_t shares, uint32_t s, uint32_t *common, uint32_t *denom)
{
    std::vector<uint32_t> u(shares), start(shares);
    for (uint32_t t = shares; t-- > 0;) u[t] = medoid_walk_distinct(A, nA, B, nB, shares, t);
    uint32_t distinct = 0;
    for (uint32_t t = 0; t < shares; ++t) { start[t] = distinct; distinct += u[t]; } // the block scan
    uint32_t c = 0;
    for (uint32_t t = shares; t-- > 0;) c += medoid_walk_common(A, nA, B, nB, shares, t, start[t], s);
    *common = c;
    *denom = medoid_denom(distinct, s);
}
