// tests/emul/fasta_emul.cpp -- CPU emulator of the device FASTA parser (mhx_fasta.hip, test tool).
// Runs the host+device functions of auriclass_amd/csrc/mhx_fasta.h in the kernels' launch order: the scan kernel tile
// by tile (the 256 threads' load_chunk and chunk_state, the state scan as the kernel combines it -- per 64 lanes, then
// over the four wave totals --, the known / if-sequence / if-header counts), the one workgroup of the offsets pass with its
// share of tiles per thread, and the compaction.  Not part of the product; built by tests/test_fasta_emulation.py with g++.
#include <cstdint>
#include <vector>
#include "../../auriclass_amd/csrc/mhx_fasta.h"

using namespace mhx;

namespace {

// block_scan_state of mhx_fasta.hip: an inclusive scan by doubling steps inside every wave of 64 lanes (what the
// __shfl_up loop does), lane 0's exclusive value kPass, the waves' totals combined in order.  s: the threads' states, in:
// the state every thread starts in (kPass: no line starts in front of it inside the tile); returns the tile's end state.
uint32_t scan_states(const uint32_t (&s)[kFaThreads], uint32_t (&in)[kFaThreads])
{
    uint32_t incl[kFaThreads], tmp[kFaThreads / 64];
    for (int w = 0; w < kFaThreads / 64; ++w) {
        uint32_t *v = incl + 64 * w;
        for (int l = 0; l < 64; ++l) v[l] = s[64 * w + l];
        for (int o = 1; o < 64; o <<= 1) {
            uint32_t up[64];
            for (int l = 0; l < 64; ++l) up[l] = l >= o ? v[l - o] : v[l];
            for (int l = 0; l < 64; ++l)
                if (l >= o) v[l] = combine(up[l], v[l]);
        }
        tmp[w] = v[63];
    }
    uint32_t all = kPass;
    for (int t = 0; t < kFaThreads; ++t) {
        const int lane = t & 63, wave = t >> 6;
        const uint32_t excl = lane == 0 ? (uint32_t)kPass : incl[t - 1];
        uint32_t before = kPass;
        all = kPass;
        for (int w = 0; w < kFaThreads / 64; ++w) {
            if (w < wave) before = combine(before, tmp[w]);
            all = combine(all, tmp[w]);
        }
        in[t] = combine(before, excl);
    }
    return all;
}

} // namespace

// base: 16-byte aligned, readable up to n rounded up to 16 bytes (the device's contract).  out: room for out_cap bytes,
// seps: for seps_cap positions (unordered, as the device leaves them; *nseps counts all).  Returns 0, or 1 when a kept
// byte would land outside out (nothing is written there).
extern "C" int emul_fasta(const uint8_t *base, uint64_t n, uint8_t *out, uint64_t out_cap, uint64_t *total, uint64_t *seps, uint64_t seps_cap,
                          uint64_t *nseps, uint32_t *fastq_flag)
{
    const uint32_t ntiles = (uint32_t)((n + kFaTile - 1) / kFaTile);
    std::vector<uint32_t> summary(3 * (size_t)ntiles + 3), tile_in(ntiles + 1);
    std::vector<uint64_t> tile_off(ntiles + 1);
    uint32_t flags = 0, d[16];
    static uint32_t s[kFaThreads], st_in[kFaThreads];
    static ChunkMasks c[kFaThreads];
    // fasta_scan_kernel
    for (uint32_t b = 0; b < ntiles; ++b) {
        for (int t = 0; t < kFaThreads; ++t) {
            c[t] = load_chunk(base, (uint64_t)b * kFaTile + (uint64_t)t * kFaBytesPerThread, n, d);
            if (c[t].ls & c[t].fq) flags |= 1u;
            s[t] = chunk_state(c[t]);
        }
        const uint32_t tile_state = scan_states(s, st_in);
        uint32_t t_known = 0, t_seq = 0, t_hdr = 0;
        for (int t = 0; t < kFaThreads; ++t) {
            if (st_in[t] != kPass) t_known += (uint32_t)__builtin_popcountll(kept_mask(c[t], st_in[t]));
            else {
                t_seq += (uint32_t)__builtin_popcountll(kept_mask(c[t], kSeq));
                t_hdr += (uint32_t)__builtin_popcountll(kept_mask(c[t], kHdr));
            }
        }
        summary[3 * (size_t)b] = tile_state;
        summary[3 * (size_t)b + 1] = t_known + t_seq;
        summary[3 * (size_t)b + 2] = t_known + t_hdr;
    }
    // fasta_offsets_kernel
    {
        static uint32_t st[kFaOffsetThreads], in[kFaOffsetThreads];
        static unsigned long long sums[kFaOffsetThreads];
        for (uint32_t t = 0; t < (uint32_t)kFaOffsetThreads; ++t) st[t] = fa_span_state(summary.data(), fa_span(t, ntiles));
        for (uint32_t t = 0; t < (uint32_t)kFaOffsetThreads; ++t) {
            in[t] = fa_state_before(st, t);
            sums[t] = fa_walk_states(summary.data(), fa_span(t, ntiles), in[t], tile_in.data());
        }
        for (uint32_t t = 0; t < (uint32_t)kFaOffsetThreads; ++t) {
            unsigned long long before = 0;
            for (uint32_t i = 0; i < t; ++i) before += sums[i];
            before = fa_walk_offsets(summary.data(), fa_span(t, ntiles), in[t], before, tile_off.data());
            if (t == (uint32_t)kFaOffsetThreads - 1) tile_off[ntiles] = before;
        }
    }
    // fasta_compact_kernel
    uint64_t count = 0;
    int rc = 0;
    for (uint32_t b = 0; b < ntiles; ++b) {
        for (int t = 0; t < kFaThreads; ++t) {
            c[t] = load_chunk(base, (uint64_t)b * kFaTile + (uint64_t)t * kFaBytesPerThread, n, d);
            s[t] = chunk_state(c[t]);
        }
        scan_states(s, st_in);
        uint32_t before = 0;
        for (int t = 0; t < kFaThreads; ++t) {
            const uint64_t off = (uint64_t)b * kFaTile + (uint64_t)t * kFaBytesPerThread;
            const uint32_t state = st_in[t] == kPass ? tile_in[b] : st_in[t];
            const uint64_t hdr = header_mask(c[t], state);
            uint64_t keep = (~hdr & c[t].keepc) | (hdr & c[t].nl);
            uint64_t pos = tile_off[b] + before;
            before += (uint32_t)__builtin_popcountll(keep);
            const uint64_t sepbits = hdr & c[t].nl;
            while (keep) {
                const int q = __builtin_ctzll(keep);
                if (pos < out_cap) out[pos] = base[off + q];
                else rc = 1;
                if ((sepbits >> q) & 1ull) {
                    if (count < seps_cap) seps[count] = pos;
                    ++count;
                }
                ++pos;
                keep &= keep - 1ull;
            }
        }
    }
    *total = tile_off[ntiles];
    *nseps = count;
    *fastq_flag = flags & 1u;
    return rc;
}
