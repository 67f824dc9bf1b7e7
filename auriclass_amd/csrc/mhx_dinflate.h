// mhx_dinflate.h -- per-lane logic of the device DEFLATE decoder (mhx_dinflate.hip), written as host+device inline
// functions in the way of mhx_tile.h: the kernels call them one lane per segment or candidate position, and the CPU
// emulator (tests/emul/dinflate_emul.cpp) runs the very same functions, and the very same round driver, lane by lane.
//
// One gzip member on the device (the design of the host's mhx_pinflate.cpp, moved to many more lanes):
//   search     the member is cut at target bit offsets (seg_bits apart); for each target the first later bit position
//              (below the next target) where a dynamic-Huffman block header is valid -- BTYPE 2, HLIT/HDIST in range, a
//              complete code-length code, complete literal/length and distance codes, an end-of-block code -- becomes a
//              segment start.  Lanes test consecutive positions.  Segment 0 starts at the true start.
//   decode     each segment is decoded by one lane into 16-bit symbols: a byte, or kMarker | w = "byte w of the unknown
//              32 KiB in front of the segment".  Blocks are decoded while their header lies before the next segment's
//              start, so a segment ends on a block boundary at or past its successor's start; it records that bit, its
//              symbol count and whether it saw the final block.  The count stays exact when the symbol slab is full.
//   chain      segment j is right if segment j-1 is right and stopped exactly where j started (segment 0 is right:
//              induction).  A broken link is redone from where the predecessor stopped, at most kMaxPasses times.
//   resolve    markers read the output in front of the segment: first the last 32 KiB of every segment, in order (one
//              workgroup walks the chain), then everything else in parallel.
//   crc        CRC-32 per segment on the device; the host joins them (crc32_combine) and checks the trailer.
// Work goes in rounds (search, decode, chain, resolve, CRC each), so device memory stays bounded for any member: a round's
// first segment starts where the previous round verifiably stopped, its markers read the previous round's output.  The
// first round is small and each further one twice as large, up to a bound, so a small member costs one small round.
//
// Robustness: every loop is bounded by input bits or output capacity, reads past the input return zero bits and are
// reported, every table index is masked or checked.  A failure of any kind is reported to the caller, whose rule is
// that the host decoder then has the last word.
#pragma once
#include <stdint.h>
#include <string.h>

#include "mhx_deflate.h"

#include <algorithm>
#include <vector>

namespace mhx {
namespace dinf {

using namespace deflate;

constexpr uint32_t kWin = 32768;
constexpr uint16_t kMarker = 0x8000;
constexpr uint64_t kNoBit = ~0ull;         // "no candidate" / "no stop target"
constexpr int kLaneWords = kLitCap + kDistCap + kLensBytes / 4; // per-lane workspace: both tables and the code lengths
constexpr int kMaxPasses = 16;

// segment status
enum : uint32_t { kSegOk = 0, kSegData = 1, kSegEnd = 2 };

// ---- bit input: reads past the n bytes return zero bits; pos() > 8 n tells that it happened ----
struct Bits {
    const uint8_t *p;
    uint64_t n;    // bytes of input
    uint64_t next; // next byte to load
    uint64_t buf;
    int cnt;
    MHX_HD void refill()
    {
        if (next + 8 <= n) {
            uint64_t v;
            memcpy(&v, p + next, 8);
            buf |= v << cnt;
            next += (uint64_t)((63 - cnt) >> 3);
            cnt |= 56;
        } else {
            while (cnt <= 56) {
                const uint64_t b = next < n ? p[next] : 0;
                buf |= b << cnt;
                ++next;
                cnt += 8;
            }
        }
    }
    MHX_HD void seek(uint64_t bit)
    {
        next = bit >> 3;
        buf = 0;
        cnt = 0;
        refill();
        drop((int)(bit & 7));
    }
    MHX_HD uint32_t peek(int k) const { return (uint32_t)(buf & ((1ull << k) - 1)); }
    MHX_HD void drop(int k) { buf >>= k; cnt -= k; }
    MHX_HD uint32_t take(int k)
    {
        if (cnt < k) refill();
        const uint32_t v = peek(k);
        drop(k);
        return v;
    }
    MHX_HD uint64_t pos() const { return next * 8 - (uint64_t)cnt; }
    MHX_HD bool overrun() const { return pos() > n * 8; }
    MHX_HD bool fill(int k) // read_dynamic's refill: reads past the input are harmless here, its overrun() tests catch them
    {
        if (cnt < k) refill();
        return true;
    }
};

// Search test: is `bit` the start of a dynamic-Huffman block header that a real encoder could have written?
MHX_HD bool header_candidate(const uint8_t *in, uint64_t n, uint64_t bit)
{
    Bits b{in, n, 0, 0, 0};
    b.seek(bit);
    b.drop(1); // BFINAL: either
    if (b.take(2) != 2) return false;
    uint32_t kraft[2];
    if (read_dynamic(b, nullptr, true, kraft) != kHeaderOk || kraft[0] != 32768u) return false;
    // distances: complete, or the single one-bit code that encoders write for a block with one distance (or none)
    if (kraft[1] != 32768u && kraft[1] != 16384u) return false;
    return !b.overrun();
}

// ---- one segment, symbolically ----
struct SegResult {
    uint64_t stop_bit; // bit after the last block decoded
    uint64_t n_sym;    // symbols produced (exact even when more than the slab holds)
    uint32_t status;   // kSeg*
    uint32_t final_block;
};

// Decodes blocks from start_bit while their header lies before stop_target (kNoBit: until the final block).  Symbols go to
// sym[0, cap); window: a match may reach up to 32 KiB in front of the segment (markers), else that is an error (the start
// of a member).  ws: kLaneWords words of workspace.
MHX_HD void decode_segment(const uint8_t *in, uint64_t n, uint64_t start_bit, uint64_t stop_target, bool window,
                           uint16_t *sym, uint64_t cap, uint32_t *ws, SegResult *res)
{
    uint32_t *lit = ws, *dist = ws + kLitCap;
    uint8_t *lens = (uint8_t *)(ws + kLitCap + kDistCap);
    Bits b{in, n, 0, 0, 0};
    b.seek(start_bit);
    uint64_t o = 0;
    uint32_t status = kSegOk, final_block = 0;
    const uint64_t hist = window ? kWin : 0;
    while (!final_block && b.pos() < stop_target) {
        if (b.overrun()) { status = kSegEnd; break; }
        if (b.cnt < 3) b.refill();
        final_block = b.take(1);
        const uint32_t type = b.take(2);
        if (type == 0) {
            b.drop(b.cnt & 7);
            if (b.cnt < 32) b.refill();
            const uint32_t len = b.take(16), nlen = b.take(16);
            if (b.overrun()) { status = kSegEnd; break; }
            if ((len ^ nlen) != 0xFFFFu) { status = kSegData; break; }
            if (b.pos() / 8 + len > n) { status = kSegEnd; break; }
            for (uint32_t i = 0; i < len; ++i) {
                const uint32_t v = b.take(8);
                if (o < cap) sym[o] = (uint16_t)v;
                ++o;
            }
            continue;
        }
        if (type == 3) { status = kSegData; break; }
        if (type == 1) fixed_lens(lens);
        else if (read_dynamic(b, lens, false, nullptr) != kHeaderOk) { status = b.overrun() ? kSegEnd : kSegData; break; }
        if (!build_table(lens, 288, kLitBits, lit, kLitCap, kLitLenTable) || !build_table(lens + 288, 32, kDistBits, dist, kDistCap, kDistTable)) {
            status = kSegData;
            break;
        }
        // the symbol loop of one block; each pass consumes at least one bit, so it ends within the input
        for (;;) {
            if (b.cnt < 48) b.refill();
            if (b.overrun()) { status = kSegEnd; break; }
            uint32_t e = lit[b.buf & ((1u << kLitBits) - 1)];
            if (e & kKindSub) {
                b.drop(kLitBits);
                e = lit[((e >> kValShift) + (uint32_t)(b.buf & ((1ull << (e & 0xFF)) - 1))) % kLitCap];
            }
            if (e & kKindInvalid) { status = kSegData; break; }
            b.drop((int)(e & 0xFF));
            if (e & kKindLiteral) {
                if (o < cap) sym[o] = (uint16_t)(e >> kValShift);
                ++o;
                continue;
            }
            if (e & kKindEnd) break;
            const int le = (int)((e >> kExtraShift) & 15u);
            const uint32_t len = (e >> kValShift) + (uint32_t)(b.buf & ((1ull << le) - 1));
            b.drop(le);
            if (b.cnt < 32) b.refill();
            uint32_t d = dist[b.buf & ((1u << kDistBits) - 1)];
            if (d & kKindSub) {
                b.drop(kDistBits);
                d = dist[((d >> kValShift) + (uint32_t)(b.buf & ((1ull << (d & 0xFF)) - 1))) % kDistCap];
            }
            if (!(d & kKindBase)) { status = kSegData; break; }
            b.drop((int)(d & 0xFF));
            const int de = (int)((d >> kExtraShift) & 15u);
            const uint32_t distance = (d >> kValShift) + (uint32_t)(b.buf & ((1ull << de) - 1));
            b.drop(de);
            if ((uint64_t)distance > o + hist) { status = kSegData; break; }
            for (uint32_t i = 0; i < len; ++i, ++o) {
                if (o >= cap) { o += len - i; break; }
                sym[o] = o >= distance ? sym[o - distance] : (uint16_t)(kMarker | (uint32_t)(kWin + o - distance));
            }
        }
        if (status != kSegOk) break;
    }
    if (status == kSegOk && b.overrun()) status = kSegEnd;
    res->stop_bit = b.pos();
    res->n_sym = o;
    res->status = status;
    res->final_block = final_block;
}

// ---- resolution: symbol -> byte; markers read the output in front of the segment (never before `floor`) ----
MHX_HD bool resolve_symbol(uint16_t s, const uint8_t *out, uint64_t seg_out, uint64_t floor, uint8_t *dst)
{
    if (!(s & kMarker)) { *dst = (uint8_t)s; return true; }
    const uint64_t w = s & 0x7FFFu;
    if (seg_out + w < floor + kWin) return false; // would read in front of the member
    *dst = out[seg_out + w - kWin];
    return true;
}

// ---- CRC-32 (gzip polynomial), table driven ----
MHX_HD void crc_table(uint32_t *t)
{
    for (uint32_t i = 0; i < 256; ++i) t[i] = crc_entry(i);
}
MHX_HD uint32_t crc_update(const uint32_t *t, uint32_t crc, const uint8_t *p, uint64_t n)
{
    uint32_t c = ~crc;
    for (uint64_t i = 0; i < n; ++i) c = t[(c ^ p[i]) & 0xFF] ^ (c >> 8);
    return ~c;
}

// ---- host side: the gzip member header and the round driver, shared by the HIP host code and the emulator ----

// Offset of the DEFLATE data of the member at in[0], 0 when there is no member there (the host decoder ends there too),
// -1 for a member header the host decoder refuses.
inline int64_t member_data_offset(const uint8_t *in, size_t n)
{
    const int64_t h = gzip_member(in, n);
    return h < 0 ? -1 : h;
}

// What the driver asks of a backend (the kernels, or the emulator):
//   search(targets, ntargets, limit_bit, cands)   cands[i] = first candidate in [targets[i], targets[i+1] or limit_bit),
//                                                  kNoBit if none
//   slabs(nseg, cap)                               room for nseg symbol slabs of cap symbols (contents may be lost)
//   decode(idx, nidx, starts, stops, window, res)  decodes slab slots idx[..] (slot j: starts[j], stops[j], window[j])
//   out_room(n)                                    the output holds n bytes from its start (contents kept); false: no room
//   resolve(nseg, n_sym, out_off, floor)           slot j -> out[out_off[j], + n_sym[j]); false: a marker in front of floor
//   crc(nseg, n_sym, out_off, crcs)                CRC-32 of every slot's output
struct MemberStats {
    uint64_t segments = 0, redone = 0, hops = 0, out_bytes = 0;
};
enum MemberStatus { kMemberOk = 0, kMemberFail = 1 };
struct MemberOut {
    uint64_t end_bit = 0; // bit after the final block
    uint64_t out_n = 0;
    uint32_t crc = 0;
};
using CrcCombine = uint32_t (*)(uint32_t, uint32_t, long);

// Rounds: the first covers first_segs targets, every further one twice as many, up to max_segs -- the search and the
// decode of a round reach no further than its own targets, so a small member costs one small round, not a walk over
// everything behind it in the buffer.
template <class Backend>
int inflate_member(Backend &be, uint64_t n_bytes, uint64_t start_bit, uint64_t seg_bits, uint32_t first_segs, uint32_t max_segs,
                   uint64_t out_base, CrcCombine combine, MemberOut *mo, MemberStats *st)
{
    const uint64_t limit = n_bytes * 8;
    uint64_t cap = std::max<uint64_t>(seg_bits / 8 * 8, 1u << 16); // symbols per slab: 8x the target size to start with
    uint64_t cur = start_bit, out_pos = out_base;
    uint32_t crc = 0;
    bool first_round = true;
    uint64_t round_n = std::max<uint32_t>(1, std::min(first_segs, max_segs));
    std::vector<uint64_t> targets, cands, s, stop;
    std::vector<uint8_t> win;
    std::vector<SegResult> res;
    std::vector<uint32_t> idx;
    for (;;) {
        // this round's targets: cur + k seg_bits, k = 1 .. round_n - 1; its last segment stops at the first block boundary
        // at or past round_end (or runs to the final block when the input ends before that)
        const uint64_t round_end = round_n * seg_bits < limit - std::min(limit, cur) ? cur + round_n * seg_bits : kNoBit;
        targets.clear();
        for (uint64_t k = 1; k < round_n && cur + k * seg_bits < limit; ++k) targets.push_back(cur + k * seg_bits);
        cands.assign(targets.size(), kNoBit);
        if (!targets.empty() && !be.search(targets.data(), targets.size(), std::min(round_end, limit), cands.data())) return kMemberFail;
        s.assign(1, cur);
        for (uint64_t c : cands)
            if (c != kNoBit && c > s.back()) s.push_back(c);
        const size_t m = s.size();
        stop.resize(m);
        win.resize(m);
        for (size_t j = 0; j < m; ++j) {
            stop[j] = j + 1 < m ? s[j + 1] : round_end;
            win[j] = !(first_round && j == 0);
        }
        if (!be.slabs(m, cap)) return kMemberFail;
        res.assign(m, SegResult{0, 0, 0, 0});
        idx.resize(m);
        for (size_t j = 0; j < m; ++j) idx[j] = (uint32_t)j;
        st->segments += m;
        size_t last = m; // index of the final segment of the round (m: the round ends without a final block)
        for (int pass = 0;; ++pass) {
            if (pass > kMaxPasses) return kMemberFail;
            if (!idx.empty() && !be.decode(idx.data(), idx.size(), s.data(), stop.data(), win.data(), res.data())) return kMemberFail;
            // the verified prefix
            size_t v = 0;
            uint64_t need_cap = 0;
            last = m;
            for (; v < m; ++v) {
                if (v > 0 && res[v - 1].stop_bit != s[v]) break;
                if (res[v].status != kSegOk) break;
                if (res[v].n_sym > cap) need_cap = std::max(need_cap, res[v].n_sym);
                if (res[v].final_block) { last = v; break; }
            }
            if (last < m || v == m) {
                if (need_cap) { // a verified segment overflowed its slab: larger slabs, the round again
                    cap = need_cap + need_cap / 8;
                    if (!be.slabs(m, cap)) return kMemberFail;
                    idx.resize(m);
                    for (size_t j = 0; j < m; ++j) idx[j] = (uint32_t)j;
                    continue;
                }
                break;
            }
            if (v == 0 || (res[v - 1].stop_bit == s[v] && res[v].status != kSegOk)) return kMemberFail; // a true error
            // redo every segment whose link is broken, from where its predecessor stopped
            idx.clear();
            for (size_t j = v; j < m; ++j) {
                if (res[j - 1].stop_bit != s[j] || res[j].status != kSegOk) {
                    if (res[j - 1].status != kSegOk && j > v) continue; // its predecessor is redone first
                    s[j] = res[j - 1].stop_bit;
                    idx.push_back((uint32_t)j);
                }
            }
            st->redone += idx.size();
        }
        const size_t used = last < m ? last + 1 : m;
        std::vector<uint64_t> nsym(used), off(used);
        uint64_t total = out_pos;
        for (size_t j = 0; j < used; ++j) { nsym[j] = res[j].n_sym; off[j] = total; total += nsym[j]; }
        if (!be.out_room(total)) return kMemberFail;
        if (!be.resolve(used, nsym.data(), off.data(), out_base)) return kMemberFail;
        st->hops += used;
        std::vector<uint32_t> crcs(used);
        if (!be.crc(used, nsym.data(), off.data(), crcs.data())) return kMemberFail;
        for (size_t j = 0; j < used; ++j) crc = combine(crc, crcs[j], (long)nsym[j]);
        out_pos = total;
        cur = res[used - 1].stop_bit;
        first_round = false;
        if (last < m) break;
        if (round_end == kNoBit || cur < round_end) return kMemberFail; // cannot happen for a verified round: no progress
        round_n = std::min<uint64_t>(round_n * 2, max_segs);
    }
    mo->end_bit = cur;
    mo->out_n = out_pos - out_base;
    mo->crc = crc;
    st->out_bytes += mo->out_n;
    return kMemberOk;
}

} // namespace dinf
} // namespace mhx
