// tests/emul/dinflate_emul.cpp -- CPU emulator of the device gzip decoder (test tool).
// Runs the host+device functions of auriclass_amd/csrc/mhx_dinflate.h lane by lane, stage by stage, in the order the
// kernels of mhx_dinflate.hip separate them (search, decode, chain check and redo, resolution of the tails in order and
// then of the rest, CRC-32 per segment), under the very round driver the device path uses.  Not part of the product;
// built by tests/test_dinflate_emulation.py with g++ -lz.
#include <zlib.h>

#include <cstdint>
#include <cstring>
#include <vector>

#include "../../auriclass_amd/csrc/mhx_dinflate.h"

using namespace mhx::dinf;

namespace {

struct EmulBackend {
    const uint8_t *in;
    uint64_t n;
    std::vector<uint16_t> sym;
    std::vector<uint32_t> ws;
    std::vector<uint8_t> out;
    uint64_t cap = 0;
    bool search(const uint64_t *targets, size_t nt, uint64_t limit, uint64_t *cands)
    {
        for (size_t i = 0; i < nt; ++i) { // one workgroup per target, 256 lanes per step
            const uint64_t lo = targets[i], hi = i + 1 < nt ? targets[i + 1] : limit;
            uint64_t best = kNoBit;
            for (uint64_t base = lo; base < hi && best == kNoBit; base += 256)
                for (uint64_t lane = 0; lane < 256; ++lane) {
                    const uint64_t bit = base + lane;
                    if (bit < hi && header_candidate(in, n, bit) && bit < best) best = bit;
                }
            cands[i] = best;
        }
        return true;
    }
    bool slabs(size_t m, uint64_t c)
    {
        sym.assign(m * c, 0xEEEE); // stale contents must never reach the output
        ws.assign(m * (size_t)kLaneWords, 0xDEADBEEF);
        cap = c;
        return true;
    }
    bool decode(const uint32_t *idx, size_t ni, const uint64_t *starts, const uint64_t *stops, const uint8_t *window, SegResult *res)
    {
        for (size_t t = 0; t < ni; ++t) {
            const uint32_t j = idx[t];
            decode_segment(in, n, starts[j], stops[j], window[j] != 0, sym.data() + (size_t)j * cap, cap, ws.data() + (size_t)j * kLaneWords, &res[j]);
        }
        return true;
    }
    bool out_room(size_t total)
    {
        if (out.size() < total) out.resize(total, 0xAA);
        return true;
    }
    bool resolve(size_t m, const uint64_t *nsym, const uint64_t *off, uint64_t floor)
    {
        bool ok = true;
        for (size_t j = 0; j < m; ++j) { // the chain: tails in order
            const uint64_t from = nsym[j] > kWin ? nsym[j] - kWin : 0;
            for (uint64_t i = from; i < nsym[j]; ++i)
                ok &= resolve_symbol(sym[(size_t)j * cap + i], out.data(), off[j], floor, out.data() + off[j] + i);
        }
        for (size_t j = 0; j < m; ++j) { // the rest, any order: backwards, to catch a dependence on order
            const uint64_t end = nsym[j] > kWin ? nsym[j] - kWin : 0;
            for (uint64_t i = end; i-- > 0;)
                ok &= resolve_symbol(sym[(size_t)j * cap + i], out.data(), off[j], floor, out.data() + off[j] + i);
        }
        return ok;
    }
    bool crc(size_t m, const uint64_t *nsym, const uint64_t *off, uint32_t *crcs)
    {
        uint32_t table[256];
        crc_table(table);
        for (size_t j = 0; j < m; ++j) crcs[j] = crc_update(table, 0, out.data() + off[j], nsym[j]);
        return true;
    }
};

uint32_t combine(uint32_t a, uint32_t b, long n) { return (uint32_t)crc32_combine(a, b, (z_off_t)n); }
uint32_t le32(const uint8_t *p) { return p[0] | (p[1] << 8) | (p[2] << 16) | ((uint32_t)p[3] << 24); }

} // namespace

// All members of gz[0, n) through the emulated device path.  0: success, *out_n bytes (up to cap copied to out);
// 1: the device path reports a failure (the library would hand the input to the host decoder).
// stats8: [0] members, [1] segments, [2] redone, [3] hops, [5] bytes.
extern "C" int emul_gunzip(const uint8_t *gz, uint64_t n, uint64_t seg_bytes, uint32_t round_segs, uint8_t *dst, uint64_t cap,
                           uint64_t *out_n, uint64_t *stats8)
{
    EmulBackend be{gz, n, {}, {}, {}, 0};
    memset(stats8, 0, 8 * sizeof(uint64_t));
    uint64_t off = 0, total = 0;
    while (off < n) {
        const int64_t h = member_data_offset(gz + off, n - off);
        if (h == 0) break;
        if (h < 0) return 1;
        MemberOut mo;
        MemberStats ms;
        const int rc = inflate_member(be, n, (off + (uint64_t)h) * 8, seg_bytes * 8, round_segs < 4 ? round_segs : 4, round_segs, total, combine, &mo,
                                     &ms);
        stats8[1] += ms.segments;
        stats8[2] += ms.redone;
        stats8[3] += ms.hops;
        if (rc != kMemberOk) return 1;
        const uint64_t tb = (mo.end_bit + 7) / 8;
        if (tb + 8 > n || le32(gz + tb) != mo.crc || le32(gz + tb + 4) != (uint32_t)mo.out_n) return 1;
        total += mo.out_n;
        ++stats8[0];
        off = tb + 8;
    }
    stats8[5] = total;
    *out_n = total;
    memcpy(dst, be.out.data(), total < cap ? total : cap);
    return 0;
}
