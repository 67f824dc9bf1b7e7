// mhx_dinflate.hip -- gzip decoded on the device (mhx_gunzip_device): the kernels of the stages in mhx_dinflate.h and the
// host side that strings them together.  The host decoder has the last word: a member the device cannot take to its end
// with a matching CRC-32 and length -- no consistent chain within the pass bound, an invalid code, a mismatch, no room --
// sends the whole input through mhx_gunzip_buffer, whose bytes and error are the result.  So the device path only ever
// changes the speed.
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <string.h>
#include <zlib.h>

#include <algorithm>
#include <chrono>
#include <vector>

#include "mhx_dinflate.h"
#include "mhx_engine_internal.h"
#include "mhx_internal.h"

namespace mhx {
namespace {

using namespace dinf;

constexpr int kSearchBlock = 256;
constexpr int kDecodeBlock = 64;
constexpr int kResolveBlock = 1024;
constexpr size_t kInPad = 64;

// one workgroup per target: lanes test consecutive bit positions of [targets[i], targets[i + 1]) until one is a candidate
__global__ __launch_bounds__(kSearchBlock) void dinf_search_kernel(const uint8_t *in, uint64_t n, const uint64_t *targets,
                                                                   uint32_t ntargets, uint64_t limit, uint64_t *cands)
{
    __shared__ unsigned long long best;
    const uint32_t i = blockIdx.x;
    if (i >= ntargets) return;
    const uint64_t lo = targets[i], hi = i + 1 < ntargets ? targets[i + 1] : limit;
    if (threadIdx.x == 0) best = kNoBit;
    __syncthreads();
    for (uint64_t base = lo; base < hi; base += kSearchBlock) {
        const uint64_t bit = base + threadIdx.x;
        if (bit < hi && header_candidate(in, n, bit)) atomicMin(&best, (unsigned long long)bit);
        __syncthreads();
        const unsigned long long found = best; // every lane reads it before any lane may start the next step's atomics
        __syncthreads();
        if (found != kNoBit) break;
    }
    if (threadIdx.x == 0) cands[i] = best;
}

// one lane per slot to decode, `per` lanes of each workgroup busy: few segments are spread over many CUs rather than packed
// into few waves (a lane's decode is latency-bound; its wave runs at the pace of its slowest lane either way)
__global__ __launch_bounds__(kDecodeBlock) void dinf_decode_kernel(const uint8_t *in, uint64_t n, const uint32_t *idx, uint32_t nidx, uint32_t per,
                                                                   const uint64_t *starts, const uint64_t *stops, const uint8_t *window,
                                                                   uint16_t *sym, uint64_t cap, uint32_t *ws, SegResult *res)
{
    const uint32_t t = blockIdx.x * per + threadIdx.x;
    if (threadIdx.x >= per || t >= nidx) return;
    const uint32_t j = idx[t];
    decode_segment(in, n, starts[j], stops[j], window[j] != 0, sym + (uint64_t)j * cap, cap, ws + (uint64_t)j * kLaneWords, &res[j]);
}

// one workgroup walks the chain: the last 32 KiB of every segment in order, each reading only what earlier steps resolved
__global__ __launch_bounds__(kResolveBlock) void dinf_resolve_tails_kernel(const uint16_t *sym, uint64_t cap, uint32_t nseg,
                                                                           const uint64_t *nsym, const uint64_t *off, uint64_t floor,
                                                                           uint8_t *out, uint32_t *err)
{
    for (uint32_t j = 0; j < nseg; ++j) {
        const uint64_t n = nsym[j], from = n > kWin ? n - kWin : 0;
        const uint16_t *s = sym + (uint64_t)j * cap;
        for (uint64_t i = from + threadIdx.x; i < n; i += kResolveBlock)
            if (!resolve_symbol(s[i], out, off[j], floor, out + off[j] + i)) atomicOr(err, 1u);
        __syncthreads();
    }
}

// everything in front of the tails, all segments at once (blockIdx.y: segment)
__global__ __launch_bounds__(256) void dinf_resolve_bulk_kernel(const uint16_t *sym, uint64_t cap, const uint64_t *nsym,
                                                                const uint64_t *off, uint64_t floor, uint8_t *out, uint32_t *err)
{
    const uint32_t j = blockIdx.y;
    const uint64_t n = nsym[j], end = n > kWin ? n - kWin : 0;
    const uint16_t *s = sym + (uint64_t)j * cap;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < end; i += (uint64_t)gridDim.x * 256)
        if (!resolve_symbol(s[i], out, off[j], floor, out + off[j] + i)) atomicOr(err, 1u);
}

// one lane per segment
__global__ __launch_bounds__(64) void dinf_crc_kernel(const uint8_t *out, uint32_t nseg, const uint64_t *nsym, const uint64_t *off,
                                                      uint32_t *crcs)
{
    __shared__ uint32_t table[256];
    for (int i = threadIdx.x; i < 256; i += 64) table[i] = crc_entry((uint32_t)i);
    __syncthreads();
    const uint32_t j = blockIdx.x * 64 + threadIdx.x;
    if (j >= nseg) return;
    crcs[j] = crc_update(table, 0, out + off[j], nsym[j]);
}

uint32_t combine_crc(uint32_t a, uint32_t b, long n) { return (uint32_t)crc32_combine(a, b, (z_off_t)n); }

uint64_t g_stats[8];

size_t env_size(const char *name, size_t dflt)
{
    const char *e = getenv(name);
    if (!e) return dflt;
    const long long v = atoll(e);
    return v > 0 ? (size_t)v : dflt;
}

// The kernels behind the round driver of mhx_dinflate.h.  Errors of the runtime make a stage return false (the caller then
// hands the input to the host).
struct DeviceBackend {
    hipStream_t st;
    const uint8_t *d_in = nullptr;
    uint64_t n = 0;
    uint8_t *user_out = nullptr; // the caller's buffer, while what is decoded fits it
    size_t user_cap = 0;
    uint8_t *out = nullptr;
    size_t out_len = 0;          // bytes of output produced so far (what a switch to the own buffer copies)
    DevArray<uint8_t> own_out;
    DevArray<uint16_t> sym;
    DevArray<uint32_t> ws;
    DevArray<uint64_t> words; // targets / cands, or starts + stops + nsym + off
    DevArray<uint8_t> win;
    DevArray<uint32_t> idx, crcs, err;
    DevArray<SegResult> res;
    uint64_t cap = 0;
    size_t nslots = 0;
    float ms = 0.f;

    bool ok(hipError_t e) { return e == hipSuccess; }
    bool search(const uint64_t *targets, size_t nt, uint64_t limit, uint64_t *cands)
    {
        if (!ok(words.grow(2 * nt))) return false;
        if (!ok(hipMemcpyAsync(words, targets, nt * 8, hipMemcpyHostToDevice, st))) return false;
        dinf_search_kernel<<<(uint32_t)nt, kSearchBlock, 0, st>>>(d_in, n, words, (uint32_t)nt, limit, words + nt);
        if (!ok(hipGetLastError())) return false;
        if (!ok(hipMemcpyAsync(cands, words + nt, nt * 8, hipMemcpyDeviceToHost, st))) return false;
        return ok(hipStreamSynchronize(st));
    }
    bool slabs(size_t m, uint64_t c)
    {
        if (m * c > sym.cap() && !ok(sym.grow(m * c + (m * c) / 4))) return false;
        if (!ok(ws.grow(m * (size_t)kLaneWords)) || !ok(res.grow(m)) || !ok(win.grow(m)) || !ok(idx.grow(m)) || !ok(crcs.grow(m)) ||
            !ok(words.grow(4 * m)) || !ok(err.grow(1)))
            return false;
        cap = c;
        nslots = m;
        return true;
    }
    bool decode(const uint32_t *ix, size_t ni, const uint64_t *starts, const uint64_t *stops, const uint8_t *window, SegResult *r)
    {
        const size_t m = nslots;
        if (!ok(hipMemcpyAsync(idx, ix, ni * 4, hipMemcpyHostToDevice, st)) ||
            !ok(hipMemcpyAsync(words, starts, m * 8, hipMemcpyHostToDevice, st)) ||
            !ok(hipMemcpyAsync(words + m, stops, m * 8, hipMemcpyHostToDevice, st)) ||
            !ok(hipMemcpyAsync(win, window, m, hipMemcpyHostToDevice, st)) ||
            !ok(hipMemcpyAsync(res, r, m * sizeof(SegResult), hipMemcpyHostToDevice, st)))
            return false;
        const uint32_t per = (uint32_t)std::min<size_t>(kDecodeBlock, std::max<size_t>(1, (ni + 1023) / 1024));
        dinf_decode_kernel<<<(uint32_t)((ni + per - 1) / per), kDecodeBlock, 0, st>>>(d_in, n, idx, (uint32_t)ni, per, words, words + m, win,
                                                                                      sym, cap, ws, res);
        if (!ok(hipGetLastError())) return false;
        if (!ok(hipMemcpyAsync(r, res, m * sizeof(SegResult), hipMemcpyDeviceToHost, st))) return false;
        return ok(hipStreamSynchronize(st));
    }
    bool out_room(size_t total)
    {
        if (user_out && total <= user_cap) { out = user_out; return true; }
        if (own_out.cap() >= total) return true;
        DevArray<uint8_t> bigger;
        if (!ok(bigger.grow(std::max(total, own_out.cap() * 2)))) return false;
        if (out_len && !ok(hipMemcpyAsync(bigger, out, out_len, hipMemcpyDeviceToDevice, st))) return false;
        if (!ok(hipStreamSynchronize(st))) return false;
        own_out = std::move(bigger);
        out = own_out;
        user_out = nullptr; // from here on the result lives in the own buffer
        return true;
    }
    bool upload_layout(size_t m, const uint64_t *nsym, const uint64_t *off)
    {
        return ok(hipMemcpyAsync(words + 2 * nslots, nsym, m * 8, hipMemcpyHostToDevice, st)) &&
               ok(hipMemcpyAsync(words + 3 * nslots, off, m * 8, hipMemcpyHostToDevice, st));
    }
    bool resolve(size_t m, const uint64_t *nsym, const uint64_t *off, uint64_t floor)
    {
        if (!upload_layout(m, nsym, off) || !ok(hipMemsetAsync(err, 0, 4, st))) return false;
        const uint64_t *d_nsym = words + 2 * nslots, *d_off = words + 3 * nslots;
        dinf_resolve_tails_kernel<<<1, kResolveBlock, 0, st>>>(sym, cap, (uint32_t)m, d_nsym, d_off, floor, out, err);
        uint64_t most = 0;
        for (size_t j = 0; j < m; ++j) most = std::max(most, nsym[j]);
        if (most > kWin) {
            const uint32_t gx = (uint32_t)std::min<uint64_t>((most - kWin + 255) / 256, 64);
            dinf_resolve_bulk_kernel<<<dim3(gx, (uint32_t)m), 256, 0, st>>>(sym, cap, d_nsym, d_off, floor, out, err);
        }
        if (!ok(hipGetLastError())) return false;
        uint32_t e = 1;
        if (!ok(hipMemcpyAsync(&e, err, 4, hipMemcpyDeviceToHost, st)) || !ok(hipStreamSynchronize(st))) return false;
        out_len = off[m - 1] + nsym[m - 1];
        return e == 0;
    }
    bool crc(size_t m, const uint64_t *nsym, const uint64_t *off, uint32_t *c)
    {
        (void)nsym;
        (void)off; // uploaded by resolve()
        dinf_crc_kernel<<<(uint32_t)((m + 63) / 64), 64, 0, st>>>(out, (uint32_t)m, words + 2 * nslots, words + 3 * nslots, crcs);
        if (!ok(hipGetLastError())) return false;
        if (!ok(hipMemcpyAsync(c, crcs, m * 4, hipMemcpyDeviceToHost, st))) return false;
        return ok(hipStreamSynchronize(st));
    }
};

uint32_t le32(const uint8_t *p) { return p[0] | (p[1] << 8) | (p[2] << 16) | ((uint32_t)p[3] << 24); }

// the host decoder's verdict on in[0, n), into the device buffer when it fits
int host_gunzip_into(const uint8_t *in, size_t n, uint8_t *d_out, size_t cap, size_t *out_n, hipStream_t st)
{
    size_t need = 0;
    int rc = mhx_gunzip_buffer(in, n, nullptr, 0, &need);
    if (rc) return rc;
    *out_n = need;
    if (!d_out || need > cap || need == 0) return MHX_OK;
    std::vector<uint8_t> tmp(need);
    rc = mhx_gunzip_buffer(in, n, tmp.data(), need, &need);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(d_out, tmp.data(), need, hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st));
    return MHX_OK;
}

} // namespace
} // namespace mhx

using namespace mhx;

extern "C" int mhx_gunzip_device(const void *gz, size_t n, void *d_out, size_t cap, size_t *out_n)
{
    return guarded("mhx_gunzip_device", [&]() -> int { // (the arguments are checked before the engine: the prologue stays as it was)
        clear_error();
        if (!gz || !out_n) return fail(MHX_E_ARG, "null argument");
        int rc = require_engine();
        if (rc) return rc;
        const auto t0 = std::chrono::steady_clock::now();
        memset(g_stats, 0, sizeof(g_stats));
        const uint8_t *in = (const uint8_t *)gz;
        hipStream_t st = g.stream;
        const size_t min_member = env_size("MHX_DINFLATE_MIN", 1u << 20);     // smaller members: the host decoder
        const size_t seg_bytes = env_size("MHX_DINFLATE_SEGMENT", 64u << 10); // target compressed bytes per segment
        // segments of the largest round; one resolution launch spans a round's segments in its grid's y dimension
        const uint32_t round_segs = (uint32_t)std::min<size_t>(env_size("MHX_DINFLATE_ROUND", 1024), 65535);
        const int host_threads = ingest_thread_budget();
        size_t total = 0;
        bool on_device = false;
        rc = [&]() -> int {
            DeviceBackend be;
            be.st = st;
            be.user_out = (uint8_t *)d_out;
            be.user_cap = d_out ? cap : 0;
            be.out = be.user_out;
            DevArray<uint8_t> d_in;
            size_t off = 0;
            bool uploaded = false;
            (void)on_device;
            // Members go to the device while at least min_member compressed bytes remain and the last one it decoded was that
            // large; a BGZF block (bgzip's many small members), a header the host refuses, the first small member decoded and
            // everything behind them go to the host decoders (BgzfReader for a run of BGZF blocks).
            while (off < n) {
                const int64_t h = member_data_offset(in + off, n - off);
                if (h == 0) break; // no further member: the host decoder ignores what is left, so does this
                if (h < 0 || n - off < min_member || bgzf_block_size(in + off, n - off)) break;
                if (!uploaded) {
                    if (!be.ok(d_in.grow(n + kInPad)) || !be.ok(hipMemsetAsync(d_in + n, 0, kInPad, st)) ||
                        !be.ok(hipMemcpyAsync(d_in, in, n, hipMemcpyHostToDevice, st)))
                        return 1;
                    be.d_in = d_in;
                    be.n = n;
                    uploaded = true;
                }
                MemberOut mo;
                MemberStats ms;
                const int mrc = inflate_member(be, n, (uint64_t)(off + (size_t)h) * 8, (uint64_t)seg_bytes * 8, 16, round_segs, total,
                                               combine_crc, &mo, &ms);
                g_stats[1] += ms.segments;
                g_stats[2] += ms.redone;
                g_stats[3] += ms.hops;
                if (mrc != kMemberOk) return 1;
                const size_t tb = (size_t)((mo.end_bit + 7) / 8);
                if (tb + 8 > n || le32(in + tb) != mo.crc || le32(in + tb + 4) != (uint32_t)mo.out_n) return 1;
                total += mo.out_n;
                be.out_len = total;
                ++g_stats[0];
                const bool small = tb + 8 - off < min_member;
                off = tb + 8;
                on_device = true;
                if (small) break;
            }
            if (off < n && member_data_offset(in + off, n - off) != 0) { // the rest through the host decoders, appended
                std::vector<uint8_t> tmp(std::max<size_t>(4 * (n - off), 1u << 20));
                size_t rest = 0;
                int hrc = mhx_gunzip_buffer_mt(in + off, n - off, tmp.data(), tmp.size(), &rest, host_threads);
                if (hrc == MHX_E_CAPACITY) {
                    tmp.resize(rest);
                    hrc = mhx_gunzip_buffer_mt(in + off, n - off, tmp.data(), tmp.size(), &rest, host_threads);
                }
                if (hrc) return 1; // the sequential decoder on the whole input decides what the error is
                if (rest) {
                    if (!be.out_room(total + rest)) return 1;
                    if (!be.ok(hipMemcpyAsync(be.out + total, tmp.data(), rest, hipMemcpyHostToDevice, st)) || !be.ok(hipStreamSynchronize(st)))
                        return 1;
                }
                g_stats[4] += n - off;
                total += rest;
            }
            return 0;
        }();
        g_stats[5] = 0;
        if (rc != 0) { // the host has the last word
            memset(g_stats, 0, sizeof(g_stats));
            g_stats[4] = n;
            clear_error();
            rc = host_gunzip_into(in, n, (uint8_t *)d_out, cap, &total, st);
            if (rc) return rc;
        }
        g_stats[5] = total;
        if (g.profiling) g_stats[6] = (uint64_t)std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        *out_n = total;
        if (d_out && total > cap) return fail(MHX_E_CAPACITY, "gunzip: output buffer too small (%zu needed)", total);
        return MHX_OK;
    });
}

extern "C" int mhx_last_inflate_stats(uint64_t *out8)
{
    clear_error();
    if (!out8) return fail(MHX_E_ARG, "null argument");
    memcpy(out8, g_stats, sizeof(g_stats));
    return MHX_OK;
}
