// mhx_engine_segments.cpp -- host side of the segmented sketch (mhx_sketch_segments: one bottom-s list per segment of an
// MHX_FMT_SEQ stream; `mash sketch -i` at buffer level).  Segments of at most kSegCut windows are sketched by ONE launch of
// segsketch_kernel (mhx_segsketch.hip: a workgroup per segment, everything in LDS); the others go, one after another,
// through the sketcher on their slice of the stream, where each of them amortises its step.  Device memory is bounded:
// a host-pointer call stages its stream and its rows in rounds of at most kSegBytesRound / kSegRowsRound bytes.
#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>
#include <exception>
#include <new>
#include <vector>

#include "mhx_device.h"
#include "mhx_engine_internal.h"
#include "mhx_internal.h"
#include "mhx_segsketch.h"

using namespace mhx;

namespace {
constexpr uint64_t kSegBytesRound = 64ull << 20;  // stream bytes of a host-pointer call on the device at a time
constexpr uint64_t kSegRowsRound = 256ull << 20;  // bytes of result rows staged on the device at a time

// One segment above the cut: its bytes (device or host memory) through the sketcher kept in g.seg.  hashes: its bottom-s
// list, ascending.  A too tight admission budget is repaired as everywhere else: once more with 16 times the budget.
int sketch_large_segment(const uint8_t *bytes, uint64_t n, bool on_device, int k, uint32_t s, std::vector<uint64_t> &hashes)
{
    SegCtx &c = g.seg;
    uint64_t boost = c.sk && c.k == k && c.s == s ? c.scale : 1;
    for (int attempt = 0; attempt < 6; ++attempt) {
        int rc = MHX_OK;
        if (!c.sk || c.k != k || c.s != s || c.scale != boost) {
            c.sk.reset();
            mhx_sketcher *sk = nullptr;
            rc = create_sketcher(k, s, 1, 0, boost, &sk);
            if (rc) return rc;
            c.sk.reset(sk);
            c.k = k; c.s = s; c.scale = boost;
        } else {
            rc = mhx_sketcher_reset(c.sk.get());
            if (rc) return rc;
        }
        rc = on_device ? mhx_sketcher_push_device(c.sk.get(), bytes, n, MHX_FMT_SEQ) : mhx_sketcher_push_host(c.sk.get(), bytes, n, MHX_FMT_SEQ);
        uint32_t nh = 0;
        if (!rc) {
            hashes.resize(s);
            rc = mhx_sketcher_finish(c.sk.get(), hashes.data(), nullptr, &nh);
        }
        if (rc == MHX_E_CAPACITY) { boost *= 16; clear_error(); continue; }
        if (rc) return rc;
        hashes.resize(nh);
        return MHX_OK;
    }
    return fail(MHX_E_CAPACITY, "could not size the device table for a segment of %llu bytes", (unsigned long long)n);
}

// Everything on the device: the stream, the offsets (h_off holds the same n_seg + 1 words on the host), rows and len.
// Complete when it returns.
int segments_on_device(const uint8_t *d_bytes, const uint64_t *h_off, const uint64_t *d_off, uint32_t n_seg, int k, uint32_t s,
                       uint64_t *d_rows, uint32_t *d_len, uint32_t stride)
{
    HIPCHK(launch_segsketch(k, d_bytes, d_off, n_seg, s, d_rows, d_len, stride, g.stream));
    std::vector<uint64_t> hashes;
    for (uint32_t i = 0; i < n_seg; ++i) {
        if (seg_is_small(seg_windows(h_off[i], h_off[i + 1], k))) continue;
        const int rc = sketch_large_segment(d_bytes + h_off[i], h_off[i + 1] - h_off[i], true, k, s, hashes);
        if (rc) { (void)hipStreamSynchronize(g.stream); return rc; }
        const uint32_t nh = (uint32_t)hashes.size(); // <= min(s, windows) <= stride
        if (nh) HIPCHK(hipMemcpyAsync(d_rows + (size_t)i * stride, hashes.data(), (size_t)nh * sizeof(uint64_t), hipMemcpyHostToDevice, g.stream));
        HIPCHK(hipMemcpyAsync(d_len + i, &nh, sizeof(nh), hipMemcpyHostToDevice, g.stream));
        HIPCHK(hipStreamSynchronize(g.stream)); // hashes and nh are used again
    }
    HIPCHK(hipStreamSynchronize(g.stream));
    return MHX_OK;
}

// ascending, inside the stream; *need = min(s, the largest window count): the row length no stride may fall below
int check_offsets(const uint64_t *h_off, uint32_t n_seg, uint64_t n, int k, uint32_t s, uint32_t *need)
{
    uint64_t max_w = 0;
    for (uint32_t i = 0; i < n_seg; ++i) {
        if (h_off[i + 1] < h_off[i]) return fail(MHX_E_ARG, "sketch_segments: seg_off[%u] > seg_off[%u]", i, i + 1);
        max_w = std::max(max_w, seg_windows(h_off[i], h_off[i + 1], k));
    }
    if (h_off[n_seg] > n) return fail(MHX_E_ARG, "sketch_segments: seg_off ends at %llu, the stream at %llu", (unsigned long long)h_off[n_seg], (unsigned long long)n);
    *need = (uint32_t)std::min<uint64_t>(s, max_w);
    return MHX_OK;
}
} // namespace

namespace mhx {
// The stream on the device, offsets and results on the host (offsets checked by the caller, stride >= what check_offsets
// asks for): rows go through the device staging in rounds of kSegRowsRound bytes; entries behind len[i] are zero.
int segments_resident(const uint8_t *d_bytes, const uint64_t *h_off, uint32_t n_seg, int k, uint32_t s, uint32_t stride, uint64_t *h_rows,
                      uint32_t *h_len)
{
    SegCtx &c = g.seg;
    const uint64_t row_bytes = (uint64_t)std::max(stride, 1u) * sizeof(uint64_t);
    const uint32_t per_round = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(n_seg, kSegRowsRound / row_bytes));
    for (uint32_t i0 = 0; i0 < n_seg; i0 += per_round) {
        const uint32_t cnt = std::min(per_round, n_seg - i0);
        HIPCHK(c.d_off.grow((size_t)cnt + 1, g.stream));
        HIPCHK(c.d_rows.grow(std::max<size_t>((size_t)cnt * stride, 1), g.stream));
        HIPCHK(c.d_len.grow(cnt, g.stream));
        HIPCHK(hipMemcpyAsync(c.d_off, h_off + i0, ((size_t)cnt + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, g.stream));
        if (stride) HIPCHK(hipMemsetAsync(c.d_rows, 0, (size_t)cnt * stride * sizeof(uint64_t), g.stream));
        const int rc = segments_on_device(d_bytes, h_off + i0, c.d_off, cnt, k, s, c.d_rows, c.d_len, stride);
        if (rc) return rc;
        if (stride) HIPCHK(hipMemcpyAsync(h_rows + (size_t)i0 * stride, c.d_rows, (size_t)cnt * stride * sizeof(uint64_t), hipMemcpyDeviceToHost, g.stream));
        HIPCHK(hipMemcpyAsync(h_len + i0, c.d_len, (size_t)cnt * sizeof(uint32_t), hipMemcpyDeviceToHost, g.stream));
        HIPCHK(hipStreamSynchronize(g.stream));
    }
    return MHX_OK;
}
} // namespace mhx

extern "C" int mhx_sketch_segments(const void *bytes, uint64_t n, const uint64_t *seg_off, uint32_t n_seg, int k, uint32_t s, uint64_t *rows,
                                   uint32_t *len, uint32_t stride, int device_ptrs)
{
    return entry("mhx_sketch_segments", [&]() -> int {
        if (!hash_k_supported(k)) return fail(MHX_E_ARG, "k-mer size %d not supported (1..32)", k);
        if (s == 0) return fail(MHX_E_ARG, "sketch_segments: sketch size 0");
        if (n_seg == 0) return MHX_OK;
        if (n_seg > 0x7FFFFFFFu) return fail(MHX_E_ARG, "sketch_segments: too many segments for one call (%u)", n_seg);
        if (!seg_off || !len || (!bytes && n)) return fail(MHX_E_ARG, "sketch_segments: null argument");
        std::vector<uint64_t> off_copy;
        const uint64_t *h_off = seg_off;
        if (device_ptrs) {
            off_copy.resize((size_t)n_seg + 1);
            HIPCHK(hipMemcpyAsync(off_copy.data(), seg_off, off_copy.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, g.stream));
            HIPCHK(hipStreamSynchronize(g.stream));
            h_off = off_copy.data();
        }
        uint32_t need = 0;
        int rc = check_offsets(h_off, n_seg, n, k, s, &need);
        if (rc) return rc;
        if (stride < need) return fail(MHX_E_ARG, "sketch_segments: stride %u, but a segment may fill %u entries", stride, need);
        if (need && !rows) return fail(MHX_E_ARG, "sketch_segments: null argument");
        const uint8_t *stream = (const uint8_t *)bytes;
        if (device_ptrs) return segments_on_device(stream, h_off, seg_off, n_seg, k, s, rows, len, stride);

        // host pointers: runs of whole segments whose bytes fit a round are staged and sketched where they lie; a segment larger
        // than a round (far above the cut) is pushed from the host, the sketcher stages it by itself
        SegCtx &c = g.seg;
        std::vector<uint64_t> rebased, hashes;
        for (uint32_t i0 = 0; i0 < n_seg;) {
            uint32_t i1 = i0 + 1;
            while (i1 < n_seg && h_off[i1 + 1] - h_off[i0] <= kSegBytesRound) ++i1;
            const uint64_t span = h_off[i1] - h_off[i0];
            if (span > kSegBytesRound) { // one segment
                rc = sketch_large_segment(stream + h_off[i0], span, false, k, s, hashes);
                if (rc) return rc;
                if (stride) memset(rows + (size_t)i0 * stride, 0, (size_t)stride * sizeof(uint64_t));
                if (!hashes.empty()) memcpy(rows + (size_t)i0 * stride, hashes.data(), hashes.size() * sizeof(uint64_t));
                len[i0] = (uint32_t)hashes.size();
            } else {
                HIPCHK(c.d_bytes.grow((size_t)span + 64, g.stream));
                if (span) HIPCHK(hipMemcpyAsync(c.d_bytes, stream + h_off[i0], (size_t)span, hipMemcpyHostToDevice, g.stream));
                HIPCHK(hipMemsetAsync(c.d_bytes + span, 0, 64, g.stream));
                rebased.resize((size_t)(i1 - i0) + 1);
                for (uint32_t i = i0; i <= i1; ++i) rebased[i - i0] = h_off[i] - h_off[i0];
                rc = segments_resident(c.d_bytes, rebased.data(), i1 - i0, k, s, stride, rows + (size_t)i0 * stride, len + i0);
                if (rc) return rc;
            }
            i0 = i1;
        }
        return MHX_OK;
    });
}

extern "C" uint32_t mhx_sketch_segments_cut(void) { return kSegCut; }
