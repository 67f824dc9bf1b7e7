// mhx_tighten.h -- the arithmetic of the tighten pass (table_tighten_kernel): which histogram bin a hash falls in, how many
// qualifying entries a pass asks for, where the cumulative count reaches that number and what the admission threshold
// becomes.  Shared by the kernel and the CPU emulator under tests/emul/ (MHX_HD), so that the rule can be run without a GPU.
#pragma once
#include <math.h>
#include "mhx_hd.h"
#include "mhx_device_consts.h"

namespace mhx {

static_assert(kHistBins == 1 << 11, "tighten_bin takes the 11 leading bits below T's top bit");
constexpr uint32_t kNoCut = 0xFFFFFFFFu;

// the histogram covers [0, 2^(64 - lz)): the 11 bits of a hash <= T that follow T's leading zeros select the bin
MHX_HD int tighten_lz(uint64_t T) { return T ? __builtin_clzll(T) : 63; }
MHX_HD uint32_t tighten_bin(uint64_t key, int lz) { return (uint32_t)((key << lz) >> (64 - 11)); }

// Entries a pass wants below the new threshold.  Exact pass: s.  Sampled pass: counts are ~Binomial(truth, 1/sample); ask for
// the expected s/sample plus six standard deviations (+16 for small s) so that the sampling error cannot push T below the
// true s-th qualifying hash (~1e-9 per pass; finish() counts exactly and refuses a short result below a lowered T)
MHX_HD uint32_t tighten_target(uint32_t sketch_size, uint32_t sample)
{
    if (sample <= 1) return sketch_size;
    const float mean = (float)sketch_size / (float)sample;
    return (uint32_t)(mean + 6.0f * sqrtf(mean)) + 16u;
}

// One thread's share of the search: c[0 .. n) are the counts of bins first_bin .. first_bin + n - 1 (value order), `before`
// the sum of every lower bin.  The first bin at which the cumulative count reaches s, or kNoCut when that happens elsewhere.
MHX_HD uint32_t tighten_cut_among(const uint32_t *c, int n, uint32_t first_bin, uint32_t before, uint32_t s)
{
    uint32_t cut = kNoCut, run = before;
    for (int j = 0; j < n; ++j) {
        if (run < s && run + c[j] >= s) cut = first_bin + (uint32_t)j;
        run += c[j];
    }
    return cut;
}

// The threshold a pass leaves behind.  T only ever decreases, and only to a value below which at least s entries with
// count >= m already exist (the last value of bin `cut`), so every hash of the final sketch stays admitted (and therefore
// fully counted) for the whole run.  A threshold with fewer than 11 significant bits (lz > 52) is left alone.
// m > 1: `established` goes (and stays) up once T follows the solid hashes -- no more caps; until then, and unless the table
// looks like a small genome sequenced deeply, next_cap (the byte-count cap in front of the next launch of the same push,
// cap_threshold_kernel's rule without its launch; 0: none) bounds the result and raises `bounded`.
MHX_HD uint64_t tighten_threshold(uint64_t T, int lz, uint32_t cut, uint32_t min_mult, uint64_t next_cap, uint64_t occupied,
                                  uint64_t solid, bool &established, bool &bounded)
{
    uint64_t now = T;
    if (cut != kNoCut && lz <= 52) {
        const uint64_t edge = (((uint64_t)cut + 1) << (53 - lz)) - 1; // last value of bin `cut`
        if (edge < T) {
            now = edge;
            if (min_mult > 1) established = true;
        }
    }
    if (next_cap && !established && !(occupied > 0 && solid * 5 >= occupied) && now > next_cap) {
        now = next_cap;
        bounded = true;
    }
    return now;
}

} // namespace mhx
