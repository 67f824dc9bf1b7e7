// mhx_engine_nj.h -- what the host side of the jackknife (mhx_engine_resample.cpp) takes from neighbour joining's
// (mhx_engine_nj.cpp): the checks, where the state and the records of a call lie in a staging area, and the whole of a tree
// behind "the rows are staged".  Internal.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "mhx_device.h"
#include "mhx_engine_internal.h"
#include "mhx_engine_triangle.h"

namespace mhx {

// what mhx_dist_nj checks before anything is launched, the outputs aside; *done: nothing to compute (n <= 1)
int nj_check(const uint64_t *rows, const uint32_t *len, uint32_t n, uint32_t stride, int k, uint32_t s, int device_ptrs, bool *done);
// The state of a call ([r][act 0][act 1][pre 0][pre 1][cand][ctl]) and its five record arrays ([join_a][join_b][d][r_a][r_b]) as
// regions of a staging area: declared into `in` when constructed (records that are not wanted take no room), place() sets the
// pointers of `a` to them at `base`.
struct NjStateAt {
    size_t o_r, o_act[2], o_pre[2], o_cand, o_ctl;
    NjStateAt(Carve &in, uint32_t n);
    void place(NjArgs &a, uint8_t *base, uint32_t n, int k) const;
};
struct NjRecordsAt {
    size_t o_a, o_b, o_d, o_ra, o_rb;
    NjRecordsAt(Carve &in, uint32_t n, bool wanted = true);
    void place(NjArgs &a, uint8_t *base) const;
};
// The tree of the staged rows c: the dense triangle into tri (allocated, with a.words its pair words), the init pass into
// a.words, the joins, the records into a's arrays (device).  release: the triangle's two arrays are let go behind the init pass,
// which is then waited for.  Returns when the device is done; *clamps: the updates the clamp changed; g.last_dist_ms: the
// triangle plus the joins.
int nj_tree(const TriCall &c, const NjArgs &a, StoredTriangle &tri, bool release, uint64_t *clamps);

} // namespace mhx
