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
// the pair words of n lists against MHX_LINKAGE_STORE_MB
int nj_budget(uint32_t n);
// the state of a call ([r][act 0][act 1][pre 0][pre 1][cand][ctl]) and its five record arrays ([join_a][join_b][d][r_a][r_b]):
// their bytes, and the pointers of `a` set to them at `at`
size_t nj_state_bytes(uint32_t n);
size_t nj_records_bytes(uint32_t n);
void nj_place_state(NjArgs &a, uint8_t *at, uint32_t n, int k);
void nj_place_records(NjArgs &a, uint8_t *at, uint32_t n);
// The tree of the staged rows c: the dense triangle into p_common / p_denom (packed, [n (n - 1) / 2] each), the init pass into
// a.words, the joins, the records into a's arrays (device).  `release` (may be null) is emptied behind the init pass, which is
// then waited for.  Returns when the device is done; *clamps: the updates the clamp changed; g.last_dist_ms: the triangle plus
// the joins.
int nj_tree(const TriCall &c, const NjArgs &a, uint32_t *p_common, uint32_t *p_denom, DevArray<uint8_t> *release, uint64_t *clamps);

} // namespace mhx
