"""CPU emulation of the sharded path's merge (auriclass_amd/csrc/mhx_merge.h, the very functions the kernels and
merge_slabs_impl run): tests/emul/merge_emul.cpp runs the scatter, bin and compact phases of a whole call with the
workgroups and virtual threads in seeded shuffled orders, and the table path's insert over a small table.  Everything
against the rule of tests/merge_rule.py on the crafted cases of tests/merge_cases.py -- and this is where the cases are
shown to be what they are built for: which bin overflows, how many qualify, which flag comes back."""
import ctypes

import numpy as np
import pytest

from tests import emul_build
from tests import merge_cases as mc
from tests import merge_rule as mr

MAX64, MAX32 = mr.MAX64, mr.MAX32
SEEDS = (1, 2, 3)


@pytest.fixture(scope="module")
def emul():
    L = emul_build.load("merge_emul")
    u32, u64, vp = ctypes.c_uint32, ctypes.c_uint64, ctypes.c_void_p
    L.emul_merge_consts.argtypes = [vp]
    L.emul_merge_consts.restype = None
    L.emul_merge_geometry.argtypes = [u64, u64, u32, vp]
    L.emul_merge_geometry.restype = ctypes.c_int
    L.emul_merge_binned.argtypes = [vp, u64, u64, u32, vp, u32, u32, u64, u64, u32, vp, vp, vp]
    L.emul_merge_binned.restype = ctypes.c_int64
    L.emul_merge_table.argtypes = [vp, u64, u64, u32, vp, u32, u32, u64, u64, vp, vp, u64]
    L.emul_merge_table.restype = ctypes.c_int
    return L


def c_geometry(L, total, t_min, n_ranks):
    out = np.zeros(7, np.uint64)
    ok = L.emul_merge_geometry(total, t_min, n_ranks, out.ctypes.data)
    return tuple(int(x) for x in out) if ok else None


def finish(entries, rk, case):
    """what merge_slabs_impl and finish() do behind either device path: 2^64-1 from header word 3, the first s, the
    exactness rule"""
    t_min = mr.t_min_of(rk)
    maxkey = sum(int(h[3]) for h, _, _ in rk)
    if t_min == MAX64 and maxkey >= case.m:
        entries = entries + [(MAX64, min(maxkey, MAX32))]
    if len(entries) < case.s and t_min < mr.hash_max(case.k):
        return mr.CAPACITY
    kept = entries[:case.s]
    return np.array([h for h, _ in kept], np.uint64), np.array([c for _, c in kept], np.uint32)


def same(a, b):
    if isinstance(a, str) or isinstance(b, str):
        return isinstance(a, str) and isinstance(b, str) and a == b
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def run_binned(L, case, rk, seed, hdr_words=0):
    """(flags or negative code, result or None, fills, quals, geometry)"""
    buf, cap = mc.layout(rk, hdr_words)
    n = np.array([int(h[0]) for h, _, _ in rk], np.uint64)
    total, t_min = mc.totals(rk)
    geo = c_geometry(L, total, t_min, len(rk))
    if geo is None:
        assert L.emul_merge_binned(buf.ctypes.data, hdr_words + cap + cap // 2, cap, hdr_words, n.ctypes.data, len(rk), case.m, t_min, seed, 2,
                                   np.zeros(8, np.uint64).ctypes.data, None, None) == -1
        return -1, None, None, None, None
    out_cap = mc.fin_cap(case.s)
    out = np.full(4 + out_cap + out_cap // 2, 0xEEEEEEEEEEEEEEEE, np.uint64)
    fills, quals = np.zeros(geo[0], np.uint32), np.zeros(geo[0], np.uint32)
    flags = L.emul_merge_binned(buf.ctypes.data, hdr_words + cap + cap // 2, cap, hdr_words, n.ctypes.data, len(rk), case.m, t_min, seed, out_cap,
                                out.ctypes.data, fills.ctypes.data, quals.ctypes.data)
    assert flags >= 0, flags
    assert int(out[1]) == t_min and int(out[2]) == flags and int(out[3]) == 0
    result = None
    if flags == 0:
        grand = int(out[0])
        assert grand == int(quals.sum())
        k = min(grand, out_cap)
        assert k >= min(grand, case.s)
        h, c = out[4:4 + k], out[4 + out_cap:].view(np.uint32)[:k]
        assert (out[4 + k:4 + out_cap] == 0xEEEEEEEEEEEEEEEE).all()          # nothing written behind the last entry
        result = finish(list(zip(h.tolist(), c.tolist())), rk, case)
    return flags, result, fills, quals, geo


def run_table(L, case, rk, seed, log2_slots=19, own=None):
    """the table path on a table that holds `own`'s entries (the own rank's, already there) -> result"""
    buf, cap = mc.layout(rk)
    n = np.array([int(h[0]) for h, _, _ in rk], np.uint64)
    _, t_min = mc.totals(rk)
    nslots = 1 << log2_slots
    keys, cnts = np.full(nslots, MAX64, np.uint64), np.zeros(nslots, np.uint32)
    if own is not None:   # this rank's entries: put there by the same insert, from a buffer of its slab alone
        obuf, ocap = mc.layout([own])
        on = np.array([int(own[0][0])], np.uint64)
        assert L.emul_merge_table(obuf.ctypes.data, ocap + ocap // 2, ocap, 0, on.ctypes.data, 1, 1, MAX64 - 1, seed, keys.ctypes.data, cnts.ctypes.data, nslots) == 0
    assert L.emul_merge_table(buf.ctypes.data, cap + cap // 2, cap, 0, n.ctypes.data, len(rk), case.own_rank, t_min, seed, keys.ctypes.data,
                              cnts.ctypes.data, nslots) == 0
    keep = (keys != np.uint64(MAX64)) & (keys <= np.uint64(t_min)) & (cnts >= case.m)    # the extraction: count >= m, hash <= T
    order = np.argsort(keys[keep])
    return finish(list(zip(keys[keep][order].tolist(), cnts[keep][order].tolist())), rk, case)


def test_constants_and_geometry_port(emul):
    out = np.zeros(4, np.uint32)
    emul.emul_merge_consts(out.ctypes.data)
    assert tuple(out) == (mc.MAX_RANKS, mc.MAX_BINS, mc.MAX_SLOTS, mc.MAX_QUAL)


def check_geometry(emul, total, t_min, n_ranks):
    geo = c_geometry(emul, total, t_min, n_ranks)
    assert (geo[:5] if geo else None) == mc.geometry(total, t_min, n_ranks), (total, t_min, n_ranks)
    if geo is None:
        return None
    nbins, shift, region, slots, used, scatter_lds, bin_lds = geo
    assert 256 <= nbins <= mc.MAX_BINS and nbins & (nbins - 1) == 0
    assert 256 <= slots <= mc.MAX_SLOTS and slots & (slots - 1) == 0
    assert 4 * region <= 3 * slots                                     # the bin pass's guard (flag 2) cannot trip
    assert (t_min >> shift) < nbins and used == (t_min >> shift) + 1   # every hash <= t_min has a bin
    assert total <= nbins * 1024 and (nbins == 256 or total > nbins * 512)
    # the LDS both passes lay out is what launch_merge_bins requests, within the limit it sets once per kernel
    assert scatter_lds == 2 * 4 * nbins <= 2 * 4 * mc.MAX_BINS
    assert bin_lds == 12 * slots + 12 * mc.MAX_QUAL <= 12 * mc.MAX_SLOTS + 12 * mc.MAX_QUAL <= 160 * 1024
    assert region >= total / used                                      # room for the average fill, at least
    return geo


def test_geometry_sweep(emul):
    totals = sorted({1, 2, 255, 256, 1023, 1024, 1025, 2700, 2800, 3071, 3072, 3073, 100_000} |
                    {x + d for j in range(18, 25) for x in (1 << j,) for d in (-1, 0, 1)})
    t_mins = sorted({0, 1, 2, 3, MAX32, MAX64 - 1, MAX64} | {max(0, (1 << j) + d) for j in range(2, 64) for d in (-1, 0, 1)})
    binned = 0
    for total in totals:
        for t_min in t_mins:
            for n_ranks in (1, 64, 65):
                geo = check_geometry(emul, total, t_min, n_ranks)
                binned += geo is not None
                if n_ranks == 65 or total > mc.MAX_BINS * 1024:
                    assert geo is None
    assert binned > 2000
    # at a power of two t_min uses nbins/2 + 1 bins and the average doubles; one below it uses them all
    full, half = check_geometry(emul, 200_000, (1 << 40) - 1, 4), check_geometry(emul, 200_000, 1 << 40, 4)
    assert (full[4], half[4]) == (256, 129) and half[1] == full[1] + 1 and half[2] > full[2]
    # an m = 1 merge of distinct entries near the top of a bin count: the region outgrows what a bin can rank
    assert check_geometry(emul, 262_144, 1 << 40, 4)[2] > mc.MAX_QUAL


@pytest.mark.parametrize("case", mc.all_cases(), ids=repr)
def test_case_through_the_emulator(emul, case):
    rk = mc.ranks(case)
    want = mr.merge(rk, case.k, case.s, case.m)
    total, t_min = mc.totals(rk)
    seen = set()
    for seed in SEEDS:
        flags, got, fills, quals, geo = run_binned(emul, case, rk, seed)
        seen.add(flags)
        if flags == 0:
            assert same(got, want), seed
        if flags >= 0:
            check_geometry(emul, total, t_min, len(rk))
            if case.name.startswith("uniform"):                       # below both limits, at the seeds committed
                assert fills.max() <= geo[2] and quals.max() <= mc.MAX_QUAL
            if case.name.startswith("one-bin"):
                assert fills[case.note["bin"]] > geo[2] and np.count_nonzero(fills) == 1
            if case.name.startswith("too-many"):
                assert quals.max() > mc.MAX_QUAL and fills.max() <= geo[2]
            if case.name.startswith("compaction"):
                assert np.flatnonzero(quals).tolist() == case.note["bins"] and geo[0] == 1024
                assert case.m == 1 or np.count_nonzero(fills) == 1024  # m = 2: entries in every bin, qualifiers in some
    assert seen == {-1 if case.flag is None else case.flag}           # exactly the flag the case is built for, whatever the order
    if case.flag != 0:                                                # the call goes on to the table path
        assert same(run_table(emul, case, rk, 5), want)


def test_headers_inside_the_slabs(emul):
    """the 8-word-header form of merge_gathered: the same results from slabs that carry their headers"""
    for name in ("uniform-seed12-m2-R3-t200000000000063", "t_min-10000000000-m1", "compaction-six-m2"):
        case = mc.by_name(name)
        rk = mc.ranks(case)
        flags, got, _, _, _ = run_binned(emul, case, rk, 4, hdr_words=8)
        assert flags == 0 and same(got, mr.merge(rk, case.k, case.s, case.m))


def test_nbins_step(emul):
    a = c_geometry(emul, *mc.totals(mc.ranks(mc.by_name("nbins-step-262144"))), 5)
    b = c_geometry(emul, *mc.totals(mc.ranks(mc.by_name("nbins-step-262145"))), 5)
    assert (a[0], b[0]) == (256, 512)


@pytest.mark.parametrize("n_ranks,own_rank", [(64, 0), (65, 63), (65, 64), (70, 69), (70, 5)])
def test_table_path_skips_the_own_slab(emul, n_ranks, own_rank):
    """the own rank's entries are in the table already: its slab -- in the first launch of 64 ranks or in the second -- is
    passed over, and every other one is not.  Shared with merge_slabs_impl are the ranks of a launch and the own slab's index
    within it (merge_launch_ranks, merge_launch_own); the loop over the launches and the skip itself are the emulator's own
    here, and slab_insert_kernel's are pinned on the device (test_gpu_merge_crafted.py, the cases with own reads)."""
    case = mc.many_ranks(n_ranks, own_rank, 2)
    rng = np.random.default_rng(own_rank)
    pool = np.concatenate([h[:int(hdr[0])] for hdr, h, _ in case.foreign[:8]])
    mine = np.unique(pool[rng.random(len(pool)) < 0.5])
    own = (mc.header(len(mine), MAX64 - 1), mine, rng.integers(1, 3, size=len(mine)).astype(np.uint32))
    rk = mc.ranks(case, own)
    want = mr.merge(rk, case.k, case.s, case.m)
    assert not isinstance(want, str)
    assert same(run_table(emul, case, rk, 6, log2_slots=14, own=own), want)
    # the same slabs with the own one NOT passed over count its entries twice: the rule sees the difference
    twice = mc.ranks(case, own)
    twice.append(own)
    assert not same(mr.merge(twice, case.k, case.s, case.m), want)
