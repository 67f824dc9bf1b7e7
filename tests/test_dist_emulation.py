"""CPU emulation of the all-vs-refs distance path (auriclass_amd/csrc/mhx_dist.h, the very functions the dist_* kernels of
mhx_dist.hip run): tests/emul/dist_emul.cpp runs them sequentially over whole batches -- shift, split pass, range
pass, window totals, finish walk -- in the base form (1024 value ranges) and in the windowed form (1024 x W ranges for
lists of more than 65 536 hashes); `common` and `denom` of every pair against the oracle's compareSketches."""
import ctypes

import numpy as np
import pytest

from oracle import mash_oracle as mo
from tests import emul_build
from tests import extreme_cases as xc

WORST_HI = int(2 ** 63.01)   # the scale is rounded up to a power of two: values just above 2^63 leave half of the ranges in use


@pytest.fixture(scope="module")
def emul():
    L = emul_build.load("dist_emul")
    L.emul_dist_windows.argtypes = [ctypes.c_uint64]
    L.emul_dist_windows.restype = ctypes.c_uint32
    L.emul_dist_max_windows.restype = ctypes.c_uint32
    L.emul_dist_wide_max_queries.argtypes = [ctypes.c_uint32, ctypes.c_uint32]
    L.emul_dist_wide_max_queries.restype = ctypes.c_uint32
    L.emul_dist.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32,
                            ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    L.emul_dist.restype = ctypes.c_int
    return L


def sketch_like(rng, n, hi=2 ** 64):
    return np.unique(rng.integers(0, hi, size=n, dtype=np.uint64))


def pad_rows(lists, stride):
    M = np.zeros((len(lists), stride), np.uint64)
    for i, v in enumerate(lists):
        M[i, :len(v)] = v
    return M, np.array([len(v) for v in lists], np.uint32)


def clade_refs(rng, s, hi=2 ** 64, nr=24):
    """References as in test_dist_all_vs_refs_fast_path_equals_oracle: 11 close to a base list, the others half fresh, one
    shorter than s."""
    base = sketch_like(rng, s, hi)
    refs = []
    for j in range(nr):
        keep = rng.random(len(base)) >= (0.002 * (j + 1) if j < 11 else 0.5)
        refs.append(np.unique(np.concatenate([base[keep], sketch_like(rng, int((~keep).sum()), hi)])))
    refs[3] = refs[3][:s - (s * 15) // 100]
    return refs


def clade_queries(rng, refs, nq, hi=2 ** 64):
    qrys = []
    for i in range(nq):
        src = refs[i % len(refs)]
        keep = rng.random(len(src)) >= 0.6 * i / max(1, nq - 1)
        qrys.append(np.unique(np.concatenate([src[keep], sketch_like(rng, int((~keep).sum()), hi)])))
    return qrys


def lane_forms_batch():
    """The batch of test_dist_one_query_per_lane_forms_equal_oracle (tests/test_gpu_parity.py)."""
    rng = np.random.default_rng(41)
    s = 4000
    base = sketch_like(rng, s)
    refs = []
    for j in range(24):
        keep = rng.random(len(base)) >= (0.002 * (j + 1) if j < 11 else 0.5)
        refs.append(np.unique(np.concatenate([base[keep], sketch_like(rng, int((~keep).sum()))])))
    qrys = []
    for i in range(150):
        src = refs[i % 24]
        keep = rng.random(len(src)) >= 0.6 * i / 149
        qrys.append(np.unique(np.concatenate([src[keep], sketch_like(rng, int((~keep).sum()))])))
    qrys[5] = refs[5].copy()
    qrys[6] = qrys[6][:17]
    qrys[7] = np.zeros(0, np.uint64)
    qrys[8] = qrys[8][:len(qrys[8]) // 3]
    qrys[9] = qrys[9][qrys[9] >= np.uint64(1 << 63)]
    qrys[10] = qrys[10][::7]
    return qrys, refs, s


def run_emul(L, qrys, refs, s, windows=0):
    stride = (max(max(map(len, refs)), max(map(len, qrys)), 1) + 15) // 16 * 16
    Q, ql = pad_rows(qrys, stride)
    R, rl = pad_rows(refs, stride)
    common = np.full((len(qrys), len(refs)), 0xFFFFFFFF, np.uint32)
    denom = np.full((len(qrys), len(refs)), 0xFFFFFFFF, np.uint32)
    stats = np.zeros(4, np.uint32)
    rc = L.emul_dist(Q.ctypes.data, ql.ctypes.data, len(qrys), R.ctypes.data, rl.ctypes.data, len(refs), stride, s, windows,
                     common.ctypes.data, denom.ctypes.data, stats.ctypes.data)
    return rc, common, denom, stats


def check_pairs(common, denom, qrys, refs, s, k=27):
    for qi, q in enumerate(qrys):
        for ri, r in enumerate(refs):
            c, d, _ = mo.compare(r, q, s, k)
            assert (int(common[qi, ri]), int(denom[qi, ri])) == (c, d), (qi, ri, len(q), len(r))


@pytest.mark.parametrize("windows", [1, 2, 16])
def test_small_lists_in_every_geometry(emul, windows):
    """Empty, tiny and truncated queries, one with nothing in the lower half of the value space, a query equal to a reference:
    in the base form and with W forced to 2 and 16 on the same lists of 4000 (most of the 16 384 ranges are then empty)."""
    qrys, refs, s = lane_forms_batch()
    rc, common, denom, stats = run_emul(emul, qrys, refs, s, windows)
    assert rc == 0 and stats[0] == 1024 * windows
    check_pairs(common, denom, qrys, refs, s)


def test_small_lists_get_the_base_form_from_the_rule(emul):
    qrys, refs, s = lane_forms_batch()
    rc, common, denom, stats = run_emul(emul, qrys[:12], refs, s)
    assert rc == 0 and stats[0] == 1024
    check_pairs(common, denom, qrys[:12], refs, s)


@pytest.mark.parametrize("s,hi,ranges", [(70_000, 2 ** 64, 2048), (250_000, 2 ** 64, 4096), (250_000, WORST_HI, 4096),
                                         (1_000_000, 2 ** 64, 16384)])
def test_long_lists_with_the_rules_own_geometry(emul, s, hi, ranges):
    """Clade-shaped references of 70 000, 250 000 and 1 000 000 hashes: the rule gives 2048, 4096 and 16 384 ranges, no slice
    outgrows the byte counters, no range the table, and every pair is the oracle's."""
    rng = np.random.default_rng(71)
    refs = clade_refs(rng, s, hi)
    qrys = clade_queries(rng, refs, 5, hi)
    qrys[2] = qrys[2][:len(qrys[2]) // 3]
    qrys[3] = qrys[3][::5]
    rc, common, denom, stats = run_emul(emul, qrys, refs, s)
    print("s", s, "ranges", stats[0], "longest slice", stats[1], "most distinct keys in a range", stats[2], "shift", stats[3])
    assert rc == 0 and stats[0] == ranges
    assert stats[1] <= 255 and stats[2] <= 1536
    check_pairs(common, denom, qrys, refs, s)


def test_crowded_values_raise_the_flag(emul):
    """The construction of test_dist_non_uniform_values_fall_back_to_the_generic_kernel: the emulated range pass gives the
    block up (the generic kernel's case), in the base form and in a forced windowed one."""
    rng = np.random.default_rng(22)
    lo = 1 << 62
    refs = [lo + sketch_like(rng, 3000, hi=2 ** 20) for _ in range(8)]
    refs.append(np.concatenate([refs[0][:1000], np.array([2 ** 64 - 5], np.uint64)]))
    qrys = [np.unique(np.concatenate([refs[i % 8][::2], lo + sketch_like(rng, 1500, hi=2 ** 20)])) for i in range(4)]
    for windows in (0, 4):
        rc, _, _, stats = run_emul(emul, qrys, refs, 3000, windows)
        assert rc == 1 and stats[2] > 1536


def test_geometry_rule(emul):
    """W from the longest list alone: 1 up to 65 536 entries, 16 at 1 000 000 and at 2^20, powers of two, monotone, the
    smallest W with longest / (1024 W) <= 64; nothing (the generic kernel) beyond the largest W."""
    w = emul.emul_dist_windows
    wmax = emul.emul_dist_max_windows()
    assert wmax >= 16
    for n in (0, 1, 17, 1000, 50_000, 65_535, 65_536):
        assert w(n) == 1, n
    assert w(65_537) == 2 and w(131_072) == 2 and w(131_073) == 4
    assert w(250_000) == 4 and w(500_000) == 8 and w(1_000_000) == 16 and w(1 << 20) == 16
    last = 1
    for n in list(range(1, 1 << 20, 4099)) + [(1 << 20)] + [65_536 * m + d for m in (1, 2, 4, 8, 16) for d in (-1, 0, 1)]:
        got = w(n)
        if n > 65_536 * wmax:
            assert got == 0, n
            continue
        assert got >= 1 and got & (got - 1) == 0 and got <= wmax
        assert n <= 65_536 * got and (got == 1 or n > 65_536 * got // 2), (n, got)   # the smallest W that fits
    for n in sorted(range(1, 65_536 * wmax + 1, 65_521)):
        assert w(n) >= last
        last = w(n)
    assert w(65_536 * wmax + 1) == 0 and w(1 << 31) == 0 and w(1 << 40) == 0


def test_batches_of_the_windowed_form_keep_32_bit_indices(emul):
    """The host bounds a windowed block's workspace (256 MiB); the bound is what keeps the kernels' q * (R + 1) products and
    the window kernel's work item count below 2^32."""
    for ranges in (2048, 4096, 8192, 16384):
        for nr in (1, 5, 24, 32):
            n = emul.emul_dist_wide_max_queries(nr, ranges)
            cell = 4 * ((nr + 3) // 4)
            work = 4 * (ranges + 1) * (n + nr) + ranges * n * cell + (ranges // 64) * n * cell * 4 + 4 * 256
            assert n >= 1 and work <= 256 << 20
            assert n * (ranges + 1) < 2 ** 32 and n * ranges * cell < 2 ** 32


def run_slices(L, qrys, refs, s, windows=0):
    """the references in slices of 32, as the host cuts them: one emulated block each"""
    out = [run_emul(L, list(qrys), list(refs[r0:r0 + 32]), s, windows) for r0 in range(0, len(refs), 32)]
    return [o[0] for o in out], np.hstack([o[1] for o in out]), np.hstack([o[2] for o in out]), [o[3] for o in out]


def assert_matrix(common, denom, want, what):
    bad = np.argwhere((common != want[0]) | (denom != want[1]))
    assert bad.size == 0, (what, [(int(q), int(r), int(common[q, r]), int(want[0][q, r]), int(denom[q, r]), int(want[1][q, r])) for q, r in bad[:6]])


@pytest.mark.parametrize("windows", [0, 2])
@pytest.mark.parametrize("mirrored", [False, True])
def test_the_vacant_slot_marker_as_a_hash(emul, mirrored, windows):
    """2^64 - 1 (kEmptyKey) in lists that reach the range table, next to values of the same home slot: the planted batch of
    tests/extreme_cases.py, references inserted in index order, in the base form and with W forced to 2.  Every pair is the
    oracle's, and the block stays on the fast path.
    Observed before the range table kept 2^64 - 1 out of its slots (dist_table_insert_plain took it for a key, the slot
    stayed vacant with the reference's bit on it), in both geometries, as common/denom against the oracle's --
    plain: (query 0, reference 0) 424/476 for 423/477, one too high; (query 1, reference 0) 0/897 for 1/896 and (query 6,
    reference 0: the same list twice) 449/451 for 450/450, one too low;
    mirrored: (query 0, reference 8) 1/897 for 0/898; (query 1, reference 8) 0/894 for 1/893; (query 6, reference 8) 446/448
    for 447/447; every other pair right."""
    qrys, refs, s = xc.batch(40, mirrored)
    rc, common, denom, stats = run_slices(emul, qrys, refs, s, windows)
    assert rc == [0, 0] and all(st[0] == (1024 if not windows else 2048) and st[3] == (54 if not windows else 53) for st in stats)
    assert_matrix(common, denom, xc.batch_expected(40, mirrored), "mirrored" if mirrored else "plain")


@pytest.mark.parametrize("case,args,shift", [("with_zero", (), 54), ("below_the_ranges", (1024, 300, 1000), 0), ("below_the_ranges", (16, 10, 16), 0),
                                             ("power_of_two_top", (40, False), 30), ("power_of_two_top", (40, True), 31)])
def test_values_uniform_draws_never_produce(emul, case, args, shift):
    """hash 0 in zero-padded rows; every value below the number of ranges (shift 0); the largest value exactly 2^40 - 1 and
    exactly 2^40"""
    qrys, refs, s = getattr(xc, case)(*args)
    rc, common, denom, stats = run_slices(emul, qrys, refs, s)
    assert rc == [0, 0] and all(st[0] == 1024 and st[3] == shift for st in stats)
    assert_matrix(common, denom, xc.oracle_matrix(qrys, refs, s), case)
