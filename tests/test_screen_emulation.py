"""CPU emulation of the containment screen's table (auriclass_amd/csrc/mhx_screen.h, the very functions the kernels run):
table build, probe and tally, run sequentially by tests/emul/screen_emul.cpp, against a plain statement of the rule --
count(h) = occurrences of h among the probes, per reference the number of entries with a non-zero count and element
[len / 2] of their ascending counts."""
import ctypes

import numpy as np
import pytest

from tests import emul_build

MAXKEY = np.uint64(0xFFFFFFFFFFFFFFFF)


@pytest.fixture(scope="module")
def emul():
    L = emul_build.load("screen_emul")
    L.emul_screen.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint64,
                              ctypes.c_uint64] + [ctypes.c_void_p] * 4
    L.emul_screen.restype = ctypes.c_int64
    L.emul_screen_table_slots.argtypes = [ctypes.c_uint64]
    L.emul_screen_table_slots.restype = ctypes.c_uint64
    return L


def pack(refs):
    stride = max(1, max((len(r) for r in refs), default=1))
    rows = np.zeros((len(refs), stride), dtype=np.uint64)
    lens = np.zeros(len(refs), dtype=np.uint32)
    for i, r in enumerate(refs):
        rows[i, :len(r)] = r
        lens[i] = len(r)
    return rows, lens


def run(L, refs, probes, slots=0):
    rows, lens = pack(refs)
    probes = np.ascontiguousarray(probes, dtype=np.uint64)
    counts = np.zeros(rows.shape, dtype=np.uint32)
    shared = np.zeros(len(refs), dtype=np.uint32)
    median = np.zeros(len(refs), dtype=np.uint32)
    t = ctypes.c_uint64(0)
    occ = L.emul_screen(rows.ctypes.data, lens.ctypes.data, len(refs), rows.shape[1], probes.ctypes.data, probes.size, slots,
                        counts.ctypes.data, shared.ctypes.data, median.ctypes.data, ctypes.byref(t))
    return occ, counts, shared, median, t.value


def rule(refs, probes):
    """The plain statement: per reference (counts per entry, shared, median)."""
    values, occurrences = np.unique(np.asarray(probes, dtype=np.uint64), return_counts=True)
    out = []
    for r in refs:
        r = np.asarray(r, dtype=np.uint64)
        at = np.searchsorted(values, r)
        at_c = np.minimum(at, max(values.size - 1, 0))
        hit = (at < values.size) & (values[at_c] == r) if values.size else np.zeros(r.size, bool)
        c = np.where(hit, occurrences[at_c] if values.size else 0, 0).astype(np.uint64)
        nz = np.sort(c[c > 0])
        out.append((c, int(nz.size), int(nz[nz.size // 2]) if nz.size else 0))
    return out


def check(L, refs, probes, slots=0):
    occ, counts, shared, median, t = run(L, refs, probes, slots)
    want = rule(refs, probes)
    distinct = np.unique(np.concatenate([np.asarray(r, np.uint64) for r in refs] + [np.zeros(0, np.uint64)]))
    assert occ == int((distinct != MAXKEY).sum())           # duplicates across references collapse into one key
    assert t == (int(distinct.max()) if distinct.size else 0)
    for i, (c, s, m) in enumerate(want):
        assert np.array_equal(counts[i, :len(refs[i])].astype(np.uint64), c), i
        assert (int(shared[i]), int(median[i])) == (s, m), i
    return occ


def random_case(seed, bits, nr, n, dup=0.7, nprobes=20000):
    rng = np.random.default_rng(seed)
    hi = 1 << bits
    pool = np.unique(rng.integers(0, hi, size=2 * n, dtype=np.uint64))
    base = np.sort(rng.choice(pool, size=min(n, pool.size), replace=False))
    refs = []
    for _ in range(nr):                                   # a "clade": most hashes shared with the first reference
        keep = base[rng.random(base.size) < dup]
        own = np.unique(rng.integers(0, hi, size=max(1, n // 4), dtype=np.uint64))
        refs.append(np.unique(np.concatenate([keep, own])))
    # probes: reference hashes with skewed multiplicities (a few hashes drawn very often), and foreign hashes
    allh = np.unique(np.concatenate(refs))
    heavy = rng.choice(allh, size=min(16, allh.size), replace=False)
    probes = np.concatenate([rng.choice(allh, size=nprobes), np.repeat(heavy, 300), rng.integers(0, hi, size=nprobes, dtype=np.uint64)])
    rng.shuffle(probes)
    return refs, probes


@pytest.mark.parametrize("seed,bits,nr,n", [(1, 64, 4, 500), (2, 64, 24, 2000), (3, 32, 5, 800), (4, 32, 1, 50), (5, 64, 1, 1),
                                            (6, 12, 6, 900), (7, 64, 40, 64)])
def test_random_reference_sets_with_duplicates(emul, seed, bits, nr, n):
    refs, probes = random_case(seed, bits, nr, n)
    check(emul, refs, probes)


def test_empty_and_one_entry_references(emul):
    rng = np.random.default_rng(11)
    full = np.unique(rng.integers(0, 1 << 64, size=300, dtype=np.uint64))
    refs = [full, np.zeros(0, np.uint64), full[7:8], np.zeros(0, np.uint64)]
    probes = np.concatenate([np.repeat(full[:100], 3), np.repeat(full[7:8], 40)])
    occ, counts, shared, median, _ = run(emul, refs, probes)
    check(emul, refs, probes)
    assert list(shared) == [100, 0, 1, 0] and list(median[1:]) == [0, 43, 0]
    # nothing probed at all: every row is 0 / n / 0
    check(emul, refs, np.zeros(0, np.uint64))
    # no reference at all
    assert run(emul, [], probes)[0] == 0


def test_the_key_that_cannot_live_in_the_table(emul):
    rng = np.random.default_rng(12)
    body = np.unique(rng.integers(0, 1 << 64, size=200, dtype=np.uint64))
    body = body[body != MAXKEY]
    with_max = np.concatenate([body, [MAXKEY]])
    refs = [with_max, body[:50], np.array([MAXKEY], np.uint64)]
    probes = np.concatenate([np.repeat(body, 2), np.full(9, MAXKEY, np.uint64), body[:10]])
    occ = check(emul, refs, probes)
    assert occ == body.size
    _, counts, shared, median, t = run(emul, refs, probes)
    assert counts[0, body.size] == 9 and counts[2, 0] == 9 and t == int(MAXKEY)
    assert (int(shared[2]), int(median[2])) == (1, 9)
    # the value is a key nowhere: its occurrences change nothing
    check(emul, [body], probes)


def test_table_at_its_fill_limit(emul):
    """screen_table_slots gives at least two slots per entry; a table exactly half full of distinct keys, all of which
    collide into a few runs, still finds every key and still ends every miss at a vacant slot."""
    assert emul.emul_screen_table_slots(0) == 1024 and emul.emul_screen_table_slots(512) == 1024
    assert emul.emul_screen_table_slots(513) == 2048 and emul.emul_screen_table_slots(1_200_000) == 1 << 22
    rng = np.random.default_rng(13)
    n = 2048                                              # -> 4096 slots, half full
    low = rng.integers(0, 64, size=n, dtype=np.uint64)    # every key starts its walk in the first 64 slots
    keys = np.unique((rng.integers(0, 1 << 52, size=n, dtype=np.uint64) << np.uint64(12)) | low)
    while keys.size < n:
        extra = (rng.integers(0, 1 << 52, size=n, dtype=np.uint64) << np.uint64(12)) | rng.integers(0, 64, size=n, dtype=np.uint64)
        keys = np.unique(np.concatenate([keys, extra]))[:n]
    assert emul.emul_screen_table_slots(keys.size) == 4096
    misses = (rng.integers(0, 1 << 52, size=5000, dtype=np.uint64) << np.uint64(12)) | rng.integers(0, 64, size=5000, dtype=np.uint64)
    probes = np.concatenate([np.repeat(keys, 2), misses, keys[::3]])
    assert check(emul, [keys], probes) == n
    # the same keys split over two references that share half of them
    assert check(emul, [keys[: n // 2 + n // 4], keys[n // 4:]], probes, slots=4096) == n
    # a table that is too small for its keys reports it instead of walking for ever
    assert run(emul, [keys], probes, slots=1024)[0] == -1


def test_median_selection_on_crafted_counts(emul):
    """element [len / 2] of the ascending non-zero counts, for counts that differ only in high, middle or low bytes"""
    for counts in ([1], [1, 2], [5, 5, 5, 5], [1, 70000, 70001, 3], [256, 255, 257, 65536, 65535, 1], [3, 0, 0, 9, 0, 4, 0],
                   [1000] * 7 + [1] * 6, [2, 1, 2, 1, 2, 1]):
        keys = (np.arange(len(counts), dtype=np.uint64) + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
        order = np.argsort(keys)
        keys = keys[order]
        c = np.asarray(counts)[order]
        probes = np.repeat(keys, c)
        _, got_counts, shared, median, _ = run(emul, [keys], probes)
        nz = sorted(x for x in counts if x)
        assert int(shared[0]) == len(nz) and int(median[0]) == nz[len(nz) // 2], counts
        assert list(got_counts[0]) == list(c)
