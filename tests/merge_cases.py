"""Crafted slabs for the sharded path's merge (mhx_merge.hip, merge_slabs_impl), shared by the CPU tests (rule, emulator) and
the GPU test.  A case holds every rank but its own as data -- header and slab, written by hand --; the own rank is a real
sketcher on the GPU and an empty one (n = 0, T = hash_max) on the CPU, and enters as data too: ranks(case, own).

Every generator is seeded.  What a case is built for is written in its fields: `flag`, the one flag the binned attempt
must return (0: none; None: the call is not the binned path's), `path`, where the answer must come from when the own
sketcher has `expected_bytes`, and `own_reads`, the reads of synthetic FASTQ the own sketcher is pushed first."""
import functools
import math
from dataclasses import dataclass, field

import numpy as np

from tests import merge_rule as mr

MAX64, MAX32 = mr.MAX64, mr.MAX32
BINNED, TABLE, HOST = 1, 2, 3          # engine.MERGE_BINNED, MERGE_TABLE, MERGE_HOST
MAX_RANKS, MAX_BINS, MAX_SLOTS, MAX_QUAL = 64, 16384, 4096, 1024   # mhx_merge.h (test_merge_emulation.py compares them)


@dataclass
class Case:
    name: str
    k: int
    s: int
    m: int
    own_rank: int
    foreign: list                      # [(header uint64[8], hashes uint64[>= n], counts uint32[>= n])] in rank order, own left out
    flag: object = 0
    path: int = BINNED
    expected_bytes: int = 0
    own_reads: int = 0
    note: dict = field(default_factory=dict)   # what the generator aimed at (bin, value, ...), for the CPU checks of intent

    @property
    def n_ranks(self):
        return len(self.foreign) + 1

    def __repr__(self):
        return self.name


def fin_cap(s):
    return (s + 16 * math.isqrt(s) + 4097) & ~1


def geometry(total, t_min, n_ranks):
    """merge_geometry of mhx_merge.h: (nbins, shift, region, table_slots, bins_used), or None when not the binned path"""
    if n_ranks > MAX_RANKS or total == 0 or total > MAX_BINS * 1024:
        return None
    nbins = 256
    while nbins * 1024 < total:
        nbins *= 2
    lg, bits = nbins.bit_length() - 1, (t_min | 1).bit_length()
    shift = bits - lg if bits > lg else 0
    used = (t_min >> shift) + 1
    avg = total / used
    region = int(avg + 6.0 * math.sqrt(avg) + 64.0)
    slots = 256
    while slots * 3 // 4 < region:
        slots *= 2
    return (nbins, shift, region, slots, used) if slots <= MAX_SLOTS else None


def header(n, T, maxkey=0):
    return np.array([n, T, 0, maxkey, n, 0, 0, 0], dtype=np.uint64)


def empty_own(k):
    """what an empty sketcher exports: nothing, below a threshold that never fell"""
    return header(0, mr.hash_max(k)), np.zeros(0, np.uint64), np.zeros(0, np.uint32)


def ranks(case, own=None):
    """all ranks of a case, the own one -- (header, hashes, counts) -- in its place"""
    out = list(case.foreign)
    out.insert(case.own_rank, own if own is not None else empty_own(case.k))
    return out


def totals(rk):
    return sum(int(h[0]) for h, _, _ in rk), mr.t_min_of(rk)


def layout(rk, hdr_words=0, own_rank=None):
    """the gathered buffer: one slab [hdr_words of header | hashes[cap] | counts u32[cap]] per rank, as uint64 words; the
    room behind a rank's data is filled with a pattern that would show.  own_rank: that slab is left to the caller."""
    cap = max(2, max(len(h) for _, h, _ in rk) + 7) & ~1
    words = hdr_words + cap + cap // 2
    buf = np.full(len(rk) * words, 0x0123456789ABCDEF, dtype=np.uint64)
    for r, (hdr, h, c) in enumerate(rk):
        if r == own_rank:
            continue
        at = r * words
        if hdr_words:
            buf[at:at + hdr_words] = hdr[:hdr_words]
        buf[at + hdr_words:at + hdr_words + len(h)] = h
        buf[at + hdr_words + cap:at + words].view(np.uint32)[:len(c)] = c
    return buf, cap


def _below(rng, n, limit):
    """n distinct random values <= limit (fewer when there are not that many), never 2^64-1"""
    if limit < 4 * n:
        v = np.arange(limit + 1, dtype=np.uint64)
        return rng.permutation(v)[:n]
    v = rng.integers(0, MAX64, size=2 * n + 16, dtype=np.uint64, endpoint=True)
    if limit < MAX64:
        v %= np.uint64(limit + 1)
    v = np.unique(v[v != np.uint64(MAX64)])
    return rng.permutation(v)[:n]


def _rank(rng, values, counts, T, junk=0, maxkey=0):
    """one foreign rank: the entries shuffled, `junk` entries that would change the result behind n"""
    order = rng.permutation(len(values))
    h, c = np.asarray(values, np.uint64)[order], np.asarray(counts, np.uint32)[order]
    n = len(h)
    if junk:
        h = np.concatenate([h, h[:junk] if n >= junk else np.arange(junk, dtype=np.uint64)])
        c = np.concatenate([c, np.full(len(h) - n, 1000, np.uint32)])
    return header(n, T, maxkey), h, c


def uniform(seed, m, n_foreign, t_min, s=200, pool=1500, k=21, own_rank=0, own_reads=0, name=None):
    """random values <= t_min; every rank holds about half of the pool with counts 1 .. 3, so the sums straddle m; the
    first foreign rank has T = t_min, the others a larger T and some entries between t_min and their T (not evidence)"""
    rng = np.random.default_rng(seed)
    values = _below(rng, pool, t_min)
    foreign = []
    for r in range(n_foreign):
        T = t_min if r == 0 or t_min >= mr.hash_max(k) else min(MAX64 - 1, t_min + int(rng.integers(1, 1 << 20)) * (1 + (t_min >> 8)))
        mine = values[rng.random(len(values)) < 0.5]
        cnt = rng.integers(1, 4, size=len(mine))
        above = np.unique(rng.integers(t_min + 1, T, size=50, dtype=np.uint64, endpoint=True)) if T > t_min else np.zeros(0, np.uint64)
        foreign.append(_rank(rng, np.concatenate([mine, above]), np.concatenate([cnt, np.full(len(above), 5)]), T, junk=16))
    return Case(name or f"uniform-seed{seed}-m{m}-R{n_foreign + 1}-t{t_min:x}", k, s, m, own_rank, foreign, own_reads=own_reads)


T_EDGES = (0, 1, 255, (1 << 40) - 1, 1 << 40, (1 << 40) + 1, MAX32, MAX64 - 1, MAX64)


def t_min_edge(t_min, m, maxkey_sum=0, seed=7):
    """one entry equal to t_min and one at t_min + 1, junk behind n[r], a 2^64-1 in front of it; at t_min = 2^32-1 the
    sketcher has k = 16 and every T is hash_max, at 2^64-1 header word 3 of the foreign ranks sums to `maxkey_sum`"""
    rng = np.random.default_rng(seed + t_min % 1000003)
    k = 16 if t_min == MAX32 else 21
    top = t_min >= mr.hash_max(k)                    # nobody ever rejected anything: a short sketch is the sketch
    values = _below(rng, 150 if top else 1200, t_min)
    values = values[values != np.uint64(t_min)]
    foreign = []
    for r in range(3):
        T = t_min if r == 0 or top else (t_min + 1 + r if t_min + 1 + r < MAX64 else MAX64 - 1 if r == 1 else MAX64)
        mine = values[rng.random(len(values)) < 0.6]
        h = [mine, np.array([t_min], np.uint64)]
        c = [rng.integers(1, 4, size=len(mine)), np.array([m if r == 0 else 1])]
        if t_min < MAX64 and (r > 0 or top):         # (a rank holds nothing above its own T, but for k = 16 the slab is data)
            h.append(np.array([t_min + 1], np.uint64))
            c.append(np.array([m + 5]))
        if t_min < MAX64 - 1:
            h.append(np.array([MAX64], np.uint64))    # a vacant slot's key inside the valid part
            c.append(np.array([m + 7]))
        mk = (maxkey_sum // 2 + (maxkey_sum & 1 if r == 0 else 0)) if t_min == MAX64 and r < 2 else 0
        foreign.append(_rank(rng, np.concatenate(h), np.concatenate(c), T, junk=16, maxkey=mk))
    return Case(f"t_min-{t_min:x}-m{m}" + (f"-maxkey{maxkey_sum}" if t_min == MAX64 else ""), k, 200, m, 1, foreign)


def nbins_step(total):
    """four foreign ranks, `total` entries in all: 262 144 is the last total with 256 bins.  m = 2 and every value on two
    ranks with count 1: 512 distinct values per bin on average -- with m = 1 and distinct values 1024 per bin would
    qualify, which is the too-many-qualify case"""
    rng = np.random.default_rng(total)
    t_min = MAX64 - 1
    values = _below(rng, total // 2 + 1, t_min)
    assert len(values) == total // 2 + 1
    pairs, quarter = values[:total // 2], total // 4
    parts = [pairs[:quarter], pairs[quarter:], pairs[:quarter], np.concatenate([pairs[quarter:], values[total // 2:][:total & 1]])]
    foreign = [_rank(rng, v, np.ones(len(v)), t_min) for v in parts]
    assert sum(len(v) for v in parts) == total
    return Case(f"nbins-step-{total}", 21, 1000, 2, 2, foreign)


def one_bin(path=TABLE, n_total=40_000, n_foreign=5):
    """every foreign value in bin 77 of 129, with random low bits: far more than the bin's region holds (flag 1)"""
    rng = np.random.default_rng(77)
    t_min = 1 << 40
    nbins, shift, region, _, _ = geometry(n_total, t_min, n_foreign + 1)
    assert n_total > 4 * region
    values = (np.uint64(77) << np.uint64(shift)) | _below(rng, n_total, (1 << shift) - 1)
    per = n_total // n_foreign
    foreign = [_rank(rng, values[r * per:(r + 1) * per], np.ones(per), t_min + (r > 0)) for r in range(n_foreign)]
    return Case(f"one-bin-{'host' if path == HOST else 'table'}", 21, 1000, 1, 0, foreign, flag=1, path=path, expected_bytes=int(path == HOST),
                note={"bin": 77})


def too_many_qualify(path=TABLE, n_total=160_000, n_foreign=4):
    """m = 1, t_min = 2^40, distinct uniform values: ~1250 of them in each of 128 bins, all of which qualify, under a
    region of 1515 entries (flag 4 and no other)"""
    rng = np.random.default_rng(4)
    t_min = 1 << 40
    _, _, region, _, used = geometry(n_total, t_min, n_foreign + 1)
    fill = n_total / (used - 1)
    assert fill - 4 * math.sqrt(fill) > MAX_QUAL and fill + 6 * math.sqrt(fill) < region
    values = _below(rng, n_total, t_min - 1)
    per = n_total // n_foreign
    foreign = [_rank(rng, values[r * per:(r + 1) * per], np.ones(per), t_min + (r > 0)) for r in range(n_foreign)]
    return Case(f"too-many-qualify-{'host' if path == HOST else 'table'}", 21, 1000, 1, 4, foreign, flag=4, path=path,
                expected_bytes=int(path == HOST))


COMPACT_FILL = 524_289          # entries above t_min that only make the total large: 1024 bins, four compaction workgroups


def compaction(variant, m):
    """1024 bins in use, qualifying entries where the variant puts them; for m = 2 every qualifier is two entries of count
    1 on two ranks, and single entries that do not qualify lie in the bins that have to come out empty"""
    rng = np.random.default_rng(1024 + m)
    t_min = (1023 << 54) + 5
    shift, nbins = 54, 1024
    s = 200
    if variant == "six":                 # both sides of the workgroup boundaries at 256 and 512, the first and the last bin
        per_bin = {0: 40, 255: 40, 256: 40, 511: 40, 512: 40, nbins - 1: 5}
    elif variant == "alternate":         # every other bin empty
        per_bin, s = {b: 3 for b in range(0, nbins, 2)}, 1000
    elif variant == "span":              # a sketch out of 417 bins, two workgroups' worth
        per_bin, s = {b: 12 for b in range(nbins)}, 5000
    elif variant == "overfull":          # 7168 qualify, the block holds fin_cap(200) = 4520: cut inside bin 645's run
        per_bin = {b: 7 for b in range(nbins)}
    else:
        raise ValueError(variant)
    quals, decoys = [], []
    for b in range(nbins):
        width = 6 if b == nbins - 1 else 1 << shift
        low = _below(rng, per_bin.get(b, 0) + 1, width - 1)
        vals = (np.uint64(b) << np.uint64(shift)) | low
        quals.append(vals[:per_bin.get(b, 0)])
        if m > 1 and b not in per_bin:
            decoys.append(vals[-1:])
    quals = np.concatenate(quals)
    decoys = np.concatenate(decoys) if decoys else np.zeros(0, np.uint64)
    filler = np.uint64(t_min + 1) + np.arange(COMPACT_FILL, dtype=np.uint64) * np.uint64(3)
    half = COMPACT_FILL // 2

    def ones(v):
        return np.ones(len(v), np.uint32)

    if m == 1:
        a, b = quals[::2], quals[1::2]
    else:
        a, b = quals, np.concatenate([quals, decoys])
    foreign = [_rank(rng, a, ones(a), t_min), _rank(rng, b, ones(b), t_min + 1),
               _rank(rng, filler[:half], ones(filler[:half]), MAX64 - 1), _rank(rng, filler[half:], ones(filler[half:]), MAX64 - 1)]
    return Case(f"compaction-{variant}-m{m}", 21, s, m, 1, foreign, note={"bins": sorted(per_bin)})


def many_ranks(n_ranks, own_rank, m, own_reads=0):
    """a few dozen entries per rank: 64 ranks are the binned path's most, 65 and 70 take the table path in two launches.
    With own reads T_min is 2^62+3: a quarter of the own sketcher's ~30 000 hashes lie below it and make up most of the
    first s, so an own slab counted twice (or not at all) changes the sketch"""
    rng = np.random.default_rng(n_ranks * 100 + own_rank)
    t_min = ((1 << 62) if own_reads else (1 << 50)) + 3
    values = _below(rng, 1500, t_min)
    foreign = []
    for r in range(n_ranks - 1):
        mine = values[rng.permutation(len(values))[:40]]
        foreign.append(_rank(rng, mine, rng.integers(1, 4, size=40), t_min + (r % 3), junk=4))
    return Case(f"ranks-{n_ranks}-own{own_rank}-m{m}" + ("-reads" if own_reads else ""), 21, 200, m, own_rank, foreign,
                flag=0 if n_ranks <= MAX_RANKS else None, path=BINNED if n_ranks <= MAX_RANKS else TABLE, own_reads=own_reads)


WRAP_VALUE = 0x1234_5678_9ABC


def counts_exact(m):
    """m foreign ranks: 300 values with count 1 on each of them (a sum of exactly m), 300 with count 0 on one (m - 1)"""
    rng = np.random.default_rng(300 + m)
    t_min = 1 << 45
    values = _below(rng, 600, t_min)
    foreign = []
    for r in range(m):
        c = np.ones(600, np.uint32)
        if r == m - 1:
            c[300:] = 0
        foreign.append(_rank(rng, values, c, t_min + r))
    return Case(f"counts-exact-m{m}", 21, 200, m, m, foreign)


def counts_wrap(n_foreign, m):
    """one value whose counts sum to 0xFFFFFFFF + 1 (two foreign ranks) or n_foreign * 0xFFFFFFFF, among 400 ordinary ones:
    the rule keeps it with the count 2^32-1.  Up to 63 foreign ranks the binned merge sees the 32-bit sum wrap (flag 8) and
    the table path answers; 64 foreign ranks are the table path's from the start."""
    rng = np.random.default_rng(800 + n_foreign)
    t_min = 1 << 48
    values = _below(rng, 400, t_min)
    values = values[values != np.uint64(WRAP_VALUE)]
    foreign = []
    for r in range(n_foreign):
        mine = values[rng.random(len(values)) < (0.7 if n_foreign == 2 else 0.1)]
        big = 1 if (n_foreign == 2 and r == 1) else MAX32
        foreign.append(_rank(rng, np.concatenate([mine, np.array([WRAP_VALUE], np.uint64)]),
                             np.concatenate([np.full(len(mine), m), np.array([big])]), t_min + r))
    binned = n_foreign + 1 <= MAX_RANKS
    return Case(f"counts-wrap-{n_foreign}x-m{m}", 21, 200, m, 0, foreign, flag=8 if binned else None, path=TABLE, note={"value": WRAP_VALUE})


def short(path):
    """fewer than s = 200 qualify below a T_min < hash_max: MHX_E_CAPACITY from the binned path, the table path (65 ranks)
    and the host merge (65 ranks of 520 entries on a sketcher with a 2^16-slot table)"""
    rng = np.random.default_rng(50 + path)
    t_min = 1 << 40
    if path == BINNED:
        values = _below(rng, 150, t_min)
        subsets = [values[rng.random(len(values)) < 0.7] for _ in range(3)]
        foreign = [_rank(rng, sub, np.ones(len(sub)), t_min + r) for r, sub in enumerate(subsets)]
        return Case("short-binned", 21, 200, 1, 3, foreign)
    per = 2 if path == TABLE else 520
    foreign = []
    for r in range(64):
        low = _below(rng, 2, t_min)
        high = np.uint64(t_min + 1) + _below(rng, per - 2, 1 << 50)
        v = np.concatenate([low, high])
        foreign.append(_rank(rng, v, np.ones(len(v)), t_min if r == 0 else 1 << 52))
    return Case(f"short-{'table' if path == TABLE else 'host'}", 21, 200, 1, 64, foreign, flag=None, path=path, expected_bytes=int(path == HOST))


def vacant_key(path):
    """every T at 2^64-1, and in the valid part of every foreign slab a 2^64-1 with a count >= m: a vacant slot to the
    kernels, and to the host merge, which must pass it over as they do.  Header word 3 sums to m - 1 = 1 and fewer than s
    qualify, so a 2^64-1 taken from a slab would end the sketch.  HOST: 40 000 foreign values in one bin (flag 1) on a
    sketcher with a 2^16-slot table; TABLE: 65 ranks."""
    rng = np.random.default_rng(640 + path)
    m, s = 2, 1000
    if path == HOST:
        _, shift, region, _, _ = geometry(40_010, MAX64, 6)
        assert 40_000 > 4 * region
        values = (np.uint64(200) << np.uint64(shift)) | _below(rng, 40_000, (1 << shift) - 1)
        n_foreign, per = 5, 8000
    else:
        values = _below(rng, 64 * 40, MAX64 - 1)
        n_foreign, per = 64, 40
    foreign = []
    for r in range(n_foreign):
        mine = values[r * per:(r + 1) * per]
        cnt = np.ones(per, np.uint32)
        cnt[:6] = 2                                       # 6 per rank qualify: 30 or 384 entries, fewer than s
        foreign.append(_rank(rng, np.concatenate([mine, np.array([MAX64], np.uint64)]), np.concatenate([cnt, np.array([m + 3])]), MAX64,
                             maxkey=int(r == 0)))
    return Case(f"vacant-key-{'host' if path == HOST else 'table'}", 21, s, m, n_foreign if path == TABLE else 2, foreign,
                flag=1 if path == HOST else None, path=path, expected_bytes=int(path == HOST))


UNIFORM = [(11, 1, 1, 1 << 40), (12, 2, 2, (1 << 57) + 99), (13, 3, 4, MAX64 - 1), (14, 2, 8, (1 << 33) - 1), (15, 1, 5, 12_345_678_901),
           (16, 3, 3, 1 << 63)]


@functools.lru_cache(maxsize=None)
def all_cases():
    """every case, once per process"""
    out = [uniform(seed, m, R, t, s=1000 if seed % 2 else 200) for seed, m, R, t in UNIFORM]
    for t in T_EDGES:
        if t == MAX64:
            out += [t_min_edge(t, m, maxkey_sum=mk) for m in (1, 2, 3) for mk in (m - 1, m)]
        else:
            out += [t_min_edge(t, m) for m in (1, 2, 3)]
    out += [nbins_step(262_144), nbins_step(262_145)]
    out += [one_bin(TABLE), one_bin(HOST), too_many_qualify(TABLE), too_many_qualify(HOST)]
    out += [compaction(v, m) for v in ("six", "alternate", "span", "overfull") for m in (1, 2)]
    out += [many_ranks(64, 0, 1), many_ranks(64, 63, 2), many_ranks(65, 0, 3), many_ranks(65, 64, 1), many_ranks(70, 63, 2),
            many_ranks(70, 69, 1), many_ranks(70, 64, 3)]
    out += [many_ranks(64, 63, 1, own_reads=300), many_ranks(65, 64, 2, own_reads=300), many_ranks(70, 0, 1, own_reads=300),
            many_ranks(70, 66, 2, own_reads=300)]
    out += [uniform(21, 2, 3, 1 << 62, own_reads=300, own_rank=2, name="uniform-own-reads-m2")]
    out += [counts_exact(m) for m in (1, 2, 3)]
    out += [counts_wrap(n, m) for n in (2, 63, 64) for m in (1, 2)]
    out += [short(BINNED), short(TABLE), short(HOST)]
    out += [vacant_key(HOST), vacant_key(TABLE)]
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return tuple(out)


def by_name(name):
    return next(c for c in all_cases() if c.name == name)
