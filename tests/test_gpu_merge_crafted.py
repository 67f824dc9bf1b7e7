"""The sharded path's merge on crafted slabs (tests/merge_cases.py): the own rank is a real sketcher -- empty, or pushed a
little synthetic FASTQ -- whose header (export_begin) and entries (export_pack) enter the rule as data; every other rank's
header and slab are written by the test.  Each result must equal the rule of tests/merge_rule.py exactly, hashes and counts
or MHX_E_CAPACITY, and the path that produced it (Sketcher.merge_info) must be the one the case is built for: the binned
merge, the table path behind a flag of the binned attempt or behind too many ranks, the host merge behind a table too
small for the foreign entries."""
import dataclasses

import numpy as np
import pytest
import torch

from auriclass_amd import engine, synth
from tests import merge_cases as mc
from tests import merge_rule as mr

pytestmark = pytest.mark.gpu

DEVICE, HOSTMEM, GATHERED = "device slabs", "host slabs", "headers in the slabs"
MAX_EDGE = mr.MAX64 - 1


@pytest.fixture(scope="module")
def reads():
    genome = synth.make_genome(60_000, seed=77)
    return synth.make_fastq(genome, 300, 150, seed=78, device="cpu").numpy()


def own_export(sk):
    """the own rank as data: header from export_begin, entries from export_pack"""
    hdr = sk.export_begin()
    n = int(hdr[0])
    cap = max(2, n + (n & 1))
    slab = np.zeros(cap + cap // 2, np.uint64)
    sk.export_pack(slab.ctypes.data, cap)
    return hdr, slab[:n].copy(), slab[cap:].view(np.uint32)[:n].copy()


def same(a, b):
    if isinstance(a, str) or isinstance(b, str):
        return isinstance(a, str) and isinstance(b, str) and a == b
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def merge(case, reads, form=DEVICE, sk=None):
    """one merge of the case on a sketcher (a fresh one unless given) -> (result, rule's result, merge_info)"""
    made = sk is None
    if made:
        sk = engine.Sketcher(case.k, case.s, case.m, expected_bytes=case.expected_bytes)
    try:
        if case.own_reads:
            assert case.own_reads * synth.record_bytes(150) == reads.size
            sk.push_host(reads, engine.FMT_FASTQ4)
        own = own_export(sk)
        assert bool(case.own_reads) == bool(int(own[0][0]))
        rk = mc.ranks(case, own)
        want = mr.merge(rk, case.k, case.s, case.m)
        if case.own_reads:   # the case sees an own slab counted twice, or passed over where it must not be
            assert not same(mr.merge(rk + [own], case.k, case.s, case.m), want), case.name
            assert not same(mr.merge(mc.ranks(case), case.k, case.s, case.m), want), case.name
        hdr_words = 8 if form == GATHERED else 0
        buf, cap = mc.layout(rk, hdr_words)
        headers = np.stack([h for h, _, _ in rk])
        try:
            if form == HOSTMEM:
                got = sk.merge_slabs(buf.ctypes.data, False, len(rk), cap, headers, case.own_rank)
            else:
                dev = torch.from_numpy(buf.view(np.int64)).cuda()
                torch.cuda.synchronize()
                if form == GATHERED:
                    h, c, need = sk.merge_gathered(dev.data_ptr(), len(rk), cap, case.own_rank)
                    assert need == 0
                    got = (h, c)
                else:
                    got = sk.merge_slabs(dev.data_ptr(), True, len(rk), cap, headers, case.own_rank)
        except engine.EngineError as e:
            assert e.code == engine.MHX_E_CAPACITY, e
            got = mr.CAPACITY
        return got, want, sk.merge_info()
    finally:
        if made:
            sk.close()


def check(case, reads, form=DEVICE, sk=None):
    got, want, info = merge(case, reads, form, sk)
    print(case.name, form, info, "CAPACITY" if isinstance(want, str) else len(want[0]))
    if isinstance(want, str) or isinstance(got, str):
        assert isinstance(want, str) and isinstance(got, str), (case.name, form, got, want)
    else:
        assert np.array_equal(got[0], want[0]), (case.name, form)
        assert np.array_equal(got[1], want[1]), (case.name, form)
    assert info["path"] == case.path, (case.name, form, info)
    assert info["flags"] == case.flag, (case.name, form, info)
    return info


def group(prefix):
    return [c for c in mc.all_cases() if c.name.startswith(prefix)]


@pytest.mark.parametrize("case", group("uniform"), ids=repr)
def test_uniform(case, reads):
    check(case, reads)


@pytest.mark.parametrize("case", group("t_min"), ids=repr)
def test_t_min_edges(case, reads):
    check(case, reads)


@pytest.mark.parametrize("case", group("nbins-step"), ids=repr)
def test_nbins_step(case, reads):
    info = check(case, reads)
    assert info["nbins"] == (256 if case.name.endswith("144") else 512)


@pytest.mark.parametrize("case", group("one-bin") + group("too-many"), ids=repr)
def test_overflow_falls_through(case, reads):
    """flag 1 / flag 4 from the binned attempt, then the table path (a 2^21-slot table) or, on a sketcher whose 2^16-slot
    table the foreign entries would crowd, the host merge"""
    info = check(case, reads)
    assert info["region"] == mc.geometry(sum(int(h[0]) for h, _, _ in case.foreign), 1 << 40, case.n_ranks)[2]


@pytest.mark.parametrize("case", group("compaction"), ids=repr)
def test_compaction(case, reads):
    info = check(case, reads)
    assert info["nbins"] == 1024


@pytest.mark.parametrize("case", group("ranks"), ids=repr)
def test_many_ranks(case, reads):
    check(case, reads)


@pytest.mark.parametrize("case", group("counts"), ids=repr)
def test_count_sums(case, reads):
    check(case, reads)


@pytest.mark.parametrize("case", group("short"), ids=repr)
def test_short_is_capacity_on_every_path(case, reads):
    check(case, reads)
    if case.path == mc.BINNED:                 # ... and from every rank asked
        for own_rank in (0, 1):
            check(dataclasses.replace(case, own_rank=own_rank), reads)


@pytest.mark.parametrize("case", group("vacant-key"), ids=repr)
def test_vacant_key_inside_a_slab(case, reads):
    """2^64-1 below n[r] with T_min = 2^64-1: passed over by the host merge (behind a flagged binned attempt, on a sketcher
    with a 2^16-slot table) and by the table path (65 ranks), or the sketch would end in it"""
    check(case, reads)


SUBSET = ["uniform-seed12-m2-R3-t200000000000063", "uniform-own-reads-m2", "t_min-10000000000-m3", "t_min-ffffffffffffffff-m2-maxkey2",
          "t_min-ffffffff-m1", "compaction-six-m2", "ranks-65-own64-m2-reads", "ranks-70-own66-m2-reads", "ranks-64-own63-m2", "one-bin-table", "counts-wrap-2x-m1",
          "short-binned", "short-host", "vacant-key-host"]


@pytest.mark.parametrize("name", SUBSET)
def test_host_resident_slabs(name, reads):
    check(mc.by_name(name), reads, HOSTMEM)


@pytest.mark.parametrize("name", SUBSET)
def test_headers_inside_the_slabs(name, reads):
    check(mc.by_name(name), reads, GATHERED)


def test_state_after_a_flagged_merge(reads):
    """cursor, qn and flags of the sketcher's merge workspace after a merge that overflowed: the same sketcher, reset(),
    merges a uniform case and then one with more bins, both exactly and with no flag"""
    flagged = dataclasses.replace(mc.one_bin(), m=2)            # (nothing qualifies at m = 2: the table path says so)
    sk = engine.Sketcher(21, 1000, 2)
    try:
        assert check(flagged, reads, sk=sk)["flags"] == 1
        sk.reset()
        small = check(mc.uniform(31, 2, 3, 1 << 40, s=1000), reads, sk=sk)
        sk.reset()
        large = check(mc.by_name("nbins-step-262145"), reads, sk=sk)
        assert (small["nbins"], large["nbins"]) == (256, 512)
        sk.reset()
        check(mc.uniform(32, 2, 5, MAX_EDGE, s=1000), reads, sk=sk)
    finally:
        sk.close()
