"""The device FASTA parser seen at its own output (mhx_fasta_stream / engine.fasta_stream): the dense stream byte for
byte, the separator positions and the total against the plain rule (tests/fasta_rule.py) on the shared case list
(tests/fasta_cases.py, the list the CPU emulator runs in tests/test_fasta_emulation.py), the relaunch with a grown record
list in a fresh process, and the large shapes end to end through the file-level calls."""
import os
import subprocess
import sys

import numpy as np
import pytest

from auriclass_amd import engine
from oracle import mash_oracle as mo
from tests import fasta_cases
from tests.conftest import ROOT
from tests.fasta_rule import not_for_device, rule

pytestmark = pytest.mark.gpu

FOREIGN = fasta_cases.foreign()


def check(name: str, data: bytes, relaunches=None):
    got = engine.fasta_stream(data)
    if not_for_device(data):
        assert got is None, name
        return
    assert got is not None, name
    stream, seps, again = got
    want_stream, want_seps = rule(data)
    assert len(stream) == len(want_stream), name                   # the total
    assert stream == want_stream, name
    assert np.array_equal(seps, np.array(want_seps, dtype=np.uint64)), name
    if relaunches is not None:
        assert again == relaunches, name


@pytest.mark.parametrize("group", list(fasta_cases.GROUPS))
def test_device_parser_equals_the_rule(group):
    """Every case of the list.  A buffer full of line structure goes through in front of every small case, so that the case
    finds foreign '\\n', '>', '@' and '+' bytes directly behind its end in the raw buffer it reuses."""
    check("foreign", FOREIGN)
    for name, data in fasta_cases.GROUPS[group]():
        if len(data) < len(FOREIGN):
            assert engine.fasta_stream(FOREIGN) is not None
        check(name, data)


def relaunch_child():
    """in a process of its own: the record list starts with room for 65 536 positions and only ever grows"""
    cap = fasta_cases.SEPS_CAP
    check("at the capacity", fasta_cases.many_records(cap)[0][1], relaunches=0)
    check("one more", fasta_cases.many_records(cap + 1)[0][1], relaunches=1)
    check("once grown", fasta_cases.many_records(cap + 1)[0][1], relaunches=0)
    print("ok")


def test_record_list_grows_and_the_kernels_run_again():
    env = dict(os.environ, PYTHONPATH=str(ROOT))
    code = "from tests.test_gpu_fasta_stream import relaunch_child; relaunch_child()"
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, cwd=ROOT, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-2000:] + r.stderr[-4000:]


def test_1025_tiles_end_to_end(tmp_path, monkeypatch):
    """two tiles per thread of the offsets pass, through sketch_files: device parser, host record parser and oracle"""
    from tests.test_gpu_fasta import _three_ways

    p = tmp_path / "tiles.fa"
    p.write_bytes(fasta_cases.many_tiles(1025)[0][1])
    osk = _three_ways(tmp_path, [p], 21, 1000, monkeypatch)
    assert osk.references[0].comment.startswith("[")


def test_65537_records_end_to_end(tmp_path, monkeypatch):
    from tests.test_gpu_fasta import _three_ways

    k, nrec = 21, fasta_cases.SEPS_CAP + 1
    p = tmp_path / "records.fa"
    p.write_bytes(fasta_cases.record_file(65, nrec, lo=k, hi=k + 9))
    osk = _three_ways(tmp_path, [p], k, 1000, monkeypatch)
    assert osk.references[0].comment.startswith("[%d seqs] " % nrec)


def test_4097_records_sketched_one_by_one(tmp_path):
    """the separator list past its inline copy feeding sketch_records (`mash sketch -i`): the oracle per record"""
    from tests.test_gpu_sketch_individual import expect

    k, s, nrec = 21, 50, fasta_cases.SEPS_INLINE + 1
    rng = np.random.default_rng(4097)
    lens = rng.integers(15, 61, size=nrec)
    recs = [b">r%d record %d\n" % (i, i) + fasta_cases.acgt(rng, int(L)) + b"\n" for i, L in enumerate(lens)]
    p, out = tmp_path / "records.fa", tmp_path / "i.msh"
    p.write_bytes(b"".join(recs))
    engine.sketch_files([p], k, s, out, individual=True)
    want = expect([recs], k, s)
    assert len(want.references) == int((lens >= k).sum()) < nrec
    assert out.read_bytes() == mo.msh_bytes(want)
