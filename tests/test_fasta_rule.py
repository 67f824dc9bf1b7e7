"""The plain statement of what the device FASTA parser must produce (tests/fasta_rule.py) against the oracle
(oracle/mashcore.c mo_sketch_add_fastx): a Sketcher fed the whole file and one fed the rule's records one by one hold the
same hashes, length and record count.  k is small and s larger than the number of windows, so that the whole k-mer set is
compared and not a sample of it."""
import numpy as np
import pytest

from oracle import mash_oracle as mo
from tests import fasta_cases
from tests.fasta_rule import has_fastq_line, not_for_device, records, rule

KS = (1, 3, 5, 8)
ALPHABET = np.frombuffer(b"ACGTacgtN\n\n\n>>\r \t\x7f\x00\x80\xff", np.uint8)


def oracle_equals_rule(data: bytes, k: int):
    stream, seps = rule(data)
    recs = records(stream, seps)
    s = len(stream) + 1
    whole, parts = mo.Sketcher(k, s), mo.Sketcher(k, s)
    whole.add_fastx(data)
    for r in recs:
        parts.add_seq(r)
    assert np.array_equal(whole.finish()[0], parts.finish()[0])
    counted = [len(r) for r in recs if len(r) >= k]       # mash does not count a record shorter than k
    assert whole.records == len(counted) and whole.length == sum(counted)


def test_rule_by_hand():
    assert rule(b">a\nAC\nGT\n>b x\nA C\r\n") == (b"\nACGT\nAC", [0, 5])
    assert records(b"\nACGT\nAC", [0, 5]) == [b"ACGT", b"AC"]
    assert rule(b">a\n>b\n\n>c") == (b"\n\n", [0, 1]) and records(b"\n\n", [0, 1]) == [b"", b""]
    assert rule(b">") == (b"", []) and rule(b">\n") == (b"\n", [0]) and rule(b"") == (b"", [])
    assert rule(b">a\nA>C\n\r>G\x7f\x00\x80\n") == (b"\nA>C>G\x80", [0])
    assert not not_for_device(b">a\nAC@+\n") and not has_fastq_line(b">a\nAC@+\n")
    for data in (b"", b"\n>a\nAC\n", b"ACGT\n", b">a\n+\n", b">a\nAC\n@", b"@a\nAC\n"):
        assert not_for_device(data), data
    assert has_fastq_line(b">a\n+") and not has_fastq_line(b"\n>a\nAC\n")


def test_rule_is_the_oracles_on_random_files():
    rng = np.random.default_rng(201)
    refused = 0
    for trial in range(3000):
        data = b">" + rng.choice(ALPHABET, size=int(rng.integers(0, 200))).tobytes()
        refused += not_for_device(data)
        oracle_equals_rule(data, KS[trial % 4])
    assert refused == 0


@pytest.mark.parametrize("group", ["tiny", "edges", "long_lines", "dense", "alphabet", "ends", "fastq", "fuzz"])
def test_rule_is_the_oracles_on_the_case_list(group):
    """the small groups of the shared list (the large files repeat their structure: the emulator and the GPU take them)"""
    compared = 0
    for i, (name, data) in enumerate(fasta_cases.GROUPS[group]()):
        if not_for_device(data):
            continue
        try:
            oracle_equals_rule(data, KS[i % 4])
        except AssertionError as e:
            raise AssertionError(name) from e
        compared += 1
    assert compared >= 5
