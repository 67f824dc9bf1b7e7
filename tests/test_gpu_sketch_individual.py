"""`mash sketch -i` (mhx_sketch_files_individual): one reference per record.  No mash output is recorded for this mode, so
it is pinned by the oracle applied record by record: every record goes to an oracle Sketcher of its own, and the .msh must
be, byte for byte, oracle.msh_bytes of those references (name / comment = first_name / first_comment, length = the record's
length; a record shorter than k left out, a record of >= k bytes without a valid window kept with an empty list)."""
import gzip

import numpy as np
import pytest

from auriclass_amd import engine, mash_shim
from oracle import mash_oracle as mo
from tests.conftest import REFDATA

pytestmark = pytest.mark.gpu

K, S = 21, 1000


def _acgt(rng, n):
    return bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), size=n))


def _wrap(seq: bytes, width: int) -> bytes:
    return b"\n".join(seq[i:i + width] for i in range(0, len(seq), width))


def expect(files, k, s) -> mo.SketchFile:
    """files: per file the list of its records' texts"""
    out = mo.SketchFile(kmer_size=k, sketch_size=s)
    for recs in files:
        for text in recs:
            sk = mo.Sketcher(k, s, 1)
            sk.add_fastx(text)
            if sk.records == 0:          # shorter than k (or no sequence at all): mash does not count it
                continue
            hashes, _ = sk.finish()
            out.references.append(mo.Reference(sk.first_name, sk.first_comment, int(sk.length), hashes, None))
    return out


def records(seed=1, k=K):
    rng = np.random.default_rng(seed)
    return [
        b">plasmid_1 first record, one line\n" + _acgt(rng, 2500) + b"\n",
        b">locus_2\twrapped at 60\n" + _wrap(_acgt(rng, 1234), 60) + b"\n",
        b">tiny shorter than k\n" + _acgt(rng, k - 1) + b"\n",
        b">all_n nothing to hash\n" + b"N" * 300 + b"\n",
        b">lower_3 mixed case and an N run\n" + _wrap(_acgt(rng, 700).lower() + b"NNNNNNNN" + _acgt(rng, 650), 70) + b"\n",
        b">nocomment\n" + _wrap(_acgt(rng, 5200), 80) + b"\n",          # above the cut: the sketcher route
        b">exactly_k\n" + _acgt(rng, k) + b"\n",
        b">last_one has a comment\n" + _wrap(_acgt(rng, 400), 61) + b"\n",
    ]


def sketch_i(tmp_path, paths, k=K, s=S, name="i.msh"):
    out = tmp_path / name
    text, _ = engine.sketch_files(paths, k, s, out, individual=True)
    return out, text


def test_multi_fasta_against_the_oracle_per_record(tmp_path):
    recs = records()
    p = tmp_path / "multi.fa"
    p.write_bytes(b"".join(recs))
    out, text = sketch_i(tmp_path, [p])
    want = expect([recs], K, S)
    assert [r.name for r in want.references] == ["plasmid_1", "locus_2", "all_n", "lower_3", "nocomment", "exactly_k", "last_one"]
    assert want.references[2].hashes.size == 0 and want.references[2].length == 300
    assert out.read_bytes() == mo.msh_bytes(want)
    assert text == f"Sketching {p}...\nWriting to {out}...\n"
    n = np.zeros(1, np.uint64)
    arr = (engine.ctypes.c_char_p * 1)(str(p).encode())
    assert engine.load().mhx_sketch_files_individual(arr, 1, K, S, str(out).encode(), None, 0, None,
                                                     n.ctypes.data_as(engine.ctypes.POINTER(engine.ctypes.c_uint64))) == 0
    assert int(n[0]) == 7


@pytest.mark.parametrize("k,s", [(16, 50), (17, 1000), (32, 10)])
def test_crlf_dangling_header_gz_and_two_files(tmp_path, k, s):
    recs = records(seed=k, k=k)
    crlf = [r.replace(b"\n", b"\r\n") for r in recs]
    dangling = recs[:3] + [b">dangling header without newline"]
    a, b, c = tmp_path / "crlf.fa", tmp_path / "dangling.fa.gz", tmp_path / "plain.fa"
    a.write_bytes(b"".join(crlf))
    b.write_bytes(gzip.compress(b"".join(dangling)))
    c.write_bytes(b"".join(recs[4:]))
    out, text = sketch_i(tmp_path, [a, b, c], k, s)
    assert out.read_bytes() == mo.msh_bytes(expect([crlf, dangling, recs[4:]], k, s))
    assert text == "".join(f"Sketching {p}...\n" for p in (a, b, c)) + f"Writing to {out}...\n"


def test_golden_genomes_as_one_two_record_file(tmp_path):
    """both records are far above the cut: the seam to the existing sketcher at file level"""
    texts = [gzip.decompress((REFDATA / n).read_bytes()) for n in ("NC_001416.1.fasta.gz", "NC_001604.1.fasta.gz")]
    assert all(t.count(b">") == 1 and t.endswith(b"\n") for t in texts)
    p = tmp_path / "two.fasta"
    p.write_bytes(b"".join(texts))
    out, _ = sketch_i(tmp_path, [p])
    want = expect([texts], K, S)
    assert len(want.references) == 2 and all(r.length > engine.sketch_segments_cut() + K for r in want.references)
    assert out.read_bytes() == mo.msh_bytes(want)
    # the per-file sketch of either genome alone holds the same hashes as its record
    for i, n in enumerate(("NC_001416.1.fasta.gz", "NC_001604.1.fasta.gz")):
        engine.sketch_files([REFDATA / n], K, S, tmp_path / "one.msh")
        assert np.array_equal(mo.read_msh(tmp_path / "one.msh").references[0].hashes, want.references[i].hashes)


def test_fastq_and_headless_fasta_take_the_record_parser_and_agree(tmp_path, monkeypatch):
    rng = np.random.default_rng(7)
    seqs = [(b"r1 first", _acgt(rng, 900)), (b"r2", _acgt(rng, K - 2)), (b"r3 third one", _acgt(rng, 4500)), (b"r4\tx", b"N" * 50 + _acgt(rng, 200))]
    fasta = [b">" + h + b"\n" + _wrap(q, 70) + b"\n" for h, q in seqs]
    fastq = [b"@" + h + b"\n" + q + b"\n+\n" + b"I" * len(q) + b"\n" for h, q in seqs]
    pa, pq, ph = tmp_path / "twin.fa", tmp_path / "twin.fq", tmp_path / "headless.fa"
    pa.write_bytes(b"".join(fasta))
    pq.write_bytes(b"".join(fastq))
    ph.write_bytes(b"\n" + b"".join(fasta))                                 # does not start with '>': not for the device parser
    want = mo.msh_bytes(expect([fasta], K, S))
    assert mo.msh_bytes(expect([fastq], K, S)) == want
    for p in (pa, pq, ph):
        out, _ = sketch_i(tmp_path, [p], name=p.name + ".msh")
        assert out.read_bytes() == want, p.name
    monkeypatch.setenv("MHX_HOST_FASTA", "1")                               # the plain FASTA through the host route as well
    out, _ = sketch_i(tmp_path, [pa], name="forced.msh")
    assert out.read_bytes() == want


def test_file_without_a_record_left_fails(tmp_path):
    p, q = tmp_path / "short.fa", tmp_path / "good.fa"
    p.write_bytes(b">a\nACGT\n>b\n" + b"ACGTACGTAC\n>c")
    q.write_bytes(records()[0])
    with pytest.raises(engine.NoRecordsError) as e:
        sketch_i(tmp_path, [q, p])
    assert e.value.message == f'ERROR: Did not find fasta records in "{p}".'
    (tmp_path / "empty.fa").write_bytes(b"")
    with pytest.raises(engine.NoRecordsError):
        sketch_i(tmp_path, [tmp_path / "empty.fa"])
    with pytest.raises(ValueError):
        engine.sketch_files([q], K, S, tmp_path / "x.msh", reads=True, individual=True)


def test_shim_sketch_i_and_its_refusal_of_r(tmp_path, capsys):
    recs = records(seed=3)
    p = tmp_path / "multi.fa"
    p.write_bytes(b"".join(recs))
    out, text = sketch_i(tmp_path, [p])
    assert mash_shim.main(["sketch", "-i", "-k", str(K), "-s", str(S), "-o", str(tmp_path / "shim"), str(p)]) == 0
    assert (tmp_path / "shim.msh").read_bytes() == out.read_bytes()
    assert capsys.readouterr().err == text.replace(str(out), str(tmp_path / "shim.msh"))
    assert mash_shim.main(["sketch", "-i", "-r", "-o", str(tmp_path / "no"), str(p)]) == 1
    assert capsys.readouterr().err.startswith("ERROR:") and not (tmp_path / "no.msh").exists()


def test_dist_and_screen_read_the_individual_sketch(tmp_path):
    rng = np.random.default_rng(11)
    genomes = [_acgt(rng, n) for n in (3000, 1800, 6000, 2500)]
    recs = [b">g%d record %d\n" % (i, i) + _wrap(g, 80) + b"\n" for i, g in enumerate(genomes)]
    p = tmp_path / "refs.fa"
    p.write_bytes(b"".join(recs))
    out, _ = sketch_i(tmp_path, [p])
    rows = engine.dist_files(out, out).splitlines()
    n = len(genomes)
    assert len(rows) == n * n
    for qi in range(n):
        for ri in range(n):
            ref, qry, dist, _, frac = rows[qi * n + ri].split("\t")
            assert (ref, qry) == (f"g{ri}", f"g{qi}")
            if qi == ri:
                assert dist == "0" and frac.split("/")[0] == frac.split("/")[1]
    # reads drawn from genome 2 only: one screen row per record, in order, and genome 2 is the one that is contained
    reads = b"".join(b"@r%d\n" % j + genomes[2][o:o + 150] + b"\n+\n" + b"I" * 150 + b"\n" for j, o in enumerate(range(0, 5851, 30)))
    (tmp_path / "reads.fq").write_bytes(reads)
    text, _ = engine.screen_files(out, [tmp_path / "reads.fq"])
    srows = [r.split("\t") for r in text.splitlines()]
    assert [r[4] for r in srows] == [f"g{i}" for i in range(n)] and [r[5] for r in srows] == [f"record {i}" for i in range(n)]
    shared = [int(r[1].split("/")[0]) for r in srows]
    assert shared[2] == int(srows[2][1].split("/")[1]) and max(shared[:2] + shared[3:]) < 5
