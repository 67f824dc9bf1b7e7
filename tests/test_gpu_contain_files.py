"""The containment from sketches at file level (mhx_contain_files) and through `python -m auriclass_amd.contain`, against the
rows of the restated rule (tests/contain_rule.py): names and integers exact, identity and p-value to the sixth digit as the
screen's file tests compare them; and the scenario the mode exists for, from sequence: a sample that holds a genome next to
three times as much of something else."""
import numpy as np
import pytest

from auriclass_amd import contain, engine
from oracle import mash_oracle as mo
from tests import contain_cases as cc
from tests import contain_rule as rule

pytestmark = pytest.mark.gpu
K = cc.K


def write(path, prefix, lists, s, k=K, seed=42):
    """one sketch file of the lists cut at s; returns (names, comments, lengths, lists)"""
    lists = [np.asarray(v[:s], np.uint64) for v in lists]
    names = ["%s/genome%d.fasta" % (prefix, i) for i in range(len(lists))]
    comments = ["%s record %d" % (prefix, i) for i in range(len(lists))]
    lengths = [800_000 + 4321 * i + len(prefix) for i in range(len(lists))]
    if seed == 42:
        engine.msh_write(path, k, s, names, comments, lengths, lists)
    else:
        mo.write_msh(path, mo.SketchFile(kmer_size=k, sketch_size=s, hash_seed=seed,
                                         references=[mo.Reference(n, c, l, h) for n, c, l, h in zip(names, comments, lengths, lists)]))
    return names, comments, lengths, lists


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """the `mixed` case as files: a reference file at s = 200, three query files at s = 1000"""
    engine.init()
    d = tmp_path_factory.mktemp("contain")
    qs, rs, s_q, s_r = cc.mixed()
    R = write(d / "ref.msh", "ref", rs, s_r)
    cuts = ((0, 14), (14, 15), (15, 40))
    Q = [write(d / ("q%d.msh" % i), "q%d" % i, qs[a:b], s_q) for i, (a, b) in enumerate(cuts)]
    return d, R, Q


def want_rows(R, Q, which=0, **bounds):
    shared, n_qry, n_ref = cc.expected("mixed")
    names = [n for q in Q for n in q[which]]
    sizes = [l for q in Q for l in q[2]]
    return rule.expected_rows(R[which], names, sizes, shared, n_qry, n_ref, K, **bounds)


def test_text_equals_the_rules_rows(files):
    """a reference file at s = 200 against queries at s = 1000 is accepted; one row per (query, reference) in argument, file
    and reference order"""
    d, R, Q = files
    paths = [d / "q0.msh", d / "q1.msh", d / "q2.msh"]
    text = engine.contain_files(d / "ref.msh", paths)
    want = want_rows(R, Q)
    assert len(want) == 40 * 33 and text.count("\n") == len(want)
    assert rule.same_rows(rule.rows_of_text(text), want)
    for line in text.splitlines()[:40]:
        cols = line.split("\t")
        assert cols[2] == "%g" % float(cols[2]) and cols[3] == "%g" % float(cols[3])
    # the bounds drop exactly the rule's rows
    for bounds in (dict(min_identity=0.9), dict(max_p_value=1e-10), dict(min_identity=1.0, max_p_value=1e-30), dict(min_identity=1.1)):
        cut = want_rows(R, Q, **bounds)
        assert len(cut) < len(want) and (len(cut) > 0) == (bounds.get("min_identity", 0) <= 1.0)
        assert rule.same_rows(rule.rows_of_text(engine.contain_files(d / "ref.msh", paths, **bounds)), cut), bounds
    # comments in place of names
    with_comments = [r for r in want_rows(R, Q, 1) if not r[1].startswith("q0 ")]
    assert len(with_comments) == 26 * 33 and with_comments[0][:2] == ("ref record 0", "q1 record 0")
    assert rule.same_rows(rule.rows_of_text(engine.contain_files(d / "ref.msh", paths[1:], comment=True)), with_comments)


def test_mismatch_is_refused(files, tmp_path):
    d, R, Q = files
    qs = cc.mixed()[0]
    write(tmp_path / "k19.msh", "k19", qs[:3], 1000, k=19)
    with pytest.raises(engine.EngineError) as exc:
        engine.contain_files(d / "ref.msh", [d / "q0.msh", tmp_path / "k19.msh"])
    assert exc.value.code == engine.MHX_E_MISMATCH and "different k-mer sizes" in exc.value.message
    write(tmp_path / "seed7.msh", "seed7", qs[:3], 1000, seed=7)
    with pytest.raises(engine.EngineError) as exc:
        engine.contain_files(d / "ref.msh", [tmp_path / "seed7.msh"])
    assert exc.value.code == engine.MHX_E_MISMATCH and "different hash seeds" in exc.value.message
    write(tmp_path / "s300.msh", "s300", qs[:3], 300)
    with pytest.raises(engine.EngineError) as exc:   # the query files share one sketch size, as everywhere
        engine.contain_files(d / "ref.msh", [d / "q0.msh", tmp_path / "s300.msh"])
    assert exc.value.code == engine.MHX_E_MISMATCH and "different sketch sizes" in exc.value.message
    for bad in (dict(min_identity=float("nan")), dict(max_p_value=float("nan"))):
        with pytest.raises(engine.EngineError) as exc:
            engine.contain_files(d / "ref.msh", [d / "q0.msh"], **bad)
        assert exc.value.code == engine.MHX_E_ARG


def test_command_line_prints_the_same_bytes(files, capsys, tmp_path):
    d, R, Q = files
    ref, q1, q2 = str(d / "ref.msh"), str(d / "q1.msh"), str(d / "q2.msh")
    assert contain.main([ref, q1, q2]) == 0
    assert capsys.readouterr().out == engine.contain_files(ref, [q1, q2])
    assert contain.main(["-i", "0.9", "-v", "1e-10", "-C", "-p", "8", ref, q2]) == 0
    out = capsys.readouterr().out
    assert out == engine.contain_files(ref, [q2], min_identity=0.9, max_p_value=1e-10, comment=True)
    assert rule.same_rows(rule.rows_of_text(out), [r for r in want_rows(R, Q, 1, min_identity=0.9, max_p_value=1e-10) if r[1].startswith("q2 ")])
    fa = tmp_path / "genome.fa"
    fa.write_text(">x\nACGT\n")
    assert contain.main([ref, str(fa)]) == 1
    err = capsys.readouterr()
    assert err.out == "" and "sketch" in err.err and "genome.fa" in err.err
    assert contain.main([ref, str(tmp_path / "missing.msh")]) == 1
    err = capsys.readouterr()
    assert err.out == "" and err.err.strip() != ""


def fasta(path, records):
    with open(path, "w") as f:
        for name, seq in records:
            f.write(">%s\n" % name)
            text = seq.tobytes().decode()
            for i in range(0, len(text), 70):
                f.write(text[i:i + 70] + "\n")


def test_a_contaminated_sample_from_sequence(tmp_path):
    """G: a seeded random 60 kb genome; G': G with 1 % substitutions; U: unrelated.  The sample holds G and a 180 kb unrelated
    record.  All sketched at k = 21, s = 1000.  `mash dist` puts G at a distance above 0.02 from the sample that contains it
    whole; the containment gives shared == n_ref and identity exactly 1."""
    engine.init()
    rng = np.random.default_rng(60180)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    G = rng.choice(acgt, size=60_000)
    Gp = G.copy()
    hit = rng.choice(G.size, size=G.size // 100, replace=False)
    Gp[hit] = acgt[(np.searchsorted(acgt, G[hit]) + rng.integers(1, 4, size=hit.size)) % 4]
    assert (Gp != G).sum() == G.size // 100
    U, other = rng.choice(acgt, size=60_000), rng.choice(acgt, size=180_000)
    for name, recs in (("G", [("G", G)]), ("Gp", [("Gp", Gp)]), ("U", [("U", U)]), ("sample", [("G", G), ("other", other)])):
        fasta(tmp_path / (name + ".fa"), recs)
    k, s = 21, 1000
    engine.sketch_files([tmp_path / "G.fa", tmp_path / "Gp.fa", tmp_path / "U.fa"], k, s, tmp_path / "refs.msh")
    engine.sketch_files([tmp_path / "sample.fa"], k, s, tmp_path / "sample.msh")
    refs, sample = mo.read_msh(tmp_path / "refs.msh"), mo.read_msh(tmp_path / "sample.msh")
    assert len(refs.references) == 3 and len(sample.references) == 1
    rows = rule.rows_of_text(engine.contain_files(tmp_path / "refs.msh", [tmp_path / "sample.msh"]))
    q = rule.the_list(sample.references[0].hashes, len(sample.references[0].hashes), s)
    want = []
    for r in refs.references:
        c, a, b = rule.counts(q, rule.the_list(r.hashes, len(r.hashes), s), s, s)
        want.append((r.name, sample.references[0].name, rule.identity(c, b, k), rule.p_value(c, b, sample.references[0].length, k), c, b, a))
    print(rows)
    assert rule.same_rows(rows, want)          # G' among them
    g, gp, u = rows
    assert g[4] == g[5] > 100 and g[2] == 1.0  # shared == n_ref > 100, identity exactly 1
    assert 0 < gp[4] < gp[5] and 0.9 < gp[2] < 1.0
    assert u[4] == 0 and u[2] == 0.0
    dist = [float(line.split("\t")[2]) for line in engine.dist_files(tmp_path / "refs.msh", tmp_path / "sample.msh").splitlines()]
    assert dist[0] > 0.02                      # the Jaccard path sees a sample four times the reference's size
