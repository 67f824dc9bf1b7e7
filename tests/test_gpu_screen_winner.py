"""Winner-take-all for the containment screen (`mash screen -w`) on the GPU against the plain statement of its rule
(tests/screen_winner_rule.py): shared, median and per-entry multiplicities exactly; at file level the rows as
tests/test_gpu_screen.py checks the plain ones, the -i / -v filters, the options struct and the command line."""
import ctypes
import gzip
import math
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from auriclass_amd import engine, screen as screen_cli, synth
from oracle import mash_oracle as mo
from tests import screen_rule as rule
from tests import screen_winner_rule as wrule
from tests.conftest import REFDATA
from tests.test_gpu_screen import PAIR, REF, as_fastq, pack, scenario

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


def check_winner(refs, got, want):
    shared, median, _, counts = got
    for i, (c, sh, med) in enumerate(want):
        assert np.array_equal(counts[i, :len(refs[i])], c), f"reference {i}: multiplicities differ"
        assert not counts[i, len(refs[i]):].any()
        assert (int(shared[i]), int(median[i])) == (sh, med), i


# ---------------------------------------------------------------------------------------------- buffer level
@pytest.mark.parametrize("k,s", [(16, 1000), (27, 50_000), (21, 1000)])
def test_scenario_clade_separates(k, s):
    """32-bit hashes, 64-bit hashes, and a stride of 50 000 with a 5 kb reference far shorter than the stride"""
    refs, own, foreign = scenario(k, s)
    rows, lens = pack(refs)
    fastq = own + foreign
    lengths = [100_000, 100_000, 100_000, 100_000, 5_000]
    h = rule.window_hashes(rule.fastq4_records(fastq), k)
    plain = rule.tally(refs, h)
    want = wrule.winner_tally(refs, h, k, lengths)
    print("plain shared", [p[1] for p in plain], "winner shared", [w[1] for w in want], "medians", [w[2] for w in want])
    # the statement itself shows the feature: the mutated copies lose nearly all, the genomes the reads came from keep theirs
    assert want[1][1] < plain[1][1] / 10 and want[2][1] < plain[2][1] / 10
    assert want[0][1] == plain[0][1] and want[3][1] == plain[3][1] and plain[1][1] > 0.5 * len(refs[1])
    sc = engine.Screener(k, rows, lens, s, with_set_size=False)
    try:
        sc.push_host(fastq, engine.FMT_FASTQ4)
        got = sc.finish(with_counts=True, winner=True, ref_length=lengths)
        check_winner(refs, got, want)
        assert int(got[0].sum()) == wrule.distinct_found(refs, h)
    finally:
        sc.close()


def test_alternating_with_the_plain_finish_repeat_and_reset():
    k, s = 21, 1000
    refs, own, foreign = scenario(k, s)
    rows, lens = pack(refs)
    fastq = own + foreign
    records = rule.fastq4_records(fastq)
    h = rule.window_hashes(records, k)
    plain = rule.tally(refs, h)
    want = wrule.winner_tally(refs, h, k)
    osk = mo.Sketcher(k, s, 1)
    osk.add_fastx(fastq)

    def same_plain(got, times=1):
        shared, median, size, counts = got
        assert size == osk.set_size
        for i, (c, sh, med) in enumerate(plain):
            assert np.array_equal(counts[i, :len(refs[i])], times * c) and int(shared[i]) == sh
            assert times != 1 or int(median[i]) == med

    alone = engine.Screener(k, rows, lens, s)
    sc = engine.Screener(k, rows, lens, s)
    try:
        alone.push_host(fastq, engine.FMT_FASTQ4)
        first = alone.finish(with_counts=True)
        same_plain(first)
        sc.push_host(fastq, engine.FMT_FASTQ4)
        same_plain(sc.finish(with_counts=True))                      # plain before ...
        got = sc.finish(with_counts=True, winner=True)               # (no lengths: all equal)
        check_winner(refs, got, want)
        assert got[2] == osk.set_size                                # the set size is unchanged
        after = sc.finish(with_counts=True)                          # ... and after: what it gives alone
        for x, y in zip(after, first):
            assert np.array_equal(x, y)
        check_winner(refs, sc.finish(with_counts=True, winner=True), want)   # and the winner form again, unchanged
        # the same bytes once more: the same winners, every count doubled
        sc.push_host(fastq, engine.FMT_FASTQ4)
        shared, median, _, counts = sc.finish(with_counts=True, winner=True)
        for i, (c, sh, med) in enumerate(want):
            assert np.array_equal(counts[i, :len(refs[i])], 2 * c) and int(shared[i]) == sh
        same_plain(sc.finish(with_counts=True), times=2)
        # reset, nothing pushed: nobody wins anything
        sc.reset()
        shared, median, size, counts = sc.finish(with_counts=True, winner=True)
        assert size == 0.0 and not shared.any() and not median.any() and not counts.any()
        # ... and after the next push the winners are back
        sc.push_host(fastq, engine.FMT_FASTQ4)
        check_winner(refs, sc.finish(with_counts=True, winner=True), want)
    finally:
        sc.close()
        alone.close()


def test_ties_from_real_sequence():
    """rows [a, a, a[::2]]: identical references tie on the score, the subset ties with them when every hash is found"""
    k, s = 21, 1000
    refs, own, _ = scenario(k, s)
    a = refs[0]
    refs3 = [a, a, a[::2]]
    rows, lens = pack(refs3)
    h = rule.window_hashes(rule.fastq4_records(own), k)
    found = rule.tally([a], h)[0][1]
    assert found == len(a)                                           # the statement: every hash of the genome the reads came from
    sc = engine.Screener(k, rows, lens, s, with_set_size=False)
    try:
        sc.push_host(own, engine.FMT_FASTQ4)
        for lengths, expect in (((5, 9, 9), [0, len(a), 0]),         # the longer genome; among the two of length 9 the lower index
                                ((7, 7, 7), [len(a), 0, 0]),         # all equal: index 0
                                (None, [len(a), 0, 0]),
                                ((5, 5, 9), [len(a) - len(a[::2]), 0, len(a[::2])])):   # the subset is the longest: it takes its half
            want = wrule.winner_tally(refs3, h, k, lengths)
            assert [w[1] for w in want] == expect
            check_winner(refs3, sc.finish(with_counts=True, winner=True, ref_length=lengths), want)
    finally:
        sc.close()


def test_seventy_references_of_sixty_four_entries():
    """more references than a 64-bit mask has bits, heavy sharing, a stride that is no multiple of the workgroup"""
    k, s = 21, 64
    g = synth.make_genome(20_000, seed=77)
    low = mo.bruteforce_sketch([g.tobytes()], k, 300)[0]             # the 300 smallest window hashes
    rng = np.random.default_rng(78)
    refs = [np.sort(rng.choice(low, size=64, replace=False)) for _ in range(70)]
    lengths = rng.integers(1, 4, size=70) * 10_000
    rows, lens = pack(refs)
    half = g[:10_000].tobytes()
    records = [half[i:i + 150] for i in range(0, len(half) - 100, 50)]  # reads over the first half, three deep
    h = rule.window_hashes(records, k)
    want = wrule.winner_tally(refs, h, k, lengths)
    found = wrule.distinct_found(refs, h)
    assert 100 < found < 200 and max(w[2] for w in want) >= 2
    sc = engine.Screener(k, rows, lens, s, with_set_size=False)
    try:
        sc.push_host(as_fastq(records), engine.FMT_FASTQ4)
        got = sc.finish(with_counts=True, winner=True, ref_length=lengths)
        check_winner(refs, got, want)
        assert int(got[0].sum()) == found
        check_winner(refs, sc.finish(with_counts=True, winner=True), wrule.winner_tally(refs, h, k))
    finally:
        sc.close()


# ---------------------------------------------------------------------------------------------- file level
def read_set_expectation(ref, paths, winner):
    k, s = ref.kmer_size, ref.sketch_size
    data = [mo.read_maybe_gz(p) for p in paths]
    osk = mo.Sketcher(k, s, 1)
    for d in data:
        osk.add_fastx(d)
    h = rule.window_hashes(sum((rule.fastx_records(d) for d in data), []), k)
    hashes = [r.hashes for r in ref.references]
    want = wrule.winner_tally(hashes, h, k, [r.length for r in ref.references]) if winner else rule.tally(hashes, h)
    return want, osk.set_size


def check_rows(text, size, ref, want, size_want, keep=None):
    """the rows of `text` against the statement, as test_gpu_screen.check_text; keep: indices of the references expected"""
    assert size == size_want
    rows = rule.rows_of_text(text)
    keep = list(range(len(ref.references))) if keep is None else keep
    assert len(rows) == len(keep)
    k = ref.kmer_size
    for (ident, sh, n, med, p, name, comment), i in zip(rows, keep):
        r, (c, sh_w, med_w) = ref.references[i], want[i]
        assert (sh, n, med, name, comment) == (sh_w, len(r.hashes), med_w, r.name, r.comment)
        assert ident == mo.fmt_g(rule.identity(sh_w, n, k))
        assert rule.same_to_the_sixth_digit(p, float(mo.fmt_g(rule.p_value(sh_w, n, size_want, k))))


@pytest.fixture(scope="module")
def clade(tmp_path_factory):
    """a three-reference clade .msh with distinct genome lengths; the reads of the first genome as a plain and a .gz file"""
    d = tmp_path_factory.mktemp("clade")
    k, s = 21, 1000
    refs, own, _ = scenario(k, s)
    references = [mo.Reference(name, "synthetic", length, h)
                  for name, length, h in zip(("a.fa", "a_mut2.fa", "a_mut10.fa"), (100_000, 100_003, 99_998), refs[:3])]
    msh = d / "clade.msh"
    mo.write_msh(msh, mo.SketchFile(kmer_size=k, sketch_size=s, references=references))
    rb = synth.record_bytes(150)
    cut = (len(own) // rb // 2) * rb
    r1, r2 = d / "s_1.fq", d / "s_2.fq.gz"
    r1.write_bytes(own[:cut])
    r2.write_bytes(gzip.compress(own[cut:], 1))
    ref = mo.read_msh(msh)
    want_w, size = read_set_expectation(ref, [r1, r2], True)
    want_p, _ = read_set_expectation(ref, [r1, r2], False)
    return msh, [r1, r2], ref, want_p, want_w, size


def test_clade_file_winner_rows(clade):
    msh, reads, ref, want_p, want_w, size_want = clade
    assert [w[1] for w in want_w][1:] != [w[1] for w in want_p][1:] and want_w[0][1] == want_p[0][1] == 1000
    text, size = engine.screen_files(msh, reads, winner=True)
    check_rows(text, size, ref, want_w, size_want)
    plain, size = engine.screen_files(msh, reads)
    check_rows(plain, size, ref, want_p, size_want)


def test_fixture_pair_winner_is_what_the_statement_says():
    ref = mo.read_msh(REF)
    want, size_want = read_set_expectation(ref, PAIR, True)
    text, size = engine.screen_files(REF, PAIR, winner=True)
    check_rows(text, size, ref, want, size_want)
    assert sum(w[1] for w in want) == wrule.distinct_found(
        [r.hashes for r in ref.references], rule.window_hashes(sum((rule.fastx_records(mo.read_maybe_gz(p)) for p in PAIR), []), 27))


def test_empty_read_set_winner_rows_equal_the_plain_ones():
    empty = [REFDATA / "test_empty_1.fq.gz", REFDATA / "test_empty_2.fq.gz"]
    text, size = engine.screen_files(REF, empty, winner=True)
    ref = mo.read_msh(REF)
    assert size == 0.0 and (text, size) == engine.screen_files(REF, empty)
    assert text == "".join("0\t0/%d\t0\t1\t%s\t%s\n" % (len(r.hashes), r.name, r.comment) for r in ref.references)


def filtered(text, min_identity=-1.0, max_p=1.0):
    """the lines of the unfiltered text that pass, judged by the columns they print (thresholds lie between the values)"""
    out = []
    for line, row in zip(text.splitlines(True), rule.rows_of_text(text)):
        ident, p = float(row[0]), row[4]
        if (ident > 0.0 if min_identity == 0.0 else ident >= min_identity) and p <= max_p:
            out.append(line)
    return "".join(out)


def test_filters(clade, tmp_path):
    msh, reads, ref, want_p, want_w, _ = clade
    k = ref.kmer_size
    full, _ = engine.screen_files(msh, reads)
    ids = [rule.identity(w[1], len(r.hashes), k) for w, r in zip(want_p, ref.references)]
    assert ids[0] == 1.0 > ids[1] > ids[2] > 0.9                      # the plain clade: three rows close together
    for lo, hi, kept in ((ids[1], ids[0], 1), (ids[2], ids[1], 2), (0.5, ids[2], 3)):
        text, _ = engine.screen_files(msh, reads, min_identity=(lo + hi) / 2)
        assert text == filtered(full, min_identity=(lo + hi) / 2) and len(text.splitlines()) == kept
    # -i 1 keeps a row of full containment (inclusive), and only that
    text, _ = engine.screen_files(msh, reads, min_identity=1.0)
    assert text == full.splitlines(True)[0] and text.startswith("1\t1000/1000\t")
    # a reference set with a zero row: lambda reads against {lambda, T7}
    lam = [REFDATA / "NC_001416.1.fasta.gz"]
    both, _ = engine.screen_files(REF, lam)
    rows = rule.rows_of_text(both)
    assert rows[0][1] == rows[0][2] and rows[1][1] == 0
    assert engine.screen_files(REF, lam, min_identity=0.0)[0] == both.splitlines(True)[0]      # -i 0: identity > 0 only
    assert engine.screen_files(REF, lam, min_identity=-1.0)[0] == both                        # -i -1: every row
    assert engine.screen_files(REF, lam, min_identity=-1.0, max_p_value=0.5)[0] == both.splitlines(True)[0]   # p: 0 and 1
    assert engine.screen_files(REF, lam, min_identity=-1.0, max_p_value=0.0)[0] == both.splitlines(True)[0]   # inclusive
    # the p-values of the winner rows of the clade: thresholds between them
    wfull, _ = engine.screen_files(msh, reads, winner=True)
    ps = sorted({r[4] for r in rule.rows_of_text(wfull)})
    assert len(ps) >= 2
    for lo, hi in zip(ps, ps[1:]):
        mid = math.sqrt(lo * hi) if lo > 0 else hi / 2
        text, _ = engine.screen_files(msh, reads, winner=True, max_p_value=mid)
        assert text == filtered(wfull, max_p=mid) and 0 < len(text.splitlines()) < 3
    # both filters under -w
    text, _ = engine.screen_files(msh, reads, winner=True, min_identity=0.9, max_p_value=0.5)
    assert text == filtered(wfull, 0.9, 0.5) == wfull.splitlines(True)[0]


def call_opts(ref, paths, opts, buf=None, cap=0):
    L = engine.load()
    arr = (ctypes.c_char_p * len(paths))(*[os.fsencode(str(p)) for p in paths])
    need, size = ctypes.c_size_t(0), ctypes.c_double(0)
    rc = L.mhx_screen_files_opts(os.fsencode(str(ref)), arr, len(paths), ctypes.byref(opts) if opts is not None else None, buf, cap,
                                 ctypes.byref(need), ctypes.byref(size))
    return rc, need.value, size.value


def test_options_struct_null_defaults_text_pattern_and_bad_values(clade):
    msh, reads, ref, _, _, _ = clade
    want_text, want_size = engine.screen_files(msh, reads)
    n = len(want_text.encode()) + 1
    size_of = ctypes.sizeof(engine.ScreenOpts)
    assert size_of == 24
    for opts in (None, engine.ScreenOpts(size_of, 0, -1.0, 1.0)):    # NULL and the defaults: mhx_screen_files byte for byte
        buf = ctypes.create_string_buffer(n)
        assert call_opts(msh, reads, opts, buf, n) == (engine.MHX_OK, n, want_size)
        assert buf.raw == want_text.encode() + b"\0"
    # the two-call text pattern under -w
    w = engine.ScreenOpts(size_of, 1, -1.0, 1.0)
    wtext, _ = engine.screen_files(msh, reads, winner=True)
    rc, need, _ = call_opts(msh, reads, w)
    assert (rc, need) == (engine.MHX_OK, len(wtext.encode()) + 1)
    small = ctypes.create_string_buffer(16)
    assert call_opts(msh, reads, w, small, 16)[:2] == (engine.MHX_E_CAPACITY, need)
    buf = ctypes.create_string_buffer(need)
    assert call_opts(msh, reads, w, buf, need)[:2] == (engine.MHX_OK, need) and buf.value.decode() == wtext
    # bad values
    for bad in (engine.ScreenOpts(size_of - 8, 0, -1.0, 1.0), engine.ScreenOpts(0, 0, -1.0, 1.0), engine.ScreenOpts(size_of + 8, 1, -1.0, 1.0),
                engine.ScreenOpts(size_of, 0, 1.5, 1.0), engine.ScreenOpts(size_of, 1, -1.0, -0.1), engine.ScreenOpts(size_of, 0, -1.0, 1.5),
                engine.ScreenOpts(size_of, 0, float("nan"), 1.0), engine.ScreenOpts(size_of, 0, 0.5, float("nan"))):
        assert call_opts(msh, reads, bad)[0] == engine.MHX_E_ARG
    with pytest.raises(engine.EngineError) as e:
        engine.screen_files(msh, reads, min_identity=2.0)
    assert e.value.code == engine.MHX_E_ARG
    with pytest.raises(engine.EngineError) as e:
        engine.screen_files(msh, reads, winner=True, max_p_value=-1.0)
    assert e.value.code == engine.MHX_E_ARG
    # min_identity 1 and max_p_value 0 and 1 are inside the range
    assert call_opts(msh, reads, engine.ScreenOpts(size_of, 1, 1.0, 0.0))[0] == engine.MHX_OK


def test_command_line(clade, tmp_path, capsys):
    msh, reads, ref, _, want_w, size_want = clade
    wfull, _ = engine.screen_files(msh, reads, winner=True)
    env = dict(os.environ, PYTHONPATH=str(ROOT))
    argv = ["-w", "-i", "0.9", "-p", "8", str(msh)] + [str(p) for p in reads]
    r = subprocess.run([sys.executable, "-m", "auriclass_amd.screen"] + argv, capture_output=True, text=True, env=env, cwd=ROOT, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout == filtered(wfull, 0.9) == wfull.splitlines(True)[0]
    check_rows(r.stdout, size_want, ref, want_w, size_want, keep=[0])
    # in this process: the same rows, every row without -i, exit status 1 with the engine's message
    assert screen_cli.main(argv) == 0 and capsys.readouterr().out == r.stdout
    assert screen_cli.main(["-w", str(msh)] + [str(p) for p in reads]) == 0 and capsys.readouterr().out == wfull
    assert screen_cli.main(["-w", str(tmp_path / "none.msh"), str(reads[0])]) == 1
    assert "none.msh" in capsys.readouterr().err
    assert screen_cli.main(["-i", "2", str(msh), str(reads[0])]) == 1
    assert screen_cli.main([str(msh)]) == 1
