"""Batch mode without a GPU (auriclass_amd.batch): the sample sheet and its rules, the batch command line against the
single-sample one (the shared options must be the same definitions), the assembly of report.tsv / failed.tsv from
per-sample outcomes, and the C entry point mhx_dist_files_multi as far as it goes without a device."""
import argparse
import subprocess
import sys

import pytest

from auriclass_amd import batch, engine
from auriclass_amd.args import build_parser
from auriclass_amd.classes import _REPORT_COLUMNS

SHARED = ["fastq", "fasta", "no_qc", "expected_genome_size", "non_candida_threshold", "high_dist_threshold",
          "reference_sketch_path", "clade_config_path", "kmer_size", "sketch_size", "minimal_kmer_coverage", "log_file_path",
          "verbose", "debug", "version"]


# ---- sample sheet ---------------------------------------------------------------------------------------------------
def test_sheet_names_files_comments_blank_lines_and_crlf():
    text = ("# a run\r\n"
            "\r\n"
            "s1\ta_1.fq.gz\ta_2.fq.gz\r\n"
            "   \n"
            "s 2\tdir with blank/asm.fasta\n"
            "#s3\tx\n"
            "\n"
            "isolé.3\tx.fa\ty.fa\tz.fa")                    # no newline at the end of the sheet
    got = batch.parse_sheet(text.encode("utf-8"))
    assert [(s.name, s.files, s.line) for s in got] == [
        ("s1", ["a_1.fq.gz", "a_2.fq.gz"], 3),
        ("s 2", ["dir with blank/asm.fasta"], 5),
        ("isolé.3", ["x.fa", "y.fa", "z.fa"], 8),
    ]
    assert batch.parse_sheet(b"") == [] and batch.parse_sheet(b"# nothing\n\n") == []


def test_read_sheet_reads_the_file(tmp_path):
    sheet = tmp_path / "sheet.tsv"
    sheet.write_bytes(b"a\tx.fa\r\nb\ty_1.fq\ty_2.fq\r\n")
    assert [(s.name, s.files) for s in batch.read_sheet(sheet)] == [("a", ["x.fa"]), ("b", ["y_1.fq", "y_2.fq"])]


@pytest.mark.parametrize("bad, line", [
    (b"ok\tx.fa\n\tx.fa\n", 2),                 # empty name
    (b"# c\nok\tx.fa\nok\ty.fa\n", 3),          # name used twice
    (b"a/b\tx.fa\n", 1),                        # '/' in a name
    (b"ok\tx.fa\n\nn\0ul\tx.fa\n", 3),          # NUL in a name
    (b".\tx.fa\n", 1),
    (b"ok\tx.fa\r\n..\tx.fa\r\n", 2),
    (b"ok\tx.fa\nlonely\n", 2),                 # no file
    (b"ok\tx.fa\nname\tx.fa\t\ty.fa\n", 2),     # an empty file field
    (b"ok\tx.fa\n\xff\xfe\tx.fa\n", 2),         # not UTF-8
])
def test_sheet_rule_violations_name_the_line(bad, line):
    with pytest.raises(ValueError, match=rf"line {line}\b"):
        batch.parse_sheet(bad)


# ---- command line ---------------------------------------------------------------------------------------------------
def _actions(parser):
    return {a.dest: a for a in parser._actions}


def test_batch_parser_shares_the_option_definitions_of_the_single_sample_parser():
    single, many = _actions(build_parser()), _actions(batch.build_batch_parser())
    for dest in SHARED:
        a, b = single[dest], many[dest]
        assert type(a) is type(b), dest
        assert a.option_strings == b.option_strings, dest
        assert (a.default, a.nargs, a.const, a.required, a.help) == (b.default, b.nargs, b.const, b.required, b.help), dest
        if a.type is None or isinstance(a.type, type):
            assert a.type is b.type, dest
        else:       # a range validator: same bounds, seen from outside
            for probe in ("-1", "0", "0.5", "1", "1.5", "32", "33", "100", "101", "999", "1000", "1000000", "1000001", "100000000",
                          "100000001", "x"):
                def outcome(fn):
                    try:
                        return fn(probe)
                    except (argparse.ArgumentTypeError, ValueError) as e:
                        return type(e).__name__, str(e)
                assert outcome(a.type) == outcome(b.type), (dest, probe)
    # every option of the single-sample command is shared but -n / -o, which make no sense for a run of samples
    assert set(single) - set(many) == {"name", "output_report_path", "read_file_paths"}
    assert set(many) - set(single) == {"sample_sheet", "output_dir"}
    d1, d2 = vars(build_parser().parse_args(["x.fq"])), vars(batch.build_batch_parser().parse_args(["sheet.tsv"]))
    for dest in SHARED:
        if dest != "version":
            assert d1[dest] == d2[dest], dest
    assert str(d2["output_dir"]) == "." and str(d2["sample_sheet"]) == "sheet.tsv"
    got = batch.build_batch_parser().parse_args(["sheet.tsv", "-O", "out", "-k", "21", "-s", "1000", "-m", "2", "--fasta"])
    assert (str(got.output_dir), got.kmer_size, got.sketch_size, got.minimal_kmer_coverage, got.fasta) == ("out", "21", "1000", "2", True)


@pytest.mark.parametrize("option, value", [("-k", "0"), ("-k", "33"), ("-s", "999"), ("-s", "1000001"), ("-m", "0"), ("-m", "101")])
def test_both_parsers_refuse_out_of_range_values(option, value, capsys):
    for parser, positional in ((build_parser(), "x.fq"), (batch.build_batch_parser(), "sheet.tsv")):
        with pytest.raises(SystemExit) as ei:
            parser.parse_args([positional, option, value])
        assert ei.value.code == 2
        assert f"Supplied value {value} is not within expected range" in capsys.readouterr().err


@pytest.mark.parametrize("argv", [["sheet.tsv", "-n", "x"], ["sheet.tsv", "-o", "r.tsv"], []])
def test_batch_parser_has_no_name_and_no_report_path_option(argv, capsys):
    with pytest.raises(SystemExit):
        batch.build_batch_parser().parse_args(argv)


# ---- report.tsv / failed.tsv ----------------------------------------------------------------------------------------
def test_reports_are_assembled_from_the_per_sample_files_as_bytes(tmp_path):
    header = "\t".join(_REPORT_COLUMNS) + "\n"
    rows = {"a": "a\tI\t0.0001\tPASS\tPASS\tPASS\tPASS\tPASS\tPASS\n",
            "c": "c\tnot Candida auris\t1.0\tFAIL\tFAIL: distance 1.0 to closest sample is above threshold\tSKIPPED\tSKIPPED\tSKIPPED\tSKIPPED\n",
            "e": "e\tII\t9.55405e-06\tWARN\tPASS\tPASS\tWARN: genome size outside expected range\tPASS\tPASS\n"}
    results = []
    for name in "abcde":
        if name in rows:
            path = tmp_path / f"report.{name}.tsv"
            path.write_bytes((header + rows[name]).encode())
            results.append(batch.SampleResult(name, True, path))
    results.insert(1, batch.SampleResult("b", False, None, "FileNotFoundError", "Required input file nope.fq does not exist"))
    results.insert(3, batch.SampleResult("d", False, None, "ValueError", "two\tcolumns\nand two lines\r\n"))
    assert [r.name for r in results] == list("abcde")
    batch.write_batch_reports(tmp_path, results)
    assert (tmp_path / "report.tsv").read_bytes() == (header + rows["a"] + rows["c"] + rows["e"]).encode()
    assert (tmp_path / "failed.tsv").read_text() == ("Sample\tError\tMessage\n"
                                                     "b\tFileNotFoundError\tRequired input file nope.fq does not exist\n"
                                                     "d\tValueError\ttwo columns and two lines  \n")
    # nothing failed: the header alone; nothing succeeded: the report header alone
    batch.write_batch_reports(tmp_path, [r for r in results if r.ok])
    assert (tmp_path / "failed.tsv").read_text() == "Sample\tError\tMessage\n"
    batch.write_batch_reports(tmp_path, [r for r in results if not r.ok])
    assert (tmp_path / "report.tsv").read_text() == header
    # a per-sample file that is not a report is not copied blindly
    (tmp_path / "report.a.tsv").write_text("something else\n")
    with pytest.raises(ValueError):
        batch.write_batch_reports(tmp_path, results)


# ---- the C entry point ------------------------------------------------------------------------------------------------
def test_library_exports_the_multi_query_call_and_it_needs_an_engine():
    assert "mhx_dist_files_multi" in engine.declared_symbols()
    lib = engine.load()
    assert hasattr(lib, "mhx_dist_files_multi")
    # in a process of its own, where nothing has opened the device (another test of this one may have)
    script = (
        "import ctypes, sys\n"
        "lib = ctypes.CDLL(sys.argv[1])\n"
        "lib.mhx_last_error.restype = ctypes.c_char_p\n"
        "args = [ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t)]\n"
        "lib.mhx_dist_files.argtypes = [ctypes.c_char_p, ctypes.c_char_p] + args\n"
        "lib.mhx_dist_files_multi.argtypes = [ctypes.c_char_p, ctypes.POINTER(ctypes.c_char_p), ctypes.c_int] + args\n"
        "need = ctypes.c_size_t(0)\n"
        "queries = (ctypes.c_char_p * 2)(b'a.msh', b'b.msh')\n"
        "one = lib.mhx_dist_files(b'ref.msh', b'a.msh', None, 0, ctypes.byref(need)), lib.mhx_last_error()\n"
        "many = lib.mhx_dist_files_multi(b'ref.msh', queries, 2, None, 0, ctypes.byref(need)), lib.mhx_last_error()\n"
        "print(one[0], many[0], one[1] == many[1])\n")
    out = subprocess.run([sys.executable, "-c", script, str(engine.LIB_PATH)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    assert out.stdout.split() == [str(engine.MHX_E_NO_DEVICE), str(engine.MHX_E_NO_DEVICE), "True"]
