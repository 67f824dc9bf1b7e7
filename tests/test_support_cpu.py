"""What the jackknife support of search hits shows without a GPU: its entry points are declared in include/mhx.h, exported by
the library and bound with argument types; on a machine without a device the compute entry points answer MHX_E_NO_DEVICE (the
engine is checked before any argument); the command line refuses what it can refuse by itself.  CPU only."""
import ctypes

import pytest

from auriclass_amd import engine, search


@pytest.fixture(scope="module")
def lib():
    return engine.load()


def test_symbols_are_declared_exported_and_bound(lib):
    declared = engine.declared_symbols()
    for name in ("mhx_dist_support", "mhx_search_files_support"):
        assert name in declared and hasattr(lib, name)
        assert getattr(lib, name).argtypes and getattr(lib, name).restype is ctypes.c_int
    assert len(lib.mhx_dist_support.argtypes) == 20 and len(lib.mhx_search_files_support.argtypes) == 8
    assert ctypes.sizeof(engine.SearchSupportOpts) == 48 and ctypes.sizeof(engine.SearchOpts) == 24   # the search's own options did not grow
    header = engine.HEADER_PATH.read_text()
    assert "typedef struct mhx_search_support_opts" in header and "MHX_SUPPORT_WORK_MB" in header


def test_clade_table_without_replicates(lib):
    """MHX_E_ARG where there is an engine; without one the engine check comes first"""
    arr = (ctypes.c_char_p * 1)(b"q.msh")
    opts = engine.SearchSupportOpts(ctypes.sizeof(engine.SearchSupportOpts), 5, 1.0, 1.0, 0, 0.5, 42)
    need = ctypes.c_size_t(0)
    rc = lib.mhx_search_files_support(b"ref.msh", arr, 1, ctypes.byref(opts), b"clades.csv", None, 0, ctypes.byref(need))
    err = lib.mhx_last_error()
    assert (rc == engine.MHX_E_ARG and b"replicates" in err) or (rc == engine.MHX_E_NO_DEVICE and b"no GPU engine" in err)


def test_compute_entry_points_need_the_engine(lib):
    """nulls and zeros: no engine -> MHX_E_NO_DEVICE; with one (another test of the process has initialised it) the arguments are refused"""
    for name in ("mhx_dist_support", "mhx_search_files_support"):
        fn = getattr(lib, name)
        args = [None if t in (ctypes.c_char_p, ctypes.c_void_p) or hasattr(t, "contents") else t(0) for t in fn.argtypes]
        rc = fn(*args)
        assert rc in (engine.MHX_E_NO_DEVICE, engine.MHX_E_ARG), name
        assert (rc == engine.MHX_E_NO_DEVICE) == (b"no GPU engine" in lib.mhx_last_error()), name


@pytest.mark.parametrize("argv", [["--keep", "0.5"], ["--seed", "7"], ["--clades", "clades.csv"], ["--support", "-1"], ["--support", "10001"],
                                  ["--support", "x"]])
def test_command_line_refuses(argv, capsys):
    assert search.main(argv + ["ref.msh", "q.msh"]) == 1
    out = capsys.readouterr()
    assert out.out == "" and out.err != ""


def test_command_line_refuses_a_sequence_file(capsys):
    assert search.main(["--support", "8", "ref.msh", "genome.fa"]) == 1
    out = capsys.readouterr()
    assert out.out == "" and "sketch" in out.err and "genome.fa" in out.err
