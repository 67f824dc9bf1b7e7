"""What the containment from sketches shows without a GPU: its entry points are declared in include/mhx.h, exported by the
library and bound with argument types; on a machine without a device they answer MHX_E_NO_DEVICE (the engine is checked
before any argument); the command line refuses what it can refuse by itself.  CPU only."""
import ctypes

import numpy as np
import pytest
import torch

from auriclass_amd import contain, engine

HAVE_GPU = torch.cuda.is_available()


@pytest.fixture(scope="module")
def lib():
    return engine.load()


def test_symbols_are_declared_exported_and_bound(lib):
    declared = engine.declared_symbols()
    for name in ("mhx_dist_contain", "mhx_contain_files"):
        assert name in declared and hasattr(lib, name)
        assert getattr(lib, name).argtypes and getattr(lib, name).restype is ctypes.c_int
    assert len(lib.mhx_dist_contain.argtypes) == 13 and len(lib.mhx_contain_files.argtypes) == 7
    assert ctypes.sizeof(engine.ContainOpts) == 24
    assert "typedef struct mhx_contain_opts" in engine.HEADER_PATH.read_text()


def test_c_entry_points_need_the_engine(lib):
    """nulls and zeros: no engine -> MHX_E_NO_DEVICE; with one (another test of the process has initialised it) the arguments are refused"""
    for name in ("mhx_dist_contain", "mhx_contain_files"):
        fn = getattr(lib, name)
        args = [None if t in (ctypes.c_char_p, ctypes.c_void_p) or hasattr(t, "contents") else t(0) for t in fn.argtypes]
        rc = fn(*args)
        assert rc in (engine.MHX_E_NO_DEVICE, engine.MHX_E_ARG), name
        assert (rc == engine.MHX_E_NO_DEVICE) == (b"no GPU engine" in lib.mhx_last_error()), name


@pytest.mark.skipif(HAVE_GPU, reason="checks the no-GPU behaviour")
def test_the_three_python_entry_points_fail_loudly_without_a_gpu(lib, capsys):
    q = np.arange(1, 33, dtype=np.uint64).reshape(2, 16)
    calls = (lambda: engine.dist_contain(q, [16, 16], q, [16, 16], 16, 16),
             lambda: engine.dist_contain_device(0, 0, 1, 16, 0, 0, 1, 16, 16, 0, 0, 0),
             lambda: engine.contain_files("ref.msh", ["q.msh"]))
    for call in calls:
        with pytest.raises(engine.EngineError) as e:
            call()
        assert e.value.code == engine.MHX_E_NO_DEVICE
    assert contain.main(["ref.msh", "q.msh"]) == 1   # exit status 1 with the engine's message
    out = capsys.readouterr()
    assert out.out == "" and out.err.strip() != ""


@pytest.mark.parametrize("argv", [["-i", "x"], ["-v", "x"], ["--top", "3"], []])
def test_command_line_refuses(argv, capsys):
    assert contain.main(argv + ["ref.msh"]) == 1   # (and a single path: no query)
    out = capsys.readouterr()
    assert out.out == "" and out.err != ""


def test_command_line_refuses_a_sequence_file(capsys):
    for argv in (["ref.msh", "genome.fa"], ["-p", "4", "genome.fa", "q.msh"]):
        assert contain.main(argv) == 1
        out = capsys.readouterr()
        assert out.out == "" and "sketch" in out.err and "genome.fa" in out.err
