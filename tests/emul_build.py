"""The CPU emulators of the tests (tests/emul/<name>.cpp -> tests/emul/_<name>.so): built on first use, and again
whenever the source or any header it includes -- as `g++ -MM` lists them -- is newer than the library."""
import ctypes
import subprocess
from pathlib import Path

EMUL = Path(__file__).resolve().parent / "emul"


def load(name, libs=()):
    src, so = EMUL / f"{name}.cpp", EMUL / f"_{name}.so"
    rule = subprocess.run(["g++", "-std=c++17", "-MM", str(src)], check=True, capture_output=True, text=True).stdout
    deps = rule.split(":", 1)[1].replace("\\\n", " ").split()  # (none of these paths holds a blank)
    if not so.exists() or so.stat().st_mtime < max(Path(d).stat().st_mtime for d in deps):
        subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", str(so), str(src), *libs], check=True)
    return ctypes.CDLL(str(so))
