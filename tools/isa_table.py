"""Per-kernel table of the device code of one or two source trees: for every kernel of every .hip file in
auriclass_amd/csrc, a digest of its disassembly and the register, LDS and scratch figures of its code object.

    python tools/isa_table.py TREE                 name, digest, vgpr, sgpr, lds, scratch of TREE's kernels
    python tools/isa_table.py PARENT HEAD          the same for HEAD, with "same" / "differs" / "only here" against PARENT;
                                                   every kernel is compared, the k = 1..32 forms that are the same share a row

Every .hip is compiled with the Makefile's flags plus --offload-device-only (objects under TREE/auriclass_amd/csrc/_obj_isa),
unbundled, and read with llvm-objdump -d and llvm-readelf --notes; what of the disassembly is digested: stream().
"""
import hashlib
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

LLVM = Path("/opt/rocm/llvm/bin")
FIELDS = (".vgpr_count", ".sgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size")


def make_var(makefile, name):
    return re.search(rf"^{name} \?= (.*)$", makefile, re.M).group(1).split()


def stream(body, at):
    """The instructions of one function as text: the comment column dropped, the padding behind the last instruction
    dropped, and the literal of a pc-relative address (s_getpc_b64, then s_add_u32 with the distance to a callee, which
    depends on where the linker put the two) replaced by the name of the function it points at, where it points at one."""
    lines, raw, getpc = [], [], None
    for ln in body.splitlines():
        m = re.match(r"\s*(\S.*?)\s*// ([0-9A-F]+): ", ln)
        if not m:
            continue
        ins, addr = m.group(1), int(m.group(2), 16)
        raw.append(ins)
        lit = re.match(r"(s_add_u32 \S+ \S+) (0x[0-9a-f]+|-?\d+)$", ins)
        if getpc is not None and lit:
            target = (getpc + 4 + int(lit.group(2), 0)) & 0xFFFFFFFF
            if target in at:   # any other target (a table in .rodata) keeps its literal and is compared as it stands
                ins = f"{lit.group(1)} <{at[target]}>"
        getpc = addr if ins.startswith("s_getpc_b64") else None
        lines.append(ins)
    while lines and lines[-1] == "s_nop 0":
        lines.pop()
    return lines, raw


def kernels_of(hip, outdir, flags):
    raw, elf = outdir / (hip.stem + ".bundle"), outdir / (hip.stem + ".elf")
    subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", *flags, "--offload-device-only", "-c", str(hip), "-o", str(raw)], check=True)
    subprocess.run([str(LLVM / "clang-offload-bundler"), "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                    f"--input={raw}", f"--output={elf}"], check=True)
    notes = subprocess.run([str(LLVM / "llvm-readelf"), "--notes", str(elf)], check=True, capture_output=True, text=True).stdout
    meta = {}
    for block in notes.split("  - .agpr_count:")[1:]:
        name = re.search(r"^\s+\.name:\s+(\S+)$", block, re.M).group(1)
        meta[name] = [re.search(rf"^\s+{re.escape(f)}:\s+(\d+)$", block, re.M).group(1) for f in FIELDS]
    text = subprocess.run([str(LLVM / "llvm-objdump"), "-d", str(elf)], check=True, capture_output=True, text=True).stdout
    bodies = re.findall(r"^([0-9a-f]+) <(\S+)>:\n(.*?)(?=^[0-9a-f]+ <|\Z)", text, re.M | re.S)
    at = {int(addr, 16): sym for addr, sym, _ in bodies}
    out = {}
    for _, sym, body in bodies:
        if sym in meta:
            norm, raw = (hashlib.sha256("\n".join(t).encode()).hexdigest()[:16] for t in stream(body, at))
            out[sym] = (norm, *meta[sym], hip.name, raw)   # raw: the text as it is, for the count at the end of the table
    assert set(out) == set(meta), (hip, set(meta) - set(out))
    return out


def jobs(tree):
    csrc = Path(tree) / "auriclass_amd" / "csrc"
    mk = (csrc / "Makefile").read_text()
    flags = make_var(mk, "CXXFLAGS") + make_var(mk, "KFLAGS")
    outdir = csrc / "_obj_isa"
    outdir.mkdir(exist_ok=True)
    return [(h, outdir, flags) for h in sorted(csrc.glob("*.hip"))]


def tables(trees):
    work = [(i, j) for i, t in enumerate(trees) for j in jobs(t)]
    out = [{} for _ in trees]
    with ThreadPoolExecutor(4) as ex:
        for (i, _), part in zip(work, ex.map(lambda w: kernels_of(*w[1]), work)):
            assert not set(part) & set(out[i])
            out[i].update(part)
    return out


def fold(rows):
    """Rows that differ only in the first integer template argument (sketch_tile_kernel's k) and all carry the verdict
    "same" become one row: the pattern, how many, a digest of their digests in name order, the register ranges."""
    groups = {}
    for name, row, verdict in rows:
        key = re.sub(r"ILi\d+E", "ILi*E", name, count=1) if verdict == "same" else name
        groups.setdefault((key, row[4:6], verdict), []).append((name, row))
    for (key, rest, verdict), members in groups.items():
        if len(members) == 1:
            yield (members[0][0], *members[0][1][:6], verdict)
            continue
        digest = hashlib.sha256(" ".join(r[0] for _, r in members).encode()).hexdigest()[:16]
        span = [f"{min(v)}-{max(v)}" if min(v) != max(v) else str(v[0]) for v in ([int(r[i]) for _, r in members] for i in (1, 2, 3))]
        yield (f"{key} x{len(members)}", digest, *span, *rest, verdict)


def main():
    trees = tables(sys.argv[1:3])
    head, parent = trees[-1], trees[0] if len(trees) == 2 else None
    print("# kernel  digest  vgpr sgpr lds scratch  file" + ("  verdict" if parent is not None else ""))
    counts, rows = {}, []
    for name in sorted(set(head) | set(parent or {})):
        row = head.get(name) or parent[name]
        verdict = "" if parent is None else "only in parent" if name not in head else "only in head" if name not in parent else \
            "same" if head[name][:5] == parent[name][:5] else "differs (parent: " + " ".join(parent[name][:5]) + ")"
        counts[verdict.split(" (")[0]] = counts.get(verdict.split(" (")[0], 0) + 1
        rows.append((name, row, verdict))
    for out in fold(rows) if parent is not None else ((n, *r[:6]) for n, r, _ in rows):
        print(*out)
    if parent is not None:
        print("# " + ", ".join(f"{v}: {n}" for v, n in sorted(counts.items())))
        moved = sorted(n for n in set(head) & set(parent) if head[n][6] != parent[n][6])
        print(f"# text differs before padding and call distances are taken out: {len(moved)}", *moved[:3], "..." if len(moved) > 3 else "")


if __name__ == "__main__":
    main()
