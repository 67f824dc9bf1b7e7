"""What the device FASTA parser (auriclass_amd/csrc/mhx_fasta.h, mhx_fasta.hip) must produce, stated over lines and not
over bits: the dense sequence stream the sketch kernel hashes and the positions of the record separators in it.  The rule
is the oracle's reading of a plain FASTA (oracle/mashcore.c mo_sketch_add_fastx; tests/test_fasta_rule.py ties the two)."""
from typing import List, Tuple

# what a sequence line loses: every byte <= 0x20 (line breaks, CR, blanks, control bytes) and DEL
DROPPED = bytes(range(0x21)) + b"\x7f"


def rule(data: bytes) -> Tuple[bytes, List[int]]:
    """(stream, seps).  The file is split at newlines.  A line whose first byte is '>' is a header: all it contributes is
    its own newline, and that byte's position in the stream is a separator (a last header line without a newline
    contributes nothing).  Every other line contributes its bytes without the DROPPED ones."""
    out, seps, pos = [], [], 0
    lines = data.split(b"\n")
    last = len(lines) - 1          # the piece behind the last newline (empty when the file ends with one) has no newline
    for i, line in enumerate(lines):
        if line[:1] == b">":
            if i < last:
                seps.append(pos)
                out.append(b"\n")
                pos += 1
        else:
            kept = line.translate(None, DROPPED)
            out.append(kept)
            pos += len(kept)
    return b"".join(out), seps


def records(stream: bytes, seps: List[int]) -> List[bytes]:
    """the bytes between consecutive separators (behind the last one: up to the end of the stream)"""
    ends = list(seps[1:]) + [len(stream)]
    return [stream[a + 1:b] for a, b in zip(seps, ends)]


def has_fastq_line(data: bytes) -> bool:
    """some line starts with '@' or '+' (FASTQ syntax to the kseq reader)"""
    return data[:1] in (b"@", b"+") or b"\n@" in data or b"\n+" in data


def not_for_device(data: bytes) -> bool:
    """the file goes to the host record parser: it does not start with '>', or it holds a FASTQ line"""
    return data[:1] != b">" or has_fastq_line(data)
