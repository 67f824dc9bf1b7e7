"""The rule of `mash screen` (Mash 2.x CommandScreen, nucleotides, no -w) as a plain statement, built from pieces of the
CPU oracle that exist for the sketch path: every window hash of every record, counted; looked up per reference hash.
Shared by the screen tests; not a test module itself.

    count(h)   = number of windows (k bytes A/C/G/T inside one record) whose canonical hash is h
    shared_i   = number of h in H_i with count(h) >= 1
    median_i   = element [len / 2] of the ascending list of those counts (0: none)
    identity_i = 1 if shared_i == n_i, 0 if shared_i == 0, else (shared_i / n_i) ** (1 / k)
    p_i        = 1 if shared_i == 0, else P[Binomial(n_i, r) >= shared_i], r = 1 / (1 + 4^k / floor(set_size))
    set_size   = oracle.Sketcher(k, s_ref, 1).set_size over the same input
"""
import ctypes
import math

import numpy as np

from oracle import mash_oracle as mo


def window_hashes(records, k):
    """all window hashes of the records (bytes objects), concatenated"""
    parts = []
    for seq in records:
        if len(seq) < k:
            continue
        out = np.zeros(len(seq), dtype=np.uint64)
        buf = ctypes.create_string_buffer(seq, len(seq))
        n = mo.lib().mo_all_window_hashes(buf, len(seq), k, out.ctypes.data)
        parts.append(out[:n])
    return np.concatenate(parts) if parts else np.zeros(0, np.uint64)


def fastq4_records(data: bytes):
    """sequence lines of strict 4-line FASTQ (one '\\r' before the newline dropped)"""
    lines = data.split(b"\n")
    return [s[:-1] if s.endswith(b"\r") else s for s in lines[1::4]]


def fastx_records(data: bytes):
    """records of a FASTA (multi-line) or 4-line FASTQ file"""
    if data[:1] == b">":
        recs = []
        for chunk in data.split(b">")[1:]:
            lines = chunk.split(b"\n")
            recs.append(b"".join(s.rstrip(b"\r") for s in lines[1:]))
        return recs
    return fastq4_records(data)


def tally(ref_hashes, hashes):
    """per reference: (counts per entry, shared, median) from the window hashes of the read set"""
    values, occ = np.unique(hashes, return_counts=True)
    out = []
    for H in ref_hashes:
        H = np.asarray(H, dtype=np.uint64)
        c = np.zeros(H.size, dtype=np.uint32)
        if values.size and H.size:
            at = np.searchsorted(values, H)
            at_c = np.minimum(at, values.size - 1)
            hit = (at < values.size) & (values[at_c] == H)
            c[hit] = occ[at_c[hit]]
        nz = np.sort(c[c > 0])
        out.append((c, int(nz.size), int(nz[nz.size // 2]) if nz.size else 0))
    return out


def identity(shared: int, n: int, k: int) -> float:
    if shared == n:
        return 1.0
    if shared == 0:
        return 0.0
    return math.pow(shared / n, 1.0 / k)


def p_value(shared: int, n: int, set_size: float, k: int) -> float:
    from scipy.stats import binom

    if shared == 0:
        return 1.0
    size = float(math.floor(set_size))
    r = 1.0 / (1.0 + 4.0 ** k / size) if size > 0 else 0.0
    return float(binom.sf(shared - 1, n, r))


def same_to_the_sixth_digit(a: float, b: float) -> bool:
    """the two values differ by at most one in the sixth significant digit (the resolution of a %g column); two values
    below 1e-300 count as equal (scipy flushes there)"""
    if a < 1e-300 and b < 1e-300:
        return True
    if a <= 0.0 or b <= 0.0:
        return False

    def sig6(x):
        m, e = ("%.5e" % x).split("e")
        return int(m.replace(".", "")), int(e)

    (ma, ea), (mb, eb) = sig6(a), sig6(b)
    if ea == eb:
        return abs(ma - mb) <= 1
    if abs(ea - eb) != 1:
        return False
    hi, lo = (ma, mb) if ea > eb else (mb, ma)
    return abs(hi * 10 - lo) <= 1


def rows_of_text(text: str):
    """[(identity str, shared, n, median, p float, name, comment)]"""
    rows = []
    for line in text.splitlines():
        ident, frac, med, p, name, comment = line.split("\t")
        s, n = frac.split("/")
        rows.append((ident, int(s), int(n), int(med), float(p), name, comment))
    return rows
